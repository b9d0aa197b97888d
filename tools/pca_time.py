#!/usr/bin/env python3
"""PCA timing (GPU box): the device work of a fit (msst_feat_moments + msst_feat_moments_finish, twice: the centred two-pass
covariance) and of a projection (msst_feat_project: scores and their squared norm) against the eager restatements, and the
feature-side work of anomaly_scene on a map.

Per shape -- M rows [M, 96] with a mean of 50 per channel, r directions:
  fit       hip: the four launches of fit_pca, no read-back.  eager: mu = x.mean(0); xc = x - mu; xc.T @ xc / (M - 1).
  project   hip: one launch, out [M, r] and sumsq [M].  eager: z = (x - mu) @ W.T; z.square().sum(1).
The moments launch and the finish launch are also timed apart; with the moments launch goes the rate at which it streams the rows
(4 x 96 M bytes).  The last row is the feature side of anomaly_scene on four 64 x 64 scenes (the encoder pass, common to both sides,
is left out): the map [4, 96, 64, 64] with uncovered (NaN) pixels read in place -- fit and Mahalanobis score -- against torch.cov
on the permuted and gathered map and the eager score.  Both sides are warmed up, then timed alternately in one process between
device events (the device time of the queued launches, as in tools/kmeans_time.py); the medians of --runs runs are reported.  No
speed bar hangs on this tool; every shape is reported, the ones eager wins included.  Prints ONE JSON line per shape and appends it
to --append (default profiles/pca_measured.jsonl; '' to skip).  --smoke: the smallest shape alone, two runs, nothing appended.

Run:  python tools/pca_time.py [--rows 8192,262144] [--components 3,96] [--runs 20]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from maskedsst_amd import _lib  # noqa: E402
from maskedsst_amd import pca as P  # noqa: E402
from maskedsst_amd.features import _p, _stream  # noqa: E402

SEED = 5
REPEAT = 10     # calls queued between two events: a single call is a few microseconds


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPEAT):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / REPEAT


def alternate(fast, slow, runs, warmup):
    for _ in range(warmup):
        fast()
        slow()
    a, b = [], []
    for _ in range(runs):
        a.append(event_ms(fast))
        b.append(event_ms(slow))
    return 1e3 * statistics.median(a), 1e3 * statistics.median(b)      # microseconds


def hip_fit(x):
    first = P.feature_moments(x, None, 1, cov=False)
    return P.feature_moments(x, first.mean, 1)


def eager_fit(x):
    mu = x.mean(0)
    xc = x - mu
    return mu, xc.t() @ xc / (x.shape[0] - 1)


def shape_row(M, r, args, gen, device):
    lib = _lib.load()
    x = (torch.randn(M, 96, generator=gen) * torch.exp(-torch.arange(96) / 24.0) + 50.0).to(device).contiguous()
    mu = x.mean(0).contiguous()
    w = torch.linalg.qr(torch.randn(96, r, generator=gen, dtype=torch.float64))[0].t().float().to(device).contiguous()
    nslab = int(lib.msst_feat_moments_scratch_floats(M))
    slab = torch.empty(nslab, device=device)
    buf = torch.empty(2 + 96 + 96 * 96, device=device)
    count, mean, cov = buf[:2].view(torch.int64), buf[2:98], buf[98:]

    def moments_only():
        _lib.check(lib.msst_feat_moments(_p(x), 0, M, 1, 96, _p(mu), _p(slab), nslab, _stream()), "msst_feat_moments")

    def finish_only():
        _lib.check(lib.msst_feat_moments_finish(_p(slab), nslab, M, 96, _p(mu), 1, _p(count), _p(mean), _p(cov), None, _stream()),
                   "msst_feat_moments_finish")

    def eager_project():
        z = (x - mu) @ w.t()
        return z, z.square().sum(1)

    fit_hip, fit_eager = alternate(lambda: hip_fit(x), lambda: eager_fit(x), args.runs, args.warmup)
    mom_us, fin_us = alternate(moments_only, finish_only, max(3, args.runs // 2), 1)      # the two launches apart
    proj_hip, proj_eager = alternate(lambda: P.feature_project(x, mu, w, sumsq=True), eager_project, args.runs, args.warmup)
    ss_hip, ss_eager = alternate(lambda: P.feature_project(x, mu, w, out=False, sumsq=True), lambda: eager_project()[1], args.runs, args.warmup)
    return dict(tool="pca_time", M=M, r=r, runs=args.runs, fit_us=round(fit_hip, 2), eager_fit_us=round(fit_eager, 2),
                moments_launch_us=round(mom_us, 2), finish_launch_us=round(fin_us, 2), slab_MB=round(4e-6 * nslab, 2),
                moments_rows_GBps=round(M * 96 * 4 / (mom_us * 1e-6) / 1e9, 1), moments_share_of_fit=round(2 * mom_us / fit_hip, 3),
                project_us=round(proj_hip, 2), eager_project_us=round(proj_eager, 2), sumsq_only_us=round(ss_hip, 2),
                eager_sumsq_us=round(ss_eager, 2),
                eager_faster=dict(fit=bool(fit_eager < fit_hip), project=bool(proj_eager < proj_hip), sumsq=bool(ss_eager < ss_hip)))


def scene_row(args, gen, device):
    """the feature side of anomaly_scene(pca=None) on four 64 x 64 scenes: a map with a band of uncovered pixels"""
    Bs, H, W = 4, 64, 64
    m = torch.randn(Bs, 96, H, W, generator=gen) * torch.exp(-torch.arange(96) / 24.0).view(1, 96, 1, 1) + 50.0
    m[:, :, 60:, :] = float("nan")
    m[:, :, :, 60:] = float("nan")
    m = m.to(device).contiguous()
    cover = ~torch.isnan(m[:, 0])
    fitted = P.fit_pca(m)
    mean, white = fitted._device_tables(device, True)

    def eager_map_fit():
        rows = m.permute(0, 2, 3, 1)[cover]
        return rows.mean(0), torch.cov(rows.t())

    def eager_rx():
        z = (m.permute(0, 2, 3, 1).reshape(-1, 96) - mean) @ white.t()
        return z.square().sum(1)

    fit_hip, fit_eager = alternate(lambda: hip_fit(m), eager_map_fit, args.runs, args.warmup)
    rx_hip, rx_eager = alternate(lambda: P.feature_project(m, mean, white, out=False, sumsq=True), eager_rx, args.runs, args.warmup)
    return dict(tool="pca_time", scene=f"{Bs}x{H}x{W}", covered=int(cover.sum()), runs=args.runs, map_fit_us=round(fit_hip, 2),
                eager_map_fit_us=round(fit_eager, 2), rx_us=round(rx_hip, 2), eager_rx_us=round(rx_eager, 2),
                eager_faster=dict(map_fit=bool(fit_eager < fit_hip), rx=bool(rx_eager < rx_hip)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="8192,262144", help="comma separated row counts M")
    ap.add_argument("--components", default="3,96", help="comma separated direction counts r")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--append", default=os.path.join(ROOT, "profiles", "pca_measured.jsonl"))
    ap.add_argument("--smoke", action="store_true", help="the smallest shape alone, two runs, nothing appended")
    args = ap.parse_args()
    if args.smoke:
        args.rows, args.components, args.runs, args.warmup, args.append = "8192", "3", 2, 1, ""
    device = torch.device("cuda")
    gen = torch.Generator().manual_seed(SEED)
    rows = [shape_row(M, r, args, gen, device) for M in (int(v) for v in args.rows.split(",")) for r in (int(v) for v in args.components.split(","))]
    if not args.smoke:
        rows.append(scene_row(args, gen, device))
    for row in rows:
        line = json.dumps(row)
        print(line, flush=True)
        if args.append:
            os.makedirs(os.path.dirname(os.path.abspath(args.append)), exist_ok=True)
            with open(args.append, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
