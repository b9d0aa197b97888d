#!/usr/bin/env python3
"""Gaussian (QDA / LDA) scoring time (GPU box): the one launch of GaussianClassifier.classify (msst_gauss_score: every class's squared
Mahalanobis distance, the log joint densities, the argmax and the distance to it) against the eager restatement.

Per shape -- Q rows [Q, 96] with a mean of 50 per channel, nc classes, full (one whitening table a class) or tied (one table, nc
whitened means):
  hip     one launch: classes [Q], distance [Q] and scores [Q, nc]; `hip_lean_us` is the same launch without the scores output.
  eager   a loop over the classes of ((x - mu_c) @ A_c.T).square().sum(1) into d2 [Q, nc] (rows in chunks of --chunk, so that the
          [chunk, 96] intermediates fit), then scores = const - 0.5 d2, argmax, gather.  `eager_expanded_us` (tied only) is the eager
          route one table allows: z = (x - centre) @ A.T once, then the distances to the whitened means by the expanded square.
The last row is the feature side of gaussian_predict_scene on four 64 x 64 scenes (the encoder pass, common to both sides, is left
out): the map [4, 96, 64, 64] read in place and the scores written as a map, against the eager route on the permuted map.  Both sides
are warmed up, then timed alternately in one process between device events (the device time of the queued launches, as in
tools/pca_time.py); the medians of --runs runs are reported.  No speed bar hangs on this tool; every shape is reported, the ones eager
wins included.  Prints ONE JSON line per shape and appends it to --append (default profiles/gauss_measured.jsonl; '' to skip).
--smoke: the smallest shape alone, two runs, nothing appended.

Run:  python tools/gauss_time.py [--rows 8192,262144] [--classes 16,128] [--runs 20]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from maskedsst_amd import GaussianClassifier  # noqa: E402

SEED = 5
REPEAT = 4      # calls queued between two events


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


def make_classifier(nc, tied, gen):
    """random class Gaussians around 50: one random rotation, per class a spectrum exp(-j / 24) scaled by a factor of its own"""
    q = torch.linalg.qr(torch.randn(96, 96, generator=gen, dtype=torch.float64))[0].numpy()
    lam = np.exp(-np.arange(96) / 12.0)
    means = 50.0 + 0.1 * torch.randn(nc, 96, generator=gen, dtype=torch.float64).numpy()
    scale = 0.5 + 1.5 * torch.rand(nc, generator=gen, dtype=torch.float64).numpy()
    base = (q * lam) @ q.T
    cov = base if tied else np.stack([base * s for s in scale])
    return GaussianClassifier(means, cov, np.ones(nc), tied=tied)


def eager_scores(x, clf, chunk, expanded=False):
    """the loop over the classes; expanded (tied only): one projection, then the distances to the whitened means by the expanded square"""
    t = clf._tables(x.device)
    nc = clf.n_classes
    means = clf.means.to(x.device)
    d2 = torch.empty(x.shape[0], nc, device=x.device)
    for r0 in range(0, x.shape[0], chunk):
        xs = x[r0:r0 + chunk]
        if expanded:
            z = (xs - t["centres"][0]) @ t["tables"][0].t()
            m = t["offsets"]
            d2[r0:r0 + chunk] = (z.square().sum(1, keepdim=True) + m.square().sum(1)[None, :] - 2.0 * (z @ m.t())).clamp_(min=0)
        else:
            for c in range(nc):
                d2[r0:r0 + chunk, c] = ((xs - means[c]) @ t["tables"][0 if clf.tied else c].t()).square().sum(1)
    scores = t["consts"][None, :] - 0.5 * d2
    classes = scores.argmax(1)
    return classes, scores, d2.gather(1, classes[:, None])[:, 0]


def shape_row(Q, nc, tied, args, gen, device):
    clf = make_classifier(nc, tied, gen)
    x = (torch.randn(Q, 96, generator=gen) * torch.exp(-torch.arange(96) / 24.0) + 50.0).to(device).contiguous()
    hip, eager = alternate(lambda: clf.classify(x), lambda: eager_scores(x, clf, args.chunk), args.runs, args.warmup)
    lean, expanded = alternate(lambda: clf.classify(x, scores=False), (lambda: eager_scores(x, clf, args.chunk, True)) if tied else (lambda: None),
                               max(3, args.runs // 2), 1)
    same = float((clf.classify(x).classes == eager_scores(x, clf, args.chunk)[0]).double().mean())
    T = 1 if tied else nc
    flop = 2.0 * Q * 96 * (96 * T + nc)
    return dict(tool="gauss_time", Q=Q, nc=nc, covariance="tied" if tied else "full", runs=args.runs, hip_us=round(hip, 2),
                eager_us=round(eager, 2), eager_expanded_us=round(expanded, 2) if tied else None, hip_lean_us=round(lean, 2), hip_tflops=round(flop / (hip * 1e-6) / 1e12, 2),
                classes_agree=round(same, 5), eager_faster=bool(min(eager, expanded if tied else eager) < hip))


def scene_row(args, gen, device):
    """the feature side of gaussian_predict_scene on four 64 x 64 scenes: a map with a band of uncovered pixels, 16 full classes"""
    Bs, H, W, nc = 4, 64, 64, 16
    clf = make_classifier(nc, False, gen)
    m = torch.randn(Bs, 96, H, W, generator=gen) * torch.exp(-torch.arange(96) / 24.0).view(1, 96, 1, 1) + 50.0
    m[:, :, 60:, :] = float("nan")
    m[:, :, :, 60:] = float("nan")
    m = m.to(device).contiguous()

    def eager_map():
        classes, scores, dist = eager_scores(m.permute(0, 2, 3, 1).reshape(-1, 96), clf, args.chunk)
        return classes.view(Bs, H, W), scores.view(Bs, H, W, nc).permute(0, 3, 1, 2).contiguous(), dist.view(Bs, H, W)

    hip, eager = alternate(lambda: clf._launch(m, True, float("inf"), out_layout=1), eager_map, args.runs, args.warmup)
    return dict(tool="gauss_time", scene=f"{Bs}x{H}x{W}", nc=nc, covariance="full", runs=args.runs, map_us=round(hip, 2),
                eager_map_us=round(eager, 2), eager_faster=bool(eager < hip))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="8192,262144", help="comma separated row counts Q")
    ap.add_argument("--classes", default="16,128", help="comma separated class counts nc")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chunk", type=int, default=65536, help="rows per chunk of the eager route")
    ap.add_argument("--append", default=os.path.join(ROOT, "profiles", "gauss_measured.jsonl"))
    ap.add_argument("--smoke", action="store_true", help="the smallest shape alone (full covariances), two runs, nothing appended")
    args = ap.parse_args()
    kinds = (False, True)
    if args.smoke:
        args.rows, args.classes, args.runs, args.warmup, args.append, kinds = "8192", "16", 2, 1, "", (False,)
    device = torch.device("cuda")
    gen = torch.Generator().manual_seed(SEED)
    rows = [shape_row(Q, nc, tied, args, gen, device) for Q in (int(v) for v in args.rows.split(",")) for nc in (int(v) for v in args.classes.split(","))
            for tied in kinds]
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
