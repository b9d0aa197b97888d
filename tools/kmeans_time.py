#!/usr/bin/env python3
"""k-means timing (GPU box): one Lloyd iteration (msst_kmeans_assign + msst_kmeans_update) and a whole fit (maskedsst_amd.fit_kmeans)
against the eager restatement; the two launches of an iteration are also timed apart.

Per shape -- M rows [M, 96] of Gaussian blobs, k clusters, metric -- from the same initial centroids:
  hip     two launches per iteration, no host synchronisation before the history's read-back;
  eager   what a user writes in PyTorch: chunked mm + bias, argmax, index_add_, bincount, divide (or normalise).
Both are warmed up, then timed alternately in one process between device events (the device time of the queued launches, as in
tools/knn_time.py and tools/probe_time.py); the medians of --runs runs are reported.  An iteration's time is that of --iters
iterations queued between two events, divided by --iters; a fit is fit_kmeans(iters=--fit-iters) from a tensor init against the eager
loop, each ending in ONE read-back.  With the iteration's time go the rates it means: 2 x 2 M k 96 FLOP (the two products) and the
4 x 96 M bytes of the rows.  No speed bar hangs on this tool.  Prints ONE JSON line per shape and appends it to --append (default
profiles/kmeans_measured.jsonl; '' to skip).  --smoke: the smallest shape alone, two runs, nothing appended.

Run:  python tools/kmeans_time.py [--rows 8192,262144] [--clusters 16,128] [--metrics cosine,euclidean] [--runs 20]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from maskedsst_amd import _lib, fit_kmeans  # noqa: E402
from maskedsst_amd import cluster  # noqa: E402
from maskedsst_amd.features import _p, _stream  # noqa: E402

SEED = 5
CHUNK = 65536


def eager_iteration(x, cent, bias, metric):
    k = cent.shape[0]
    labels = torch.empty(x.shape[0], dtype=torch.int64, device=x.device)
    for lo in range(0, x.shape[0], CHUNK):
        labels[lo:lo + CHUNK] = torch.addmm(bias, x[lo:lo + CHUNK], cent.t()).argmax(dim=1)
    sums = torch.zeros(k, 96, device=x.device).index_add_(0, labels, x)
    counts = torch.bincount(labels, minlength=k)
    if metric == "cosine":
        n = sums.norm(dim=1, keepdim=True)
        new = torch.where((n > 0) & (counts > 0).unsqueeze(1), sums / n.clamp_min(1e-30), cent)
        return new, bias, labels
    new = torch.where((counts > 0).unsqueeze(1), sums / counts.clamp(min=1).unsqueeze(1), cent)
    return new, -0.5 * (new * new).sum(dim=1), labels


def eager_fit(x, cent, metric, iters):
    bias = cluster._bias(cent, metric)
    moved, prev = [], None
    for _ in range(iters):
        cent, bias, labels = eager_iteration(x, cent, bias, metric)
        moved.append((labels != prev).sum() if prev is not None else torch.tensor(x.shape[0], device=x.device))
        prev = labels
    return torch.stack(moved).cpu()           # one read-back, as the fit's history


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def alternate(fast, slow, runs, warmup):
    for _ in range(warmup):
        fast()
        slow()
    a, b = [], []
    for _ in range(runs):
        a.append(event_ms(fast)[0])
        b.append(event_ms(slow)[0])
    return statistics.median(a), statistics.median(b)


def shape_row(M, k, metric, args, gen, device):
    centres = torch.randn(k, 96, generator=gen)
    x = centres[torch.randint(0, k, (M,), generator=gen)] + 0.5 * torch.randn(M, 96, generator=gen)
    init = centres + 0.2 * torch.randn(k, 96, generator=gen)
    if metric == "cosine":
        x, init = x / x.norm(dim=1, keepdim=True), init / init.norm(dim=1, keepdim=True)
    x, init = x.to(device).contiguous(), init.to(device).contiguous()

    # ---- one iteration: --iters iterations between two events
    cent, bias = init.clone(), cluster._bias(init, metric)
    assign = torch.full((M,), -1, dtype=torch.int32, device=device)
    dist = torch.empty(M, device=device)
    slab = torch.empty(int(_lib.load().msst_kmeans_scratch_floats(M, k)), device=device)
    rec = torch.empty(cluster.record_width(k), device=device)

    def hip_iters():
        for _ in range(args.iters):
            cluster.lloyd_iteration(x, cent, bias, metric, assign, dist, slab, rec)

    def eager_iters():
        c, b = init, cluster._bias(init, metric)
        for _ in range(args.iters):
            c, b, _ = eager_iteration(x, c, b, metric)

    def assign_only():
        for _ in range(args.iters):
            _lib.check(lib.msst_kmeans_assign(_p(x), 0, M, 1, 96, _p(cent), _p(bias), k, cluster.METRICS[metric], _p(assign), _p(dist), None,
                                              _p(slab), slab.numel(), _stream()), "msst_kmeans_assign")

    def update_only():
        for _ in range(args.iters):
            _lib.check(lib.msst_kmeans_update(_p(slab), slab.numel(), M, 96, k, cluster.METRICS[metric], _p(cent), _p(bias), _p(cnt), _p(shift),
                                              _p(rec), _stream()), "msst_kmeans_update")

    lib = _lib.load()
    cnt, shift = torch.empty(k, dtype=torch.int32, device=device), torch.empty(k, device=device)
    it_hip, it_eager = alternate(hip_iters, eager_iters, args.runs, args.warmup)
    assign_ms, update_ms = alternate(assign_only, update_only, max(3, args.runs // 2), 1)      # the two launches apart
    fit_hip, fit_eager = alternate(lambda: fit_kmeans(x, k=k, iters=args.fit_iters, metric=metric, init=init),
                                   lambda: eager_fit(x, init, metric, args.fit_iters), args.runs, args.warmup)
    us = 1e3 * it_hip / args.iters
    return dict(tool="kmeans_time", M=M, k=k, metric=metric, runs=args.runs, iters=args.iters, fit_iters=args.fit_iters,
                iteration_us=round(us, 2), assign_launch_us=round(1e3 * assign_ms / args.iters, 2),
                update_launch_us=round(1e3 * update_ms / args.iters, 2), eager_iteration_us=round(1e3 * it_eager / args.iters, 2),
                fit_ms=round(fit_hip, 4), eager_fit_ms=round(fit_eager, 4),
                eager_faster=dict(iteration=bool(it_eager < it_hip), fit=bool(fit_eager < fit_hip)),
                iteration_TFLOPs=round(4.0 * M * k * 96 / (us * 1e-6) / 1e12, 2), rows_GBps=round(M * 96 * 4 / (us * 1e-6) / 1e9, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="8192,262144", help="comma separated row counts M")
    ap.add_argument("--clusters", default="16,128", help="comma separated cluster counts k")
    ap.add_argument("--metrics", default="cosine,euclidean")
    ap.add_argument("--iters", type=int, default=20, help="iterations queued between two events when one iteration is timed")
    ap.add_argument("--fit-iters", type=int, default=50)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--append", default=os.path.join(ROOT, "profiles", "kmeans_measured.jsonl"))
    ap.add_argument("--smoke", action="store_true", help="the smallest shape alone, two runs, nothing appended")
    args = ap.parse_args()
    if args.smoke:
        args.rows, args.clusters, args.metrics, args.iters, args.fit_iters, args.runs, args.warmup, args.append = "8192", "16", "cosine", 3, 3, 2, 1, ""
    device = torch.device("cuda")
    gen = torch.Generator().manual_seed(SEED)
    for M in (int(v) for v in args.rows.split(",")):
        for k in (int(v) for v in args.clusters.split(",")):
            for metric in args.metrics.split(","):
                line = json.dumps(shape_row(M, k, metric, args, gen, device))
                print(line, flush=True)
                if args.append:
                    os.makedirs(os.path.dirname(os.path.abspath(args.append)), exist_ok=True)
                    with open(args.append, "a") as f:
                        f.write(line + "\n")


if __name__ == "__main__":
    main()
