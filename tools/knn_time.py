#!/usr/bin/env python3
"""kNN evaluation timing (GPU box): msst_knn_topk + msst_knn_vote against their eager restatement.

Both legs start from an encode_scene-shaped map [Bs, 96, plane] of unit features and a bank [M, 96] with labels:
  knn     the two launches on the map in place (no score matrix, no permuted copy);
  eager   what a user had to write before: permute of the map into rows (a copy), chunked torch.mm against the bank (a vendor
          library GEMM; chunks of at most 2^28 scores), topk, gather of the labels, scatter_add_ of the weights, argmax.
Both are warmed up, then timed alternately in one process between device events; the medians of --steps runs are reported, with
the share of queries whose neighbour lists / classes agree (ties and last-bit differences of the similarities may reorder
neighbours: the eager route has no fixed tie rule).  The yardstick for the GEMM part is the fp32 matrix rate: 2 * 96 * Q * M flops
against 157 TFLOP/s.  The wall time of ViTSpatialSpectral.knn_predict_scene on --scenes scenes of --scene-size (the encoder of
bench.py's flagship shape by default) is timed against encode_scene + the eager route, per bank size and k.  No speed bar hangs on
this tool.  Prints ONE JSON line and appends it to --append (default profiles/knn_measured.jsonl; '' to skip).

Run:  python tools/knn_time.py [--shapes 8192x8192,16384x262144] [--ks 20,64] [--steps 20]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from maskedsst_amd import KnnBank, ViTSpatialSpectral  # noqa: E402
from maskedsst_amd.knn import knn_launch  # noqa: E402

SEED = 5
N_CLASSES = 8
PEAK_FP32_MATRIX = 157e12


def unit(n, gen):
    return torch.nn.functional.normalize(torch.randn(n, 96, generator=gen), dim=1)


def eager_rows(rows, bank, k, temperature, chunk_scores=1 << 28):
    """rows [Q, 96] -> (classes, votes, index, sim)"""
    Q, M = rows.shape[0], len(bank)
    kk = min(k, M)
    step = max(1, chunk_scores // M)
    sims, idxs = [], []
    for q0 in range(0, Q, step):
        s, i = torch.mm(rows[q0:q0 + step], bank.features.t()).topk(kk, dim=1)
        sims.append(s)
        idxs.append(i)
    sim, index = torch.cat(sims), torch.cat(idxs)
    lab = bank.labels.long()[index]
    w = torch.exp((sim - sim[:, :1]) / temperature) if temperature > 0 else torch.ones_like(sim)
    votes = torch.zeros(Q, bank.n_classes, device=rows.device).scatter_add_(1, lab, w)
    return votes.argmax(dim=1), votes, index, sim


def eager_map(fmap, bank, k, temperature):
    Bs, _, plane = fmap.shape
    return eager_rows(fmap.permute(0, 2, 1).reshape(Bs * plane, 96).contiguous(), bank, k, temperature)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), r


def alternate(fast, slow, timer, steps, warmup):
    for _ in range(warmup):
        fast()
        slow()
    a, b = [], []
    for _ in range(steps):
        t, rf = timer(fast)
        a.append(t)
        t, rs = timer(slow)
        b.append(t)
    return statistics.median(a), statistics.median(b), rf, rs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8192x8192,16384x262144", help="comma separated QxM (queries x bank rows)")
    ap.add_argument("--ks", default="20,64")
    ap.add_argument("--temperature", type=float, default=0.07)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--scenes", type=int, default=4)
    ap.add_argument("--scene-size", type=int, default=64)
    ap.add_argument("--bands", type=int, default=200)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--append", default=os.path.join(ROOT, "profiles", "knn_measured.jsonl"))
    args = ap.parse_args()
    device = torch.device("cuda")
    gen = torch.Generator().manual_seed(SEED)
    torch.manual_seed(SEED)
    enc = ViTSpatialSpectral(
        image_size=8, spatial_patch_size=1, spectral_patch_size=10, num_classes=N_CLASSES, dim=96, depth=args.depth, heads=8, mlp_dim=64,
        dropout=0.0, emb_dropout=0.0, channels=args.bands, spectral_pos_embed=False, spectral_pos=torch.arange(args.bands // 10),
        blockwise_patch_embed=True, spectral_only=False, precision=args.precision).to(device).eval()
    scene = torch.randn(args.scenes, args.bands, args.scene_size, args.scene_size, generator=gen).to(device)
    T = args.temperature
    rows = []
    for shape in args.shapes.split(","):
        Q, M = (int(v) for v in shape.split("x"))
        Bs = 2 if Q % 2 == 0 else 1
        plane = Q // Bs
        bank = KnnBank(unit(M, gen).to(device), torch.randint(0, N_CLASSES, (M,), generator=gen).to(device), N_CLASSES)
        fmap = unit(Q, gen).view(Bs, plane, 96).permute(0, 2, 1).contiguous().to(device)          # [Bs, 96, plane]
        votes = torch.empty(Bs, N_CLASSES, plane, device=device)
        classes = torch.empty(Q, dtype=torch.int64, device=device)
        for k in [int(v) for v in args.ks.split(",")]:
            index = torch.empty(Q, k, dtype=torch.int32, device=device)
            sim = torch.empty(Q, k, device=device)
            fast = lambda: knn_launch(bank, fmap, 1, Q, plane, k, T, None, votes, 1, classes, index=index, sim=sim)   # noqa: E731
            slow = lambda: eager_map(fmap, bank, k, T)                                                               # noqa: E731
            tf, ts, _, (ec, ev, ei, es) = alternate(fast, slow, event_ms, args.steps, args.warmup)
            kk = min(k, M)
            same_index = (index[:, :kk].long() == ei).all(dim=1).double().mean()
            same_class = (classes == ec).double().mean()
            fast_s = lambda: enc.knn_predict_scene(scene, bank, k=k, temperature=T)                  # noqa: E731
            slow_s = lambda: eager_map(enc.encode_scene(scene, normalize=True).features.flatten(2), bank, k, T)   # noqa: E731
            wf, ws, _, _ = alternate(fast_s, slow_s, wall_ms, args.steps, args.warmup)
            gemm_ms = 1e3 * 2 * 96 * Q * M / PEAK_FP32_MATRIX
            rows.append(dict(Q=Q, M=M, k=k, knn_kernels_ms=round(tf, 4), eager_ms=round(ts, 4), gemm_at_peak_ms=round(gemm_ms, 4),
                             index_equal_share=float(same_index), classes_equal_share=float(same_class),
                             scene_queries=int(scene.shape[0] * scene.shape[2] * scene.shape[3]),
                             knn_predict_scene_ms=round(wf, 3), eager_scene_ms=round(ws, 3)))
    row = dict(tool="knn_time", precision=args.precision, bands=args.bands, depth=args.depth, scenes=args.scenes,
               scene_size=args.scene_size, steps=args.steps, temperature=T, results=rows)
    line = json.dumps(row)
    print(line, flush=True)
    if args.append:
        os.makedirs(os.path.dirname(os.path.abspath(args.append)), exist_ok=True)
        with open(args.append, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
