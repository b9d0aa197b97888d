#!/usr/bin/env python3
"""Scene embedding timing (GPU box): ViTSpatialSpectral.encode_scene against its eager restatement, on the encoder of bench.py's
flagship shape (8 x 8 windows x 200 bands, depth 12, 8 heads, bf16), four 64 x 64 scenes, strides 8 and 4.

Both legs run the SAME encoder kernels; they differ in what surrounds them:
  encode_scene  the scene tokenizer reads the windows out of the scene, msst_pool_spectral_fwd averages the encoder output over
                the spectral axis, msst_scene_embed_assemble folds the windows into [Bs, 96, Hs, Ws] and counts the cover;
  eager         what a user had to write before: the windows stacked into a batch (a copy: stack_windows, or unfold where they
                overlap), forward_features on it, a torch mean over S, and a fold with index_add into the flattened map, divided
                by the cover counted the same way.
Both are warmed up, then timed alternately in one process (device-synchronised wall clock per run; the median of --steps runs,
--reps repetitions).  The two new kernels are also timed on their own (ten back-to-back calls between two device events, on the
encoder output of one chunk).  The encoder dominates both legs: no speed bar hangs on this tool.  Prints ONE JSON line and appends it
to --append (default profiles/encode_scene_time.jsonl; '' to skip).

Run:  python tools/embed_time.py [--steps 20] [--reps 3] [--warmup 2] [--precision bf16] [--quick]
--quick: two 24 x 24 scenes of 50 bands at depth 1, 2 runs x 2 repetitions (the test suite's smoke run).
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

from maskedsst_amd import ViTSpatialSpectral  # noqa: E402
from maskedsst_amd.utils import stack_windows  # noqa: E402

SEED = 5


def build(args, device):
    torch.manual_seed(SEED)
    enc = ViTSpatialSpectral(
        image_size=8, spatial_patch_size=1, spectral_patch_size=10, num_classes=8, dim=96, depth=args.depth, heads=8, mlp_dim=64,
        dropout=0.0, emb_dropout=0.0, channels=args.bands, spectral_pos_embed=False, spectral_pos=torch.arange(args.bands // 10),
        blockwise_patch_embed=True, spectral_only=False, precision=args.precision)
    return enc.to(device).eval()


def stacked(scene, w, stride):
    """the windows of scene [Bs, C, Hs, Ws] as a batch [Bs nr nq, C, w, w] in the kernels' window order (a copy)"""
    if stride == w:
        return stack_windows(scene, w).contiguous()
    u = scene.unfold(2, w, stride).unfold(3, w, stride)     # [Bs, C, nr, nq, w, w]
    return u.permute(0, 2, 3, 1, 4, 5).reshape(-1, scene.shape[1], w, w).contiguous()


def fold_index(Bs, Hs, Ws, w, stride, device):
    """flat pixel index (scene, y, x) of every (window, position) in window order: what index_add folds along"""
    ys = torch.arange(0, Hs - w + 1, stride, device=device)
    xs = torch.arange(0, Ws - w + 1, stride, device=device)
    d = torch.arange(w, device=device)
    yy = (ys[:, None, None, None] + d[None, None, :, None]).expand(len(ys), len(xs), w, w)
    xx = (xs[None, :, None, None] + d[None, None, None, :]).expand(len(ys), len(xs), w, w)
    one = (yy * Ws + xx).reshape(-1)
    return (torch.arange(Bs, device=device)[:, None] * (Hs * Ws) + one[None, :]).reshape(-1)


def eager(enc, scene, w, stride, index):
    Bs, _, Hs, Ws = scene.shape
    S = enc.num_spectral_patches
    with torch.no_grad():
        y = enc.forward_features(stacked(scene, w, stride))                  # [nwin, S N, 96]
        f = y.view(y.shape[0], S, w * w, 96).mean(dim=1).reshape(-1, 96)      # [nwin N, 96]
        acc = torch.zeros(Bs * Hs * Ws, 96, device=scene.device).index_add_(0, index, f)
        cover = torch.zeros(Bs * Hs * Ws, device=scene.device).index_add_(0, index, torch.ones(len(index), device=scene.device))
        feat = torch.where(cover[:, None] > 0, acc / cover[:, None], torch.full((), float("nan"), device=scene.device))
    return feat.view(Bs, Hs, Ws, 96).permute(0, 3, 1, 2), cover.view(Bs, Hs, Ws).to(torch.int32)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def event_ms(fn, n=10):
    """ms per call of n back-to-back calls between two device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def kernels_alone(enc, scene, w, stride):
    """(pool ms, assemble ms) of the two new launches on the encoder output of all windows of the scenes as one chunk"""
    from maskedsst_amd import _lib
    from maskedsst_amd.engine import _p, _stream
    eng = enc.engine()
    Bs, _, Hs, Ws = scene.shape
    S, N = eng.S, eng.N
    with torch.no_grad():
        y = enc.forward_features(stacked(scene, w, stride)).contiguous()
    nwin = y.shape[0]
    win_feat = torch.empty(nwin, 96, N, device=scene.device)
    feat = torch.empty(Bs, 96, Hs, Ws, device=scene.device)
    cover = torch.empty(Bs, Hs, Ws, dtype=torch.int32, device=scene.device)
    st = _stream()

    def pool():
        _lib.check(eng.lib.msst_pool_spectral_fwd(_p(y), _p(win_feat), nwin, S, N, st), "msst_pool_spectral_fwd")

    def assemble():
        _lib.check(eng.lib.msst_scene_embed_assemble(_p(win_feat), 0, nwin, _p(feat), _p(cover), Bs, 96, Hs, Ws, w, stride, 1, 1, st),
                   "msst_scene_embed_assemble")

    pool(); assemble()
    return event_ms(pool), event_ms(assemble)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--scenes", type=int, default=4)
    ap.add_argument("--scene-size", type=int, default=64)
    ap.add_argument("--bands", type=int, default=200)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--strides", default="8,4")
    ap.add_argument("--append", default=os.path.join(ROOT, "profiles", "encode_scene_time.jsonl"))
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    if args.quick:
        args.steps, args.reps, args.warmup, args.scenes, args.scene_size, args.bands, args.depth = 2, 2, 1, 2, 24, 50, 1
    device = torch.device("cuda")
    enc = build(args, device)
    w = enc.num_spatial_patches_sqrt
    gen = torch.Generator().manual_seed(SEED)
    scene = torch.randn(args.scenes, args.bands, args.scene_size, args.scene_size, generator=gen).to(device)
    rows = []
    for stride in [int(s) for s in args.strides.split(",")]:
        index = fold_index(args.scenes, args.scene_size, args.scene_size, w, stride, device)
        fast = lambda: enc.encode_scene(scene, stride=stride)       # noqa: E731
        slow = lambda: eager(enc, scene, w, stride, index)          # noqa: E731
        for _ in range(args.warmup):
            fast()
            slow()
        tf, ts = [], []
        for _ in range(args.reps):
            a, b = [], []
            for _ in range(args.steps):
                t, emb = timed(fast)
                a.append(t)
                t, (ef, ec) = timed(slow)
                b.append(t)
            tf.append(round(1e3 * statistics.median(a), 3))
            ts.append(round(1e3 * statistics.median(b), 3))
        ok = emb.cover > 0
        diff = float((emb.features.permute(0, 2, 3, 1)[ok] - ef.permute(0, 2, 3, 1)[ok]).abs().max())
        pool_ms, asm_ms = kernels_alone(enc, scene, w, stride)
        rows.append(dict(stride=stride, windows=len(index) // (w * w), encode_scene_ms=tf, eager_ms=ts,
                         pool_kernel_ms=round(pool_ms, 4), assemble_kernels_ms=round(asm_ms, 4), max_abs_diff=diff,
                         cover_equal=bool(torch.equal(emb.cover, ec)),
                         nan_equal=bool(torch.equal(torch.isnan(emb.features), torch.isnan(ef)))))
    row = dict(tool="encode_scene_time", precision=args.precision, bands=args.bands, depth=args.depth, scenes=args.scenes,
               scene_size=args.scene_size, steps=args.steps, reps=args.reps, results=rows)
    line = json.dumps(row)
    print(line, flush=True)
    if args.append:
        os.makedirs(os.path.dirname(os.path.abspath(args.append)), exist_ok=True)
        with open(args.append, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
