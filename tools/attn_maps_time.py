#!/usr/bin/env python3
"""Attention-map timing (GPU box): ViTSpatialSpectral.attention_maps against an eager restatement of the same maps, on the encoder
of bench.py's flagship shape (8 x 8 windows x 200 bands, depth 12, 8 heads, bf16) at batch 32 and 256.

  attention_maps  the eval forward on two token buffers, msst_attn_maps on the input of every block (reduce="mean", both stacks);
  eager           what a user had to write before: the block inputs from Engine.blocks_fwd(save=False) (the same block kernels),
                  then per block F.layer_norm, two matmuls, softmax and the mean over the sample's sequences in torch (fp32);
  forward         the plain eval forward (forward_features) alone: what the maps cost on top of it.
All three are warmed up, then timed alternately in one process (device-synchronised wall clock per run; the median of --steps
runs, --reps repetitions).  The new launch is also timed alone (ten back-to-back calls between two device events) on the first
block's input of each stack, for both reductions.  No speed bar hangs on this tool: the kernel runs exact fp32 MFMAs (1/16 of the
bf16 rate), so all 24 blocks at batch 256 are expected to cost more than the forward itself, a fraction of it at batch <= 32.
Prints ONE JSON line and appends it to --append (default profiles/attn_maps_time.jsonl; '' to skip).

Run:  python tools/attn_maps_time.py [--steps 20] [--reps 3] [--warmup 2] [--precision bf16] [--batches 32,256] [--quick]
--quick: 50 bands, depth 1, batch 4, 2 runs x 2 repetitions (the test suite's smoke run).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from maskedsst_amd import ViTSpatialSpectral, _lib  # noqa: E402

SEED = 5


def build(args, device):
    torch.manual_seed(SEED)
    enc = ViTSpatialSpectral(
        image_size=8, spatial_patch_size=1, spectral_patch_size=10, num_classes=8, dim=96, depth=args.depth, heads=8, mlp_dim=64,
        dropout=0.0, emb_dropout=0.0, channels=args.bands, spectral_pos_embed=False, spectral_pos=torch.arange(args.bands // 10),
        blockwise_patch_embed=True, spectral_only=False, precision=args.precision)
    return enc.to(device).eval()


def eager(enc, img):
    """(spatial [B, depth, heads, N, N], spectral [B, depth, heads, S, S]): the maps restated in torch on the model's block inputs"""
    eng = enc.engine()
    S, N, H = eng.S, eng.N, enc.heads
    with torch.no_grad():
        eng.prep_weights()
        acts, _ = eng.blocks_fwd(eng.tokenize(img, None), save=False)
        out = {"spatial": [], "spectral": []}
        for i, (sname, l) in enumerate(eng._layers()):
            x = acts[i]
            B = x.shape[0]
            seq = x.view(B, S, N, 96) if sname == "spatial" else x.view(B, S, N, 96).transpose(1, 2)      # [B, G, L, 96]
            xn = F.layer_norm(seq, (96,), eng.fp.view(f"{sname}.{l}.ln1_g"), eng.fp.view(f"{sname}.{l}.ln1_b"), 1e-5)
            w = eng.fp.view(f"{sname}.{l}.wqkv")
            G, L = xn.shape[1], xn.shape[2]
            q = (xn @ w[:H * 64].t()).view(B, G, L, H, 64).permute(0, 1, 3, 2, 4)
            k = (xn @ w[H * 64:2 * H * 64].t()).view(B, G, L, H, 64).permute(0, 1, 3, 2, 4)
            out[sname].append(torch.softmax(q @ k.transpose(-1, -2) * 0.125, dim=-1).mean(dim=1))
    return torch.stack(out["spatial"], dim=1), torch.stack(out["spectral"], dim=1)


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


def kernel_alone(enc, img):
    """ms of one msst_attn_maps launch on the first block's input of each stack: {stack: {reduce: ms}}"""
    eng = enc.engine()
    S, N, H = eng.S, eng.N, enc.heads
    B = img.shape[0]
    with torch.no_grad():
        eng.prep_weights()
        acts, _ = eng.blocks_fwd(eng.tokenize(img, None), save=False)
    res = {}
    for sname, i in (("spatial", 0), ("spectral", enc.depth)):
        L, G = (N, S) if sname == "spatial" else (S, N)
        res[sname] = {}
        for name, reduce, shape in (("mean", _lib.ATTN_MEAN_SEQ, (B, H, L, L)), ("per_seq", _lib.ATTN_PER_SEQ, (B, G, H, L, L))):
            out = torch.empty(shape, device=img.device)
            fn = lambda: eng.attn_maps_block(i, acts[i], out, reduce)     # noqa: E731
            fn()
            res[sname][name] = round(event_ms(fn), 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--batches", default="32,256")
    ap.add_argument("--bands", type=int, default=200)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--append", default=os.path.join(ROOT, "profiles", "attn_maps_time.jsonl"))
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    if args.quick:
        args.steps, args.reps, args.warmup, args.batches, args.bands, args.depth = 2, 2, 1, "4", 50, 1
    device = torch.device("cuda")
    enc = build(args, device)
    gen = torch.Generator().manual_seed(SEED)
    rows = []
    for B in [int(b) for b in args.batches.split(",")]:
        img = torch.randn(B, args.bands, 8, 8, generator=gen).to(device)
        fast = lambda: enc.attention_maps(img)                      # noqa: E731
        slow = lambda: eager(enc, img)                              # noqa: E731

        def fwd():
            with torch.no_grad():
                return enc.forward_features(img)
        for _ in range(args.warmup):
            fast(); slow(); fwd()
        tf, ts, tw = [], [], []
        for _ in range(args.reps):
            a, b, c = [], [], []
            for _ in range(args.steps):
                t, maps = timed(fast)
                a.append(t)
                t, (esp, esc) = timed(slow)
                b.append(t)
                t, _ = timed(fwd)
                c.append(t)
            tf.append(round(1e3 * statistics.median(a), 3))
            ts.append(round(1e3 * statistics.median(b), 3))
            tw.append(round(1e3 * statistics.median(c), 3))
        diff = max(float((maps.spatial - esp).abs().max()), float((maps.spectral - esc).abs().max()))
        rows.append(dict(batch=B, attention_maps_ms=tf, eager_ms=ts, forward_ms=tw, kernel_ms=kernel_alone(enc, img), max_abs_diff=diff))
    row = dict(tool="attn_maps_time", precision=args.precision, bands=args.bands, depth=args.depth, steps=args.steps, reps=args.reps,
               results=rows)
    line = json.dumps(row)
    print(line, flush=True)
    if args.append:
        os.makedirs(os.path.dirname(os.path.abspath(args.append)), exist_ok=True)
        with open(args.append, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
