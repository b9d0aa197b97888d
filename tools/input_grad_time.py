#!/usr/bin/env python3
"""What the input gradient costs at the bench shape (B = 256, 200 bands, 8 x 8, depth 12, bf16), one run on one box:

1. the msst_tokenize_bwd_input launch against the msst_tokenize_bwd launch of the same step (library profiler, median of --steps);
2. the SimMIM training step (forward + backward) with and without img.requires_grad (HIP events, median);
3. the frozen-model saliency call (every parameter frozen, forward + backward down to the input) against the training step.

Prints one JSON line; --out appends it to a file (profiles/input_grad_time_measured.jsonl is the committed measurement).
Run on the GPU:  python tools/input_grad_time.py --steps 20
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--bands", type=int, default=200)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from maskedsst_amd import ViTSpatialSpectral, SimMIMSpatialSpectral, _lib
    torch.manual_seed(5)
    enc = ViTSpatialSpectral(image_size=8, spatial_patch_size=1, spectral_patch_size=10, num_classes=8, dim=96, depth=args.depth, heads=8,
                             mlp_dim=64, channels=args.bands, spectral_pos_embed=False, spectral_pos=torch.arange(args.bands // 10),
                             precision="bf16")
    model = SimMIMSpatialSpectral(encoder=enc, masking_ratio=0.7, mask_patch_size=4, tube_masking=True,
                                  to_pixels_per_spectral_block=True).cuda().train()
    lib = _lib.load()
    nk = lib.msst_profile_kernels()
    names = [lib.msst_profile_name(i).decode() for i in range(nk)]
    x = torch.randn(args.batch, args.bands, 8, 8, device="cuda")
    masks = model.draw_masks(args.batch)

    def step(want_input):
        xi = x.detach().requires_grad_(want_input)
        model(xi, masks=masks).backward()
        for p in model.parameters():
            p.grad = None

    def timed(fn, n):
        out = []
        for _ in range(n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b))
        return statistics.median(out)

    for _ in range(args.warmup):
        step(True)
    torch.cuda.synchronize()
    # 1. per-launch times of the two tokenizer backward launches, one collect per step
    lib.msst_profile_select(ctypes.c_ulonglong((1 << names.index("tokenize_bwd")) | (1 << names.index("tokenize_bwd_input"))))
    per = {"tokenize_bwd": [], "tokenize_bwd_input": []}
    for _ in range(args.steps):
        lib.msst_profile_enable(1)
        step(True)
        tot, cnt = (ctypes.c_double * nk)(), (ctypes.c_long * nk)()
        lib.msst_profile_collect(tot, cnt)
        lib.msst_profile_enable(0)
        for k in per:
            i = names.index(k)
            assert cnt[i] == 1, (k, cnt[i])
            per[k].append(1e3 * tot[i])
    lib.msst_profile_select(ctypes.c_ulonglong(2 ** 64 - 1))
    # 2. the training step with and without the input gradient
    t_without, t_with = timed(lambda: step(False), args.steps), timed(lambda: step(True), args.steps)
    # 3. the frozen-model saliency call
    for p in model.parameters():
        p.requires_grad_(False)
    step(True)
    t_frozen = timed(lambda: step(True), args.steps)
    row = dict(shape=dict(batch=args.batch, bands=args.bands, depth=args.depth, precision="bf16"), steps=args.steps,
               device=torch.cuda.get_device_name(0),
               tokenize_bwd_us=statistics.median(per["tokenize_bwd"]), tokenize_bwd_input_us=statistics.median(per["tokenize_bwd_input"]),
               step_ms=t_without, step_with_img_grad_ms=t_with, frozen_saliency_ms=t_frozen)
    line = json.dumps(row)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
