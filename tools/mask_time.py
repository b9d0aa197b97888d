#!/usr/bin/env python3
"""What the two SimMIM mask sources cost, one run on one box in one process: the host generator (``draw_masks`` + ``inverse_csr`` +
the pinned upload, the default and the parent behaviour) against the device generator (``draw_masks_device``: msst_draw_masks, one
launch), in the three mask configurations -- mask_patch_size 1 / ratio 0.5 (top-k), mask_patch_size 4 / ratio 0.7 without tube and with
tube (what bench.py runs).

  part "source"   the mask source alone at batch 256 and 2048.  host: the wall clock around draw_masks + inverse_csr + _upload (the
                  copies are asynchronous; the synchronise behind them is outside the clock).  device: host_us, the wall clock around
                  the draw_masks_device call (allocations and the launch; nothing waits), and device_us, device events around the
                  launch enqueued behind a workgroup that holds the device for --hold-us.
  part "step"     zero_grad -> model(img) -> backward -> optimizer.step at the bench shape (200 bands, depth 12, bf16, batch 256), both
                  sources; ms per step = wall clock of --inner steps and a synchronise, divided by --inner.  dp_world = 8 lines: the
                  placement attributes set by hand (rank 3 of 8), so that the host source draws the global 2048 rows as every rank of
                  an 8-GPU run does and the device source its own 256.

The variants run alternated, round after round; a figure is the median over --rounds rounds.  Prints one JSON line per variant; --out
appends them to a file (profiles/device_masks_measured.jsonl is the committed measurement).
Run on the GPU:  python tools/mask_time.py --out profiles/device_masks_measured.jsonl
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = [("topk_r0.5", dict(masking_ratio=0.5, mask_patch_size=1, tube_masking=False)),
           ("block4_r0.7", dict(masking_ratio=0.7, mask_patch_size=4, tube_masking=False)),
           ("tube4_r0.7", dict(masking_ratio=0.7, mask_patch_size=4, tube_masking=True))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bands", type=int, default=200)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=4, help="steps per sample of part step")
    ap.add_argument("--hold-us", type=int, default=3000, help="how long the device is held while the host enqueues a device-time sample")
    ap.add_argument("--parts", default="source,step")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mask_time.py measures on the GPU: no device found")
    from maskedsst_amd import ViTSpatialSpectral, SimMIMSpatialSpectral, _lib
    from maskedsst_amd.masking import inverse_csr
    from maskedsst_amd.optim import FusedAdamW
    lib = _lib.load()
    S = args.bands // 10

    def build(kw):
        torch.manual_seed(5); np.random.seed(5)
        enc = ViTSpatialSpectral(image_size=8, spatial_patch_size=1, spectral_patch_size=10, num_classes=8, dim=96, depth=args.depth, heads=8,
                                 mlp_dim=64, channels=args.bands, spectral_pos_embed=False, spectral_pos=torch.arange(S), precision="bf16")
        model = SimMIMSpatialSpectral(encoder=enc, to_pixels_per_spectral_block=True, **kw).cuda().train()
        return model, FusedAdamW(model, lr=0.008, weight_decay=0.05, grad_clamp=1.0)

    models = {name: build(kw) for name, kw in CONFIGS}
    img = torch.randn(args.batch, args.bands, 8, 8, generator=torch.Generator().manual_seed(3)).cuda()
    sink = torch.zeros(1, dtype=torch.int32, device="cuda")
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    variants = []   # (identity dict, sampler -> dict of figures or None)

    def source_host(model, batch):
        eng, T = model.engine(), model.encoder.num_patches

        def run():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            bm, idx = model.draw_masks(batch)
            ix = idx.numpy()
            ptr, pos = inverse_csr(ix, T)
            eng._upload(img.device, bm.numpy().astype(np.uint8), ix.astype(np.int32), ptr, pos)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            return dict(host_us=1e6 * (t1 - t0))
        return run

    def source_device(model, batch):
        def run():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.draw_masks_device(batch)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            out = dict(host_us=1e6 * (t1 - t0))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            _lib.check(lib.msst_debug_cu_thief(1, args.hold_us, ctypes.c_void_p(sink.data_ptr()), stream()), "hold")
            e0.record()
            model.draw_masks_device(batch)
            e1.record()
            enqueued = time.perf_counter()
            e1.synchronize()
            if 1e6 * (enqueued - t0) < args.hold_us:   # else the events would time the host
                out["device_us"] = 1e3 * e0.elapsed_time(e1)
            return out
        return run

    def step(model, opt, source, world):
        def run():
            model.mask_source = source
            model.dp_rank, model.dp_world = (3, 8) if world > 1 else (0, 1)
            try:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.inner):
                    opt.zero_grad()
                    model(img).backward()
                    opt.step()
                torch.cuda.synchronize()
                return dict(step_ms=1e3 * (time.perf_counter() - t0) / args.inner)
            finally:
                model.mask_source = "host"
                model.dp_rank, model.dp_world = 0, 1
        return run

    parts = args.parts.split(",")
    for name, _ in CONFIGS:
        model, opt = models[name]
        if "source" in parts:
            for batch in (256, 2048):
                variants.append((dict(part="source", config=name, source="host", batch=batch), source_host(model, batch)))
                variants.append((dict(part="source", config=name, source="device", batch=batch), source_device(model, batch)))
        if "step" in parts:
            for world in (1, 8):
                for source in ("host", "device"):
                    variants.append((dict(part="step", config=name, source=source, batch=args.batch, dp_world=world, inner=args.inner),
                                     step(model, opt, source, world)))
    samples = [dict() for _ in variants]
    for r in range(args.warmup + args.rounds):
        for i, (_, run) in enumerate(variants):
            got = run()
            if r >= args.warmup:
                for k, v in got.items():
                    samples[i].setdefault(k, []).append(v)
    lines = []
    for (ident, _), figs in zip(variants, samples):
        line = dict(tool="mask_time", **ident, bands=args.bands, depth=args.depth, rounds=args.rounds, device=torch.cuda.get_device_name(0))
        for k, v in figs.items():
            if len(v) >= max(1, args.rounds // 2):
                line.update({k: round(statistics.median(v), 3), k + "_min": round(min(v), 3), k + "_max": round(max(v), 3)})
            else:
                line[k] = None   # not measured: the host could not enqueue within the hold
        lines.append(line)
    for line in lines:
        print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
