#!/usr/bin/env python3
"""Classifier-head timing (GPU box) at the EnMAP finetune shape (200 bands, depth 4, 8 classes, image_size 8, B = 256):

* the finetune step (forward + backward + FusedAdamW) with the default head and with the spectral MLP head
  (spectral_mlp_head=True), both warmed up, then timed alternately in one process (device-synchronised wall clock per step,
  median reported);
* the head kernels alone, from a separate ``rocprofv3 --kernel-trace --stats`` run of this script in a fresh child process
  (``--kernels-only``: msst_spec_head_fwd / _bwd on a fixed y, nothing else launched): mean microseconds per call of the
  forward and of the backward (its four launches summed) and the GB/s they reach on the bytes they must move -- y once
  (forward), y read and dy written (backward) -- with the share of the byte floor at the 6.29 TB/s copy rate.

Prints ONE JSON line.  Run:  python tools/head_time.py [--steps 20] [--precision bf16] [--no-kernels]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from finetune import SEED, get_finetune_config  # noqa: E402
from maskedsst_amd import ViTSpatialSpectral  # noqa: E402

B = 256
COPY_TBS = 6.29   # MI355X_MICROARCH.md: measured device copy rate


def build(spectral, precision, device, depth=None):
    config = get_finetune_config(os.path.join(ROOT, "configs/finetune_config_enmap.yaml"), os.path.join(ROOT, "configs/config.yaml"),
                                 SEED, device)
    torch.manual_seed(SEED)
    model = ViTSpatialSpectral(
        image_size=config.image_size - config.patch_sub, spatial_patch_size=config.patch_size,
        spectral_patch_size=config.band_patch_size, num_classes=config.n_classes, dim=config.transformer_dim,
        depth=depth or config.transformer_depth, heads=config.transformer_n_heads, mlp_dim=config.transformer_mlp_dim,
        dropout=config.transformer_dropout, emb_dropout=config.transformer_emb_dropout, channels=config.n_bands,
        spectral_pos=config.spectral_pos, spectral_pos_embed=config.spectral_pos_embed,
        blockwise_patch_embed=config.blockwise_patch_embed, spectral_only=config.spectral_only,
        pixelwise=config.pixelwise, pos_embed_len=config.pos_embed_len, spectral_mlp_head=spectral, precision=precision)
    return config, model.to(device)


def kernels_only(reps):
    """the profiled child: the spectral head's kernels on a fixed y, nothing else"""
    dev = torch.device("cuda")
    _, model = build(True, "fp32", dev, depth=1)
    eng = model.engine()
    eng.ensure()
    S, N, nc = model.num_spectral_patches, model.num_spatial_patches, model.num_classes
    gen = torch.Generator(device="cuda").manual_seed(SEED)
    y = torch.randn(B, S * N, 96, device=dev, generator=gen)
    dl = torch.randn(B, nc, N, device=dev, generator=gen)
    for _ in range(reps):
        eng.spec_head_fwd(y)
        eng.spec_head_bwd(y, dl)
    torch.cuda.synchronize()


def kernel_stats(reps, timeout):
    """rocprofv3 --kernel-trace --stats of `--kernels-only` in a fresh child -> {group: mean us per call}"""
    exe = shutil.which("rocprofv3")
    if exe is None:
        return {"error": "rocprofv3 not found"}
    with tempfile.TemporaryDirectory() as d:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "head", "--",
               sys.executable, os.path.abspath(__file__), "--kernels-only", "--reps", str(reps)]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
        if r.returncode != 0:
            return {"error": f"rocprofv3 exit {r.returncode}: {r.stderr[-400:]}"}
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return {"error": "no kernel_stats.csv"}
        rows = list(csv.DictReader(open(files[0])))
    groups = {"fwd": ["spec_head_fwd_kernel"],
              "bwd_rows": ["spec_head_bwd_rows_kernel"], "bwd_wgrad": ["spec_head_wgrad_kernel"],
              "bwd_reduce": ["reduce_segs_kernel"], "bwd_finish": ["spec_head_wgrad_finish_kernel"]}
    out = {}
    for g, keys in groups.items():
        tot = sum(float(rw["TotalDurationNs"]) for rw in rows if any(k in rw["Name"] for k in keys))
        out[g] = tot / 1e3 / reps
    out["bwd"] = sum(out[g] for g in ("bwd_rows", "bwd_wgrad", "bwd_reduce", "bwd_finish"))
    return out


def step_times(precision, steps, warmup):
    from maskedsst_amd.optim import FusedAdamW
    import torch.nn.functional as F
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(SEED)
    models = {}
    for name, spectral in (("default", False), ("spectral", True)):
        config, model = build(spectral, precision, dev)
        models[name] = (model, FusedAdamW(model, lr=config.lr, weight_decay=5e-3))
    x = torch.randn(B, config.n_bands, 8, 8, generator=gen).to(dev)
    label = torch.randint(-1, config.n_classes, (B, 8, 8), generator=gen).to(dev)

    def step(name):
        model, opt = models[name]
        opt.zero_grad()
        F.cross_entropy(model(x), label, ignore_index=-1).backward()
        opt.step()

    for _ in range(warmup):
        for name in models:
            step(name)
    t = {name: [] for name in models}
    for _ in range(steps):
        for name in models:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(name)
            torch.cuda.synchronize()
            t[name].append(time.perf_counter() - t0)
    return {name: round(1e3 * statistics.median(v), 3) for name, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--reps", type=int, default=50, help="head calls of the profiled child")
    ap.add_argument("--no-kernels", action="store_true", help="skip the rocprofv3 child")
    ap.add_argument("--kernels-only", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.kernels_only:
        kernels_only(args.reps)
        return
    S, N = 20, 64
    y_bytes = B * S * N * 96 * 4
    res = dict(tool="head_time", shape=dict(B=B, S=S, N=N, F=96 * S, n_classes=8), precision=args.precision)
    if not args.no_kernels:   # the child runs first, before this process opens the GPU
        k = kernel_stats(args.reps, timeout=600)
        if "error" not in k:
            for g, nbytes in (("fwd", y_bytes), ("bwd", 2 * y_bytes)):
                floor_us = nbytes / (COPY_TBS * 1e12) * 1e6
                k[g + "_GBps"] = round(nbytes / (k[g] * 1e-6) / 1e9, 1)
                k[g + "_floor_us"] = round(floor_us, 2)
                k[g + "_x_floor"] = round(k[g] / floor_us, 2)
            k = {a: (round(v, 2) if isinstance(v, float) else v) for a, v in k.items()}
        res["kernels_us"] = k
    st = step_times(args.precision, args.steps, args.warmup)
    res["step_ms"] = st
    res["spectral_over_default"] = round(st["spectral"] / st["default"], 4)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
