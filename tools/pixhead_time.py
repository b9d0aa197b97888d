#!/usr/bin/env python3
"""Pixelwise-head timing (GPU box) at the EnMAP finetune shape (200 bands, depth 4, B = 256, S = 20, N = 49: windows of 7 x 7):

* the head kernels alone, from a separate ``rocprofv3 --kernel-trace --stats`` run of this script in a fresh child process per
  class count (``--kernels-only``: msst_pix_head_fwd / _bwd on a fixed y, nothing else launched), for 8 and 20 classes: mean
  microseconds per call of the forward (its two launches) and of the backward (its two launches), against the byte floor at the
  6.29 TB/s copy rate -- y read once (forward), y read and dy written (backward);
* the tokenizer at N = 49 in the same children (the scene path's generic kernel; the fp32-MFMA one is built for N = 64 only);
* the finetune step (forward + backward + FusedAdamW, device-synchronised wall clock, median) of the default head at 8 x 8 and
  of the pixelwise head at 7 x 7, timed alternately in one process;
* predict_scene in per-pixel mode (stride 1) on four 64 x 64 scenes: windows per second.

Prints ONE JSON line.  Run:  python tools/pixhead_time.py [--steps 20] [--precision bf16] [--no-kernels]
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


def build(pixelwise, precision, device, depth=None, n_classes=None):
    config = get_finetune_config(os.path.join(ROOT, "configs/finetune_config_enmap.yaml"), os.path.join(ROOT, "configs/config.yaml"),
                                 SEED, device, pixelwise=pixelwise)
    torch.manual_seed(SEED)
    model = ViTSpatialSpectral(
        image_size=config.image_size - config.patch_sub, spatial_patch_size=config.patch_size,
        spectral_patch_size=config.band_patch_size, num_classes=n_classes or config.n_classes, dim=config.transformer_dim,
        depth=depth or config.transformer_depth, heads=config.transformer_n_heads, mlp_dim=config.transformer_mlp_dim,
        dropout=config.transformer_dropout, emb_dropout=config.transformer_emb_dropout, channels=config.n_bands,
        spectral_pos=config.spectral_pos, spectral_pos_embed=config.spectral_pos_embed,
        blockwise_patch_embed=config.blockwise_patch_embed, spectral_only=config.spectral_only,
        pixelwise=config.pixelwise, pos_embed_len=config.pos_embed_len, precision=precision)
    return config, model.to(device)


def kernels_only(reps, nc):
    """the profiled child: the pixelwise head's kernels and the tokenizer on fixed inputs, nothing else"""
    dev = torch.device("cuda")
    _, model = build(True, "fp32", dev, depth=1, n_classes=nc)
    eng = model.engine()
    eng.ensure()
    S, N = model.num_spectral_patches, model.num_spatial_patches
    gen = torch.Generator(device="cuda").manual_seed(SEED)
    y = torch.randn(B, S * N, 96, device=dev, generator=gen)
    dl = torch.randn(B, nc, device=dev, generator=gen)
    img = torch.randn(B, S * 10, 7, 7, device=dev, generator=gen)
    eng.prep_weights()
    for _ in range(reps):
        eng.pix_head_fwd(y)
        eng.pix_head_bwd(y, dl)
        eng.tokenize(img, None)
    torch.cuda.synchronize()


def kernel_stats(reps, nc, timeout):
    """rocprofv3 --kernel-trace --stats of `--kernels-only` in a fresh child -> {group: mean us per call}"""
    exe = shutil.which("rocprofv3")
    if exe is None:
        return {"error": "rocprofv3 not found"}
    with tempfile.TemporaryDirectory() as d:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "pixhead", "--",
               sys.executable, os.path.abspath(__file__), "--kernels-only", "--reps", str(reps), "--nc", str(nc)]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
        if r.returncode != 0:
            return {"error": f"rocprofv3 exit {r.returncode}: {r.stderr[-400:]}"}
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return {"error": "no kernel_stats.csv"}
        rows = list(csv.DictReader(open(files[0])))
    groups = {"fwd_norm": ["pix_head_norm_kernel"], "fwd_logits": ["pix_head_logits_kernel"],
              "bwd_rows": ["pix_head_bwd_kernel"], "bwd_reduce": ["reduce_segs_kernel"], "tokenize_n49": ["tokenize_fwd"]}
    out = {}
    for g, keys in groups.items():
        tot = sum(float(rw["TotalDurationNs"]) for rw in rows if any(k in rw["Name"] for k in keys))
        out[g] = tot / 1e3 / reps
    out["fwd"] = out["fwd_norm"] + out["fwd_logits"]
    out["bwd"] = out["bwd_rows"] + out["bwd_reduce"]
    return out


def step_times(precision, steps, warmup):
    from maskedsst_amd.optim import FusedAdamW
    import torch.nn.functional as F
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(SEED)
    models = {}
    for name, pixelwise in (("default", False), ("pixelwise", True)):
        config, model = build(pixelwise, precision, dev)
        models[name] = (model, FusedAdamW(model, lr=config.lr, weight_decay=5e-3))
    x = torch.randn(B, config.n_bands, 8, 8, generator=gen).to(dev)
    label = torch.randint(-1, config.n_classes, (B, 8, 8), generator=gen).to(dev)
    data = {"default": (x, label), "pixelwise": (x[:, :, :7, :7].contiguous(), label[:, 3, 3].clamp(min=0).contiguous())}

    def step(name):
        model, opt = models[name]
        xi, li = data[name]
        opt.zero_grad()
        F.cross_entropy(model(xi), li, ignore_index=-1).backward()
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
    return {name: round(1e3 * statistics.median(v), 3) for name, v in t.items()}, models["pixelwise"][0]


def scene_rate(model, reps=3):
    dev = torch.device("cuda")
    gen = torch.Generator(device="cuda").manual_seed(SEED)
    scene = torch.randn(4, 200, 64, 64, device=dev, generator=gen)
    model.eval()
    model.predict_scene(scene)
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        model.predict_scene(scene)
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    windows = 4 * (64 - 7 + 1) ** 2
    return dict(scenes=4, size=64, windows=windows, ms=round(1e3 * statistics.median(t), 2),
                windows_per_s=round(windows / statistics.median(t), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--reps", type=int, default=50, help="head calls of the profiled child")
    ap.add_argument("--nc", type=int, default=8, help=argparse.SUPPRESS)
    ap.add_argument("--no-kernels", action="store_true", help="skip the rocprofv3 children")
    ap.add_argument("--kernels-only", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.kernels_only:
        kernels_only(args.reps, args.nc)
        return
    S, N = 20, 49
    y_bytes = B * S * N * 96 * 4
    res = dict(tool="pixhead_time", shape=dict(B=B, S=S, N=N, K=96 * N), precision=args.precision)
    if not args.no_kernels:   # the children run first, before this process opens the GPU
        res["kernels_us"] = {}
        for nc in (8, 20):
            k = kernel_stats(args.reps, nc, timeout=600)
            if "error" not in k:
                for g, nbytes in (("fwd", y_bytes), ("bwd", 2 * y_bytes)):
                    floor_us = nbytes / (COPY_TBS * 1e12) * 1e6
                    k[g + "_floor_us"] = floor_us
                    k[g + "_x_floor"] = k[g] / floor_us
                k = {a: (round(v, 2) if isinstance(v, float) else v) for a, v in k.items()}
            res["kernels_us"][f"nc{nc}"] = k
    st, pix_model = step_times(args.precision, args.steps, args.warmup)
    res["step_ms"] = st
    res["pixelwise_over_default"] = round(st["pixelwise"] / st["default"], 4)
    res["predict_scene_per_pixel"] = scene_rate(pix_model)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
