#!/usr/bin/env python3
"""Scene inference timing (GPU box): ViTSpatialSpectral.predict_scene against the notebook's per-window loop
(reference inference_example.ipynb: model(scene.narrow(2, x, w).narrow(3, y, w)) per window, argmax into the class map)
with the product model of the shipped EnMAP finetune configuration (200 bands, depth 4, 8 heads, image_size 8), on the
same seeded 64 x 64 scenes, Bs in {2, 16}.

Both methods are warmed up, then timed alternately in one process (device-synchronised wall clock per repetition; the
median is reported).  Prints ONE JSON line: windows/s of each method per Bs and the largest |logit| difference between them.

Run:  python tools/scene_time.py [--reps 5] [--precision bf16]
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

from finetune import SEED, get_finetune_config  # noqa: E402
from maskedsst_amd import ViTSpatialSpectral  # noqa: E402


def build(precision, device):
    config = get_finetune_config(os.path.join(ROOT, "configs/finetune_config_enmap.yaml"), os.path.join(ROOT, "configs/config.yaml"),
                                 SEED, device)
    torch.manual_seed(SEED)
    model = ViTSpatialSpectral(
        image_size=config.image_size - config.patch_sub, spatial_patch_size=config.patch_size,
        spectral_patch_size=config.band_patch_size, num_classes=config.n_classes, dim=config.transformer_dim,
        depth=config.transformer_depth, heads=config.transformer_n_heads, mlp_dim=config.transformer_mlp_dim,
        dropout=config.transformer_dropout, emb_dropout=config.transformer_emb_dropout, channels=config.n_bands,
        spectral_pos=config.spectral_pos, spectral_pos_embed=config.spectral_pos_embed,
        blockwise_patch_embed=config.blockwise_patch_embed, spectral_only=config.spectral_only,
        pixelwise=config.pixelwise, pos_embed_len=config.pos_embed_len, precision=precision)
    return config, model.to(device).eval()


def notebook(model, scene, w):
    Bs, _, Hs, Ws = scene.shape
    logits = torch.zeros(Bs, model.num_classes, Hs, Ws, device=scene.device)
    classes = torch.zeros(Bs, Hs, Ws, dtype=torch.int64, device=scene.device)
    with torch.no_grad():
        for x in range(0, Hs, w):
            for y in range(0, Ws, w):
                if x + w > Hs or y + w > Ws:
                    continue
                out = model(scene.narrow(2, x, w).narrow(3, y, w))
                logits[:, :, x:x + w, y:y + w] = out
                classes[:, x:x + w, y:y + w] = out.argmax(dim=1)
    return classes, logits


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--bs", default="2,16")
    args = ap.parse_args()
    device = torch.device("cuda")
    config, model = build(args.precision, device)
    w = model.num_spatial_patches_sqrt
    gen = torch.Generator().manual_seed(SEED)
    rows = []
    for Bs in [int(b) for b in args.bs.split(",")]:
        scene = torch.randn(Bs, config.n_bands, 64, 64, generator=gen).to(device)
        nwin = Bs * ((64 - w) // w + 1) ** 2
        fast = lambda: model.predict_scene(scene, return_logits=True)   # noqa: E731
        slow = lambda: notebook(model, scene, w)                        # noqa: E731
        for _ in range(2):   # warm-up: weight copies, guards, allocator
            fast()
            slow()
        tf, ts = [], []
        for _ in range(args.reps):
            t, (cf, lf) = timed(fast)
            tf.append(t)
            t, (cs, ls) = timed(slow)
            ts.append(t)
        diff = float((lf - ls).abs().max())
        agree = float((cf == cs).double().mean())
        mf, ms = statistics.median(tf), statistics.median(ts)
        rows.append(dict(Bs=Bs, windows=nwin, predict_scene_windows_per_s=round(nwin / mf, 1),
                         notebook_windows_per_s=round(nwin / ms, 1), speedup=round(ms / mf, 2),
                         max_abs_logit_diff=diff, class_agreement=agree,
                         predict_scene_ms=round(1e3 * mf, 3), notebook_ms=round(1e3 * ms, 3)))
    print(json.dumps(dict(tool="scene_time", precision=args.precision, bands=config.n_bands, depth=config.transformer_depth,
                          image_size=w, reps=args.reps, results=rows)), flush=True)


if __name__ == "__main__":
    main()
