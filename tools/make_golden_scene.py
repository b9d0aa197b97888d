#!/usr/bin/env python3
"""Golden fixtures of scene inference: the reference (HSG-AIML/MaskedSST) encoder applied to whole scenes with the window
loop of its ``inference_example.ipynb``, captured as small ``.npz`` files under ``tests/golden/`` (the reference Python
cannot travel to the GPU box; tests/test_gpu_scene.py compares ``ViTSpatialSpectral.predict_scene`` against them).

Protocol: ``random.seed(5); np.random.seed(5); torch.manual_seed(5)``; build the reference ``ViTSpatialSpectral`` in the
draw order of tests/test_gpu_finetune.py::build_encoder, draw the scenes ``torch.randn(Bs, bands, Hs, Ws)`` from the same
stream, ``eval()``, then the notebook's loop: windows of ``image_size`` at origins 0, image_size, 2 image_size, ... (rows
outer, columns inner; windows that do not fit skipped), ``model(window)`` per window, ``argmax(dim=1)`` into the class map.
Stored per case: the config, the class map (int8; -1 where no window reaches), the logit map (fp32 window outputs placed
in the scene; 0 where no window reaches) and the scenes' fingerprint.

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_scene.py
"""
import json
import os
import random
import sys

import numpy as np

np.float = float  # reference src/pos_embed.py:52 uses the alias removed in numpy>=1.24

import torch

REF = os.environ.get("MSST_REFERENCE", "/root/reference")
if not os.path.isdir(os.path.join(REF, "src")):
    raise SystemExit(f"the reference sources are not at {REF} (set MSST_REFERENCE): nothing to generate")
sys.path.insert(0, REF)
sys.dont_write_bytecode = True

from src.vit_spatial_spectral import ViTSpatialSpectral  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
SEED = 5


def seed_all():
    random.seed(SEED)
    np.random.seed(SEED)
    torch.manual_seed(SEED)


def run_case(name, cfg):
    seed_all()
    w = cfg["image_size"]
    enc = ViTSpatialSpectral(
        image_size=w, spatial_patch_size=1, spectral_patch_size=10, num_classes=cfg["n_classes"], dim=96,
        depth=cfg["depth"], heads=8, mlp_dim=64, dropout=0.0, emb_dropout=0.0, channels=cfg["bands"],
        spectral_pos_embed=cfg["spectral_pos_embed"], spectral_pos=torch.arange(cfg["bands"] // 10),
        blockwise_patch_embed=True)
    Bs, Hs, Ws = cfg["Bs"], cfg["Hs"], cfg["Ws"]
    scene = torch.randn(Bs, cfg["bands"], Hs, Ws)
    enc.eval()
    classes = torch.full((Bs, Hs, Ws), -1, dtype=torch.int64)
    logits = torch.zeros(Bs, cfg["n_classes"], Hs, Ws)
    with torch.no_grad():
        for x in range(0, Hs, w):            # the notebook's loop (its 64 x 64 generalised to Hs x Ws)
            for y in range(0, Ws, w):
                if x + w > Hs or y + w > Ws:
                    continue
                img = scene.narrow(2, x, w).narrow(3, y, w)
                output = enc(img)
                classes[:, x:x + w, y:y + w] = output.argmax(dim=1)
                logits[:, :, x:x + w, y:y + w] = output
    s = scene.double()
    out = {
        "cfg": np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8),
        "classes": classes.numpy().astype(np.int8),
        "logits": logits.numpy().astype(np.float32),
        "scene_fp": np.array([s.sum().item(), s.abs().sum().item()], dtype=np.float64),
    }
    np.savez_compressed(os.path.join(OUT, f"scene_{name}.npz"), **out)
    print(f"scene {name}: {int((classes >= 0).sum())} covered pixels, logit map abs-sum {float(logits.double().abs().sum()):.6e}")


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(8)
    run_case("50b_L2_Bs2_64x64", dict(bands=50, depth=2, n_classes=8, spectral_pos_embed=False, image_size=8, Bs=2, Hs=64, Ws=64))
    run_case("50b_L2_Bs2_40x44", dict(bands=50, depth=2, n_classes=8, spectral_pos_embed=False, image_size=8, Bs=2, Hs=40, Ws=44))
