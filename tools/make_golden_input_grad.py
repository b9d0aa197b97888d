#!/usr/bin/env python3
"""Golden fixtures of the input gradient d(loss)/d(img), captured from the reference with torch autograd
(``img.requires_grad_()``) as small ``.npz`` files under ``tests/golden/`` (the reference Python cannot travel to the GPU box;
tests/test_input_grad_host.py and tests/test_gpu_input_grad.py read them).

Protocol as tools/make_golden.py: ``random.seed(5); np.random.seed(5); torch.manual_seed(5)``; build the reference
model; ``x = torch.randn(B, bands, w, w)`` (classifier cases: then ``label = torch.randint(...)``) from the same stream; ``eval()``;
forward with ``x.requires_grad_()``; backward.  Stored per case: the config, the input, the masks and indices (SimMIM) or the labels
(classifier), the loss and the reference's ``img.grad``.  The parameters are not stored -- a 50-band depth-2 state dict alone is
4 MB, the fixtures of this directory stay near 100 KB -- but pinned like their neighbours': the seed-5 construction reproduces them
(tests/util.py::build_product), and per-parameter fingerprints (make_golden.py:fp) say so.

Cases:
* ``simmim_50b_L2_tube`` (B starts at 4): tube masks; rows >= 1 carry the reference's index quirk.  The tool asserts that some
  row names a token outside its own mask (enlarging B until one does) and records how many rows name a token twice.  That count
  is 0 and stays 0 for any B: a row's list is the tail of one sample's sorted mask list followed by the head of the next one's,
  always 16 list positions apart (240 masked, 224 taken), and two masks of three 4 x 4 quadrants out of four place a list
  position at most 16 tokens apart -- so the tests that need a token named twice build such an index row themselves.
* ``simmim_50b_L2_B4_mps1``: ``mask_patch_size=1`` (torch.rand topk), non-tube.
* ``cls_50b_L2_B2_specpos``: default head, ``spectral_pos_embed=True``, CE with labels in {-1 .. 7}.
* ``pixwise_30b_L1_B3_img5_h2`` / ``spechead_30b_L1_B2_img6_h2``: the pixelwise and the spectral MLP head at the sizes of the
  existing fixtures of those names.

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_input_grad.py
"""
import json
import os
import sys

import numpy as np

np.float = float  # reference src/pos_embed.py:52 uses the alias removed in numpy>=1.24

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True

# make_golden puts the reference sources (MSST_REFERENCE, or its default place) on sys.path and imports them
from make_golden import build, fp, seed_all, staged_forward  # noqa: E402
from src.vit_spatial_spectral import ViTSpatialSpectral  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")


def quirk_counts(bm, idx):
    """(rows that name some token twice, rows that name a token outside their own mask)"""
    dup = sum(int(len(np.unique(r)) < len(r)) for r in idx)
    foreign = sum(int((~bm[b][idx[b]]).any()) for b in range(len(idx)))
    return dup, foreign


def run_simmim(name, cfg, want_quirk=False):
    while True:
        seed_all()
        model = build(cfg)
        w = cfg.get("image_size", 8)
        x = torch.randn(cfg["B"], cfg["bands"], w, w)
        model.eval()
        x.requires_grad_(True)
        st = staged_forward(model, x)
        bm, idx = st["bool_mask"].numpy(), st["masked_indices"].numpy()
        dup, foreign = quirk_counts(bm, idx)
        if not want_quirk or foreign > 0:
            break
        assert cfg["B"] < 16, "no row names a token outside its own mask up to B = 16"
        cfg = dict(cfg, B=cfg["B"] + 1)
    st["loss"].backward()
    out = {
        "cfg": np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8),
        "x": x.detach().numpy().astype(np.float32),
        "bool_mask_bits": np.packbits(bm.astype(np.uint8), axis=1),
        "masked_indices": idx.astype(np.int16),
        "loss": np.array(st["loss"].item(), dtype=np.float64),
        "img_grad": x.grad.numpy().astype(np.float32),
        "quirk": np.array([dup, foreign], dtype=np.int64),
    }
    for k, p in model.named_parameters():
        out["p_fp/" + k] = fp(p)
    np.savez_compressed(os.path.join(OUT, f"input_grad_{name}.npz"), **out)
    print(f"input_grad {name}: B={cfg['B']} loss={st['loss'].item():.9e} |img.grad|={x.grad.norm().item():.6e} "
          f"rows with duplicates {dup}, with foreign tokens {foreign}")


def run_classifier(name, cfg):
    seed_all()
    w = cfg["image_size"]
    enc = ViTSpatialSpectral(
        image_size=w, spatial_patch_size=1, spectral_patch_size=10, num_classes=cfg["n_classes"], dim=96, depth=cfg["depth"],
        heads=cfg.get("heads", 8), mlp_dim=64, dropout=0.0, emb_dropout=0.0, channels=cfg["bands"],
        spectral_pos_embed=cfg["spectral_pos_embed"], spectral_pos=torch.arange(cfg["bands"] // 10), blockwise_patch_embed=True,
        pixelwise=cfg.get("pixelwise", False), spectral_mlp_head=cfg.get("spectral_mlp_head", False))
    B = cfg["B"]
    x = torch.randn(B, cfg["bands"], w, w)
    label = torch.randint(cfg["label_low"], cfg["n_classes"], (B, w, w))
    enc.eval()
    x.requires_grad_(True)
    logits = enc(x)
    loss = F.cross_entropy(logits, label[:, w // 2, w // 2] if cfg.get("pixelwise") else label, ignore_index=-1)
    loss.backward()
    out = {
        "cfg": np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8),
        "x": x.detach().numpy().astype(np.float32),
        "label": label.numpy().astype(np.int8),
        "loss": np.array(loss.item(), dtype=np.float64),
        "logits": logits.detach().numpy().astype(np.float32),
        "img_grad": x.grad.numpy().astype(np.float32),
    }
    for k, p in enc.named_parameters():
        out["p_fp/" + k] = fp(p)
    np.savez_compressed(os.path.join(OUT, f"input_grad_{name}.npz"), **out)
    print(f"input_grad {name}: logits {tuple(logits.shape)} loss={loss.item():.9e} |img.grad|={x.grad.norm().item():.6e}")


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(8)
    run_simmim("simmim_50b_L2_tube", dict(bands=50, depth=2, B=4), want_quirk=True)
    run_simmim("simmim_50b_L2_B4_mps1", dict(bands=50, depth=2, B=4, mask_patch_size=1, tube_masking=False))
    run_classifier("cls_50b_L2_B2_specpos", dict(bands=50, depth=2, B=2, n_classes=8, spectral_pos_embed=True, image_size=8,
                                                 label_low=-1))
    run_classifier("pixwise_30b_L1_B3_img5_h2", dict(bands=30, depth=1, B=3, n_classes=8, spectral_pos_embed=False, image_size=5,
                                                     heads=2, pixelwise=True, label_low=0))
    run_classifier("spechead_30b_L1_B2_img6_h2", dict(bands=30, depth=1, B=2, n_classes=8, spectral_pos_embed=False, image_size=6,
                                                      heads=2, spectral_mlp_head=True, label_low=-1))
