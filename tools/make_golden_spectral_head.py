#!/usr/bin/env python3
"""Golden fixtures of the spectral MLP head (reference ``ViTSpatialSpectral(..., spectral_mlp_head=True)``,
src/vit_spatial_spectral.py:440-453 and :536-564), captured from the reference as small ``.npz`` files under ``tests/golden/``
(the reference Python cannot travel to the GPU box; tests/test_spectral_head_host.py and tests/test_gpu_spectral_head.py read
them).

Protocol as tools/make_golden.py::run_finetune_case: ``random.seed(5); np.random.seed(5); torch.manual_seed(5)``; build the
reference encoder with ``spectral_mlp_head=True``; ``x = torch.randn(B, bands, H, W)``, ``label = torch.randint(-1, nc, (B, H, W))``
from the same stream; ``eval()``; logits, CE(ignore_index=-1), backward.  Stored per case: the config, the label, the logits,
the loss, ``n_params``, the parameter names, per-parameter fingerprints of the values and of the gradients (make_golden.py:fp)
and ``grad_l2``.  Also:

* ``spechead_scene_*``: the notebook's window loop (tools/make_golden_scene.py) with a spectral-head model;
* ``spechead_load_checkpoint_*``: a spectral-head SimMIM state_dict loaded by the REFERENCE's load_checkpoint into a
  spectral-head classifier with another class count (keys before / after, fingerprints, which tensors are fresh), and the
  error the reference raises when the checkpoint's encoder had the default head.

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_spectral_head.py
"""
import json
import os
import sys

import numpy as np

np.float = float  # reference src/pos_embed.py:52 uses the alias removed in numpy>=1.24

import torch
import torch.nn.functional as F

REF = os.environ.get("MSST_REFERENCE", "/root/reference")
if not os.path.isdir(os.path.join(REF, "src")):
    raise SystemExit(f"the reference sources are not at {REF} (set MSST_REFERENCE): nothing to generate")
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True

from src.vit_spatial_spectral import ViTSpatialSpectral  # noqa: E402
from src.vit_simmim_original import SimMIMSpatialSpectral  # noqa: E402
from make_golden import fp, seed_all, _stub_reference_script_imports  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")


def encoder(cfg, n_classes=None, spectral_mlp_head=True):
    return ViTSpatialSpectral(
        image_size=cfg.get("image_size", 8), spatial_patch_size=1, spectral_patch_size=10,
        num_classes=n_classes or cfg["n_classes"], dim=96, depth=cfg["depth"], heads=cfg.get("heads", 8), mlp_dim=64,
        dropout=0.0, emb_dropout=0.0, channels=cfg["bands"], spectral_pos_embed=cfg["spectral_pos_embed"],
        spectral_pos=torch.arange(cfg["bands"] // 10), blockwise_patch_embed=True, spectral_mlp_head=spectral_mlp_head)


def run_case(name, cfg):
    seed_all()
    enc = encoder(cfg)
    B, w = cfg["B"], cfg.get("image_size", 8)
    x = torch.randn(B, cfg["bands"], w, w)
    label = torch.randint(-1, cfg["n_classes"], (B, w, w))
    enc.eval()
    logits = enc(x)
    loss = F.cross_entropy(logits, label, ignore_index=-1)
    loss.backward()
    out = {
        "cfg": np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8),
        "loss": np.array(loss.item(), dtype=np.float64),
        "label": label.numpy().astype(np.int8),
        "logits": logits.detach().numpy().astype(np.float32),
        "n_params": np.array(sum(p.numel() for p in enc.parameters()), dtype=np.int64),
    }
    gsq = 0.0
    names = []
    for k, p in enc.named_parameters():
        names.append(k)
        out["p_fp/" + k] = fp(p)
        out["g_fp/" + k] = fp(p.grad)
        gsq += float((p.grad.double() ** 2).sum())
    out["names"] = np.frombuffer("\n".join(names).encode(), dtype=np.uint8)
    out["grad_l2"] = np.array(gsq ** 0.5, dtype=np.float64)
    np.savez_compressed(os.path.join(OUT, f"spechead_{name}.npz"), **out)
    print(f"spechead {name}: logits {tuple(logits.shape)} loss={loss.item():.9e} grad_l2={gsq ** 0.5:.6e} "
          f"n_params={int(out['n_params'])}")


def run_scene(name, cfg):
    """tools/make_golden_scene.py::run_case with a spectral-head encoder"""
    seed_all()
    w = cfg["image_size"]
    enc = encoder(cfg)
    Bs, Hs, Ws = cfg["Bs"], cfg["Hs"], cfg["Ws"]
    scene = torch.randn(Bs, cfg["bands"], Hs, Ws)
    enc.eval()
    classes = torch.full((Bs, Hs, Ws), -1, dtype=torch.int64)
    logits = torch.zeros(Bs, cfg["n_classes"], Hs, Ws)
    with torch.no_grad():
        for x in range(0, Hs, w):
            for y in range(0, Ws, w):
                if x + w > Hs or y + w > Ws:
                    continue
                output = enc(scene.narrow(2, x, w).narrow(3, y, w))
                classes[:, x:x + w, y:y + w] = output.argmax(dim=1)
                logits[:, :, x:x + w, y:y + w] = output
    s = scene.double()
    np.savez_compressed(os.path.join(OUT, f"spechead_scene_{name}.npz"),
                        cfg=np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8), classes=classes.numpy().astype(np.int8),
                        logits=logits.numpy().astype(np.float32),
                        scene_fp=np.array([s.sum().item(), s.abs().sum().item()], dtype=np.float64))
    print(f"spechead scene {name}: {int((classes >= 0).sum())} covered pixels")


def run_load_checkpoint(name, cfg):
    """make_golden.py::run_load_checkpoint with spectral-head encoders on both sides; plus the reference's failure for a
    checkpoint whose encoder had the default head"""
    import tempfile
    _stub_reference_script_imports()
    from src.utils import load_checkpoint

    class Cfg:
        pass

    seed_all()
    mim = SimMIMSpatialSpectral(encoder=encoder(cfg, cfg["n_classes_pretrain"]), intermediate_losses=False, masking_ratio=0.7,
                                mask_patch_size=4, to_pixels_per_spectral_block=True, tube_masking=True)
    sd = mim.state_dict()
    before = list(sd.keys())
    before_fp = {k: fp(v) for k, v in sd.items()}
    enc = encoder(cfg, cfg["n_classes_finetune"])
    fresh_fp = {k: fp(v) for k, v in enc.state_dict().items()}
    seed_all()
    mim_default = SimMIMSpatialSpectral(encoder=encoder(cfg, cfg["n_classes_pretrain"], spectral_mlp_head=False),
                                        intermediate_losses=False, masking_ratio=0.7, mask_patch_size=4,
                                        to_pixels_per_spectral_block=True, tube_masking=True)
    with tempfile.TemporaryDirectory() as d:
        c = Cfg()
        c.patch_sub, c.image_size = 0, 8
        c.checkpoint_path = os.path.join(d, "ck.pth")
        torch.save({"model_state_dict": sd, "losses": torch.zeros(1)}, c.checkpoint_path)
        enc = load_checkpoint(c, enc, "mlp_head", "cpu")
        c.checkpoint_path = os.path.join(d, "ck_default.pth")
        torch.save({"model_state_dict": mim_default.state_dict(), "losses": torch.zeros(1)}, c.checkpoint_path)
        try:
            load_checkpoint(c, encoder(cfg, cfg["n_classes_finetune"]), "mlp_head", "cpu")
            err = "no error"
        except Exception as e:   # noqa: BLE001 -- the reference's own failure is what is captured
            err = f"{type(e).__name__}: {e}"
    after = list(enc.state_dict().keys())
    out = {
        "cfg": np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8),
        "before": np.frombuffer("\n".join(before).encode(), dtype=np.uint8),
        "after": np.frombuffer("\n".join(after).encode(), dtype=np.uint8),
        "default_to_spectral_error": np.frombuffer(err.encode(), dtype=np.uint8),
    }
    src = []
    for k, v in enc.state_dict().items():
        got = fp(v)
        if np.array_equal(got, before_fp.get("encoder." + k, None)):
            src.append("checkpoint")
        elif np.array_equal(got, fresh_fp[k]):
            src.append("fresh")
        else:
            src.append("other")
        out["after_fp/" + k] = got
    out["after_source"] = np.frombuffer("\n".join(src).encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(OUT, f"spechead_load_checkpoint_{name}.npz"), **out)
    print(f"spechead load_checkpoint {name}:", {s_: src.count(s_) for s_ in set(src)}, "| default -> spectral:", err[:120])


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(8)
    run_case("200b_L4_B2", dict(bands=200, depth=4, B=2, n_classes=8, spectral_pos_embed=False))             # F = 1920
    run_case("50b_L2_B2_specpos", dict(bands=50, depth=2, B=2, n_classes=20, spectral_pos_embed=True))       # F = 480
    run_case("30b_L1_B2_img6_h2", dict(bands=30, depth=1, B=2, n_classes=8, spectral_pos_embed=False, image_size=6, heads=2))
    run_scene("50b_L2_Bs2_40x44", dict(bands=50, depth=2, n_classes=8, spectral_pos_embed=False, image_size=8, Bs=2, Hs=40, Ws=44))
    run_load_checkpoint("50b_L2", dict(bands=50, depth=2, spectral_pos_embed=False, n_classes_pretrain=8, n_classes_finetune=20))
