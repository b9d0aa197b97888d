#!/usr/bin/env python3
"""Golden fixtures of the pixelwise centre-pixel classifier (reference ``ViTSpatialSpectral(..., pixelwise=True)``,
src/vit_spatial_spectral.py:466-478 and :536-564), captured from the reference as small ``.npz`` files under ``tests/golden/``
(the reference Python cannot travel to the GPU box; tests/test_pixelwise_host.py and tests/test_gpu_pixelwise.py read them).

Protocol as tools/make_golden_spectral_head.py::run_case: ``random.seed(5); np.random.seed(5); torch.manual_seed(5)``; build the
reference encoder with ``pixelwise=True`` at an odd image size; ``x = torch.randn(B, bands, w, w)``, ``label = torch.randint(0, nc,
(B, w, w))`` from the same stream; ``eval()``; logits (``[B, nc]``, the reference's squeeze), then the training step's centre label
``label[:, c, c]``, ``c = w // 2`` (src/utils.py:630-636), CE(ignore_index=-1), backward.  Stored per case: the config, the label,
the logits, the loss, ``n_params``, the parameter names, per-parameter fingerprints of the values and of the gradients
(make_golden.py:fp) and ``grad_l2``.  Also:

* ``pixwise_load_checkpoint_*``: the REFERENCE's load_checkpoint from an 8 x 8 SimMIM state_dict into a 7 x 7 pixelwise classifier
  (config.image_size 8, patch_sub 1): with spectral_pos_embed=True (pos_embed keeps its first 49 rows), and with
  spectral_pos_embed=False (the strict load fails on pos_embedding unless the model is built with the checkpoint's pos_embed_len);
* ``pixwise_scene_*``: the DeepHyperX per-pixel loop (test() with test_stride = 1 and 2): every window of the scene through the
  model, its logits and argmax written to the window's centre pixel; every other pixel class -1, logit 0.

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_pixelwise.py
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


def encoder(cfg, n_classes=None, pixelwise=True, image_size=None, pos_embed_len=None):
    return ViTSpatialSpectral(
        image_size=image_size or cfg.get("image_size", 7), spatial_patch_size=1, spectral_patch_size=10,
        num_classes=n_classes or cfg["n_classes"], dim=96, depth=cfg["depth"], heads=cfg.get("heads", 8), mlp_dim=64,
        dropout=0.0, emb_dropout=0.0, channels=cfg["bands"], spectral_pos_embed=cfg["spectral_pos_embed"],
        spectral_pos=torch.arange(cfg["bands"] // 10), blockwise_patch_embed=True, pixelwise=pixelwise,
        pos_embed_len=pos_embed_len)


def run_case(name, cfg):
    seed_all()
    enc = encoder(cfg)
    B, w = cfg["B"], cfg.get("image_size", 7)
    x = torch.randn(B, cfg["bands"], w, w)
    label = torch.randint(0, cfg["n_classes"], (B, w, w))
    enc.eval()
    logits = enc(x)
    loss = F.cross_entropy(logits, label[:, w // 2, w // 2], ignore_index=-1)
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
    np.savez_compressed(os.path.join(OUT, f"pixwise_{name}.npz"), **out)
    print(f"pixwise {name}: logits {tuple(logits.shape)} loss={loss.item():.9e} grad_l2={gsq ** 0.5:.6e} "
          f"n_params={int(out['n_params'])}")


def run_scene(name, cfg):
    """the DeepHyperX per-pixel loop over a scene, at every stride of cfg["strides"]"""
    seed_all()
    w = cfg["image_size"]
    enc = encoder(cfg)
    Bs, Hs, Ws = cfg["Bs"], cfg["Hs"], cfg["Ws"]
    scene = torch.randn(Bs, cfg["bands"], Hs, Ws)
    enc.eval()
    out = {"cfg": np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8)}
    for stride in cfg["strides"]:
        classes = torch.full((Bs, Hs, Ws), -1, dtype=torch.int64)
        logits = torch.zeros(Bs, cfg["n_classes"], Hs, Ws)
        with torch.no_grad():
            for y0 in range(0, Hs - w + 1, stride):
                for x0 in range(0, Ws - w + 1, stride):
                    output = enc(scene.narrow(2, y0, w).narrow(3, x0, w))   # [Bs, nc]
                    classes[:, y0 + w // 2, x0 + w // 2] = output.argmax(dim=1)
                    logits[:, :, y0 + w // 2, x0 + w // 2] = output
        out[f"classes_s{stride}"] = classes.numpy().astype(np.int8)
        out[f"logits_s{stride}"] = logits.numpy().astype(np.float32)
        print(f"pixwise scene {name} stride {stride}: {int((classes >= 0).sum())} centre pixels")
    s = scene.double()
    out["scene_fp"] = np.array([s.sum().item(), s.abs().sum().item()], dtype=np.float64)
    np.savez_compressed(os.path.join(OUT, f"pixwise_scene_{name}.npz"), **out)


def run_load_checkpoint(name, cfg):
    """an 8 x 8 SimMIM state_dict (default head) -> a 7 x 7 pixelwise classifier through the REFERENCE's load_checkpoint:
    spectral_pos_embed=True (pos_embed truncated to its first 49 rows) and spectral_pos_embed=False (pos_embedding: failure
    without pos_embed_len, success with the checkpoint's length)"""
    import tempfile
    _stub_reference_script_imports()
    from src.utils import load_checkpoint

    class Cfg:
        pass

    out = {"cfg": np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8)}
    S = cfg["bands"] // 10
    for spe in (True, False):
        tag = "specpos" if spe else "posemb"
        c_ = dict(cfg, spectral_pos_embed=spe)
        seed_all()
        mim = SimMIMSpatialSpectral(encoder=encoder(c_, cfg["n_classes_pretrain"], pixelwise=False, image_size=8),
                                    intermediate_losses=False, masking_ratio=0.7, mask_patch_size=4,
                                    to_pixels_per_spectral_block=True, tube_masking=True)
        sd = mim.state_dict()
        before_fp = {k: fp(v) for k, v in sd.items()}
        pel = S * 64 + 1 if not spe else None
        enc = encoder(c_, cfg["n_classes_finetune"], pos_embed_len=pel)
        fresh_fp = {k: fp(v) for k, v in enc.state_dict().items()}
        with tempfile.TemporaryDirectory() as d:
            c = Cfg()
            c.patch_sub, c.image_size = 1, 8
            c.checkpoint_path = os.path.join(d, "ck.pth")
            torch.save({"model_state_dict": sd, "losses": torch.zeros(1)}, c.checkpoint_path)
            enc = load_checkpoint(c, enc, "mlp_head", "cpu")
            if not spe:
                try:
                    load_checkpoint(c, encoder(c_, cfg["n_classes_finetune"]), "mlp_head", "cpu")
                    err = "no error"
                except Exception as e:   # noqa: BLE001 -- the reference's own failure is what is captured
                    err = f"{type(e).__name__}: {e}"
                out[f"{tag}/error_without_pos_embed_len"] = np.frombuffer(err.encode(), dtype=np.uint8)
        out[f"{tag}/before"] = np.frombuffer("\n".join(sd.keys()).encode(), dtype=np.uint8)
        after = list(enc.state_dict().keys())
        out[f"{tag}/after"] = np.frombuffer("\n".join(after).encode(), dtype=np.uint8)
        src = []
        for k, v in enc.state_dict().items():
            got = fp(v)
            if np.array_equal(got, before_fp.get("encoder." + k, None)):
                src.append("checkpoint")
            elif np.array_equal(got, fresh_fp[k]):
                src.append("fresh")
            else:
                src.append("other")
            out[f"{tag}/after_fp/" + k] = got
        if spe:   # the kept rows: the FIRST 49 of the 64 (not a spatial crop)
            out[f"{tag}/pos_embed_is_first_rows"] = np.array(
                torch.equal(enc.pos_embed.detach(), sd["encoder.pos_embed"][:, :49]), dtype=np.bool_)
        out[f"{tag}/after_source"] = np.frombuffer("\n".join(src).encode(), dtype=np.uint8)
        print(f"pixwise load_checkpoint {name} {tag}:", {s_: src.count(s_) for s_ in set(src)},
              "| without pos_embed_len:", bytes(out.get(f"{tag}/error_without_pos_embed_len", b"-")).decode()[:160])
    np.savez_compressed(os.path.join(OUT, f"pixwise_load_checkpoint_{name}.npz"), **out)


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(8)
    run_case("200b_L4_B2", dict(bands=200, depth=4, B=2, n_classes=8, spectral_pos_embed=False))          # K = 96 * 49
    run_case("50b_L2_B2_specpos", dict(bands=50, depth=2, B=2, n_classes=20, spectral_pos_embed=True))
    run_case("30b_L1_B3_img5_h2", dict(bands=30, depth=1, B=3, n_classes=20, spectral_pos_embed=False, image_size=5, heads=2))
    run_load_checkpoint("50b_L2", dict(bands=50, depth=2, n_classes_pretrain=8, n_classes_finetune=20))
    run_scene("50b_L2_Bs2_20x22", dict(bands=50, depth=2, n_classes=8, spectral_pos_embed=False, image_size=7, Bs=2, Hs=20, Ws=22,
                                       strides=[1, 2]))
