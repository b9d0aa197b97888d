"""Pin the CPU oracle at spectral patch depths other than 10 (OracleConfig(spectral_patch=P)) against the reference captures of
tools/make_golden.py patch (P = 5 and P = 16): the SimMIM step at the bars of tests/test_oracle_golden.py::test_simmim_matches_reference
and the default-head classifier step at those of test_finetune_step.  (The fixtures are not named simmim_*: test_oracle_golden.py
builds its configuration without a spectral patch depth.)"""
import json

import numpy as np
import pytest
import torch

from conftest import load_golden, fp_np, seed_all
from oracle import init_params, simmim_forward, classify_forward
from test_oracle_golden import check_fp
from util import oracle_cfg

FIXTURES = ["patch_P5_50b_L1_B2.npz", "patch_P16_64b_L1_B3_img6_mps2_h2.npz"]


@pytest.mark.parametrize("name", FIXTURES)
def test_simmim_matches_reference(name):
    g = load_golden(name)
    cfg = oracle_cfg(g["cfg"])
    assert cfg.spectral_patch == g["cfg"]["spectral_patch"] != 10
    seed_all(5)
    params = init_params(cfg)
    x = torch.randn(g["cfg"]["B"], cfg.bands, cfg.image_size, cfg.image_size)
    for p in params.values():
        p.requires_grad_(True)
    out = simmim_forward(params, x, cfg)
    out["loss"].backward()
    np.testing.assert_array_equal(fp_np(x), g["x_fp"])
    assert list(params.keys()) == g["names"]
    assert sum(p.numel() for p in params.values()) == int(g["n_params"])
    for k, p in params.items():
        np.testing.assert_array_equal(fp_np(p), g["p_fp/" + k], err_msg=k)
    assert params["encoder.to_patch_embedding.pre_norm.weight"].shape == (cfg.spectral_patch,)
    np.testing.assert_array_equal(np.packbits(out["bool_mask"].numpy().astype(np.uint8), axis=-1), g["bool_mask_bits"])
    np.testing.assert_array_equal(out["masked_indices"].numpy().astype(np.int16), g["masked_indices"])
    assert abs(out["loss"].item() - float(g["loss"])) <= 2e-6 * abs(float(g["loss"])) + 1e-10
    for k in ["tok_embed", "tok_masked", "after_spatial", "enc_out", "pred", "target"]:
        check_fp(fp_np(out[k]), g["i_fp/" + k], 1e-5, 2e-6, k)
        flat = out[k].detach().reshape(-1)
        stride = max(1, flat.numel() // 64)
        want = g["i_slice/" + k]
        np.testing.assert_allclose(flat[::stride][:64].numpy(), want, rtol=2e-4, atol=2e-5 * max(1.0, float(np.abs(want).max())), err_msg=k)
    gsq = 0.0
    for k, p in params.items():
        if ("g_none/" + k) in g:
            assert p.grad is None or float(p.grad.abs().sum()) == 0.0, k
            continue
        ref = g["g_fp/" + k]
        got = fp_np(p.grad)
        scale = max(ref[1] / max(ref[2], 1), 1e-12)
        assert abs(got[0] - ref[0]) <= 2e-3 * ref[1] + 1e-12, (k, got[0], ref[0])
        assert abs(got[1] - ref[1]) <= 2e-4 * ref[1] + 1e-12, (k, got[1], ref[1])
        np.testing.assert_allclose(got[3:], ref[3:], rtol=5e-3, atol=50 * scale * 1e-3, err_msg=k)
        gsq += float((p.grad.double() ** 2).sum())
    assert abs(gsq ** 0.5 - float(g["grad_l2"])) <= 1e-4 * float(g["grad_l2"])


@pytest.mark.parametrize("name", FIXTURES)
def test_finetune_step_matches_reference(name):
    g = load_golden(name)
    ft = json.loads(bytes(g["ft/cfg"]).decode())
    cfg = oracle_cfg(ft)
    assert cfg.spectral_patch == ft["spectral_patch"] != 10
    seed_all(5)
    params = init_params(cfg, with_mim=False)  # bare encoder: x / labels are drawn right after it
    w = cfg.image_size
    x = torch.randn(ft["B"], cfg.bands, w, w)
    label = torch.randint(-1, cfg.n_classes, (ft["B"], w, w))
    np.testing.assert_array_equal(label.numpy().astype(np.int8), g["ft/label"])
    assert sum(p.numel() for p in params.values()) == int(g["ft/n_params"])
    for p in params.values():
        p.requires_grad_(True)
    logits = classify_forward(params, x, cfg)
    loss = torch.nn.functional.cross_entropy(logits, label, ignore_index=-1)
    loss.backward()
    assert abs(loss.item() - float(g["ft/loss"])) < 1e-5 * abs(float(g["ft/loss"]))
    check_fp(fp_np(logits), g["ft/logits_fp"], 1e-5, 2e-6, "logits")
    for k, p in params.items():
        ref = g["ft/g_fp/" + k[len("encoder."):]]
        got = fp_np(p.grad)
        assert abs(got[1] - ref[1]) <= 5e-4 * ref[1] + 1e-12, (k, got[1], ref[1])
    gsq = sum(float((p.grad.double() ** 2).sum()) for p in params.values())
    assert abs(gsq ** 0.5 - float(g["ft/grad_l2"])) <= 2e-4 * float(g["ft/grad_l2"])
