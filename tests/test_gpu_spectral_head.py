"""GPU: the spectral MLP head (ViTSpatialSpectral(spectral_mlp_head=True), msst_spec_head_fwd / _bwd) -- the classifier step against
a CPU reference and the reference captures of tools/make_golden_spectral_head.py, the head kernels alone at the EnMAP finetune size
against float64 autograd (and bitwise reproducibility), bf16 training, predict_scene, SimMIM pre-training and the scripts."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, oracle_cfg_from, seed_all, ROOT
from util import record, relerr, rel_l2, spectral_head_ref

pytestmark = pytest.mark.gpu

CASES = ["spechead_200b_L4_B2.npz", "spechead_50b_L2_B2_specpos.npz", "spechead_30b_L1_B2_img6_h2.npz"]


def spectral_encoder(cfg, n_classes=None, spectral_mlp_head=True, precision="fp32"):
    from maskedsst_amd import ViTSpatialSpectral
    return ViTSpatialSpectral(
        image_size=cfg.get("image_size", 8), spatial_patch_size=1, spectral_patch_size=10,
        num_classes=n_classes or cfg["n_classes"], dim=96, depth=cfg["depth"], heads=cfg.get("heads", 8), mlp_dim=64,
        dropout=0.0, emb_dropout=0.0, channels=cfg["bands"], spectral_pos_embed=cfg.get("spectral_pos_embed", False),
        spectral_pos=torch.arange(cfg["bands"] // 10), blockwise_patch_embed=True, spectral_mlp_head=spectral_mlp_head,
        precision=precision)


def classify_ref(params, img, cfg):
    from oracle.model import encoder_embed, pos_table, transformer_forward
    ocfg = oracle_cfg_from(cfg)
    _, tok = encoder_embed(params, img, ocfg)
    y = transformer_forward(params, tok + pos_table(params, ocfg), ocfg)
    return spectral_head_ref(y, params["encoder.mlp_head.0.weight"], params["encoder.mlp_head.0.bias"],
                             params["encoder.mlp_head.1.weight"], params["encoder.mlp_head.1.bias"], ocfg.S, ocfg.Nsq)


@pytest.mark.parametrize("name", CASES)
def test_spectral_head_step_fp32(name):
    g = load_golden(name)
    cfg = g["cfg"]
    seed_all(5)
    enc = spectral_encoder(cfg)
    w = cfg.get("image_size", 8)
    x = torch.randn(cfg["B"], cfg["bands"], w, w)
    label = torch.randint(-1, cfg["n_classes"], (cfg["B"], w, w))
    params = {"encoder." + k: v.detach().clone().requires_grad_(True) for k, v in enc.state_dict().items()}
    ref_logits = classify_ref(params, x, cfg)
    F.cross_entropy(ref_logits, label, ignore_index=-1).backward()
    enc = enc.cuda()
    logits = enc(x.cuda())
    assert logits.shape == (cfg["B"], cfg["n_classes"], w, w)
    loss = F.cross_entropy(logits, label.cuda(), ignore_index=-1)
    loss.backward()
    torch.cuda.synchronize()
    err = relerr(logits, ref_logits)
    assert err < 1e-4, err
    assert relerr(logits, torch.from_numpy(g["logits"])) < 1e-4
    assert abs(loss.item() - float(g["loss"])) <= 1e-4 * abs(float(g["loss"]))
    bad, worst = [], 0.0
    for k, p in enc.named_parameters():
        e = relerr(p.grad, params["encoder." + k].grad)
        worst = max(worst, e)
        if not e < 3e-4:
            bad.append((k, e))
    assert not bad, bad
    gsq = sum(float((p.grad.double() ** 2).sum()) for p in enc.parameters())
    assert abs(gsq ** 0.5 - float(g["grad_l2"])) <= 1e-3 * float(g["grad_l2"])
    record("test_spectral_head_step_fp32", err=err, worst_grad=worst, name=name)


def test_head_kernels_full_size_vs_float64():
    """the head alone at the EnMAP finetune shape (B = 256, S = 20, N = 64, F = 1920, 8 classes): logits, dy and the four head
    gradients against float64 autograd; two backward calls bitwise equal; a 7-sample batch gives the full batch's first 7 rows bit
    for bit"""
    cfg = dict(bands=200, depth=1, n_classes=8, spectral_pos_embed=False)
    seed_all(11)
    enc = spectral_encoder(cfg).cuda()
    with torch.no_grad():   # a non-trivial affine LayerNorm and bias
        enc.mlp_head[0].weight.copy_(1 + 0.5 * torch.randn(1920))
        enc.mlp_head[0].bias.copy_(0.3 * torch.randn(1920))
        enc.mlp_head[1].bias.copy_(torch.randn(8))
    eng = enc.engine()
    eng.ensure()
    B, S, N = 256, 20, 64
    gen = torch.Generator(device="cuda").manual_seed(3)
    y = torch.randn(B, S * N, 96, device="cuda", generator=gen) * 2 + 0.5
    dl = torch.randn(B, 8, N, device="cuda", generator=gen)
    logits = eng.spec_head_fwd(y)
    names = ["mlp_head.0.weight", "mlp_head.0.bias", "mlp_head.1.weight", "mlp_head.1.bias"]
    dy = eng.spec_head_bwd(y, dl)
    grads = [eng.fp.view(n, eng.fp.grad).clone() for n in names]
    dy2 = eng.spec_head_bwd(y, dl)
    grads2 = [eng.fp.view(n, eng.fp.grad).clone() for n in names]
    logits7 = eng.spec_head_fwd(y[:7].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(dy, dy2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))
    assert torch.equal(logits7, logits[:7])
    y64 = y.double().requires_grad_(True)
    p64 = [eng.fp.view(n).detach().double().requires_grad_(True) for n in names]
    ref = spectral_head_ref(y64, *p64, S, 8).reshape(B, 8, N)
    ref.backward(dl.double())
    errs = dict(logits=relerr(logits, ref), dy=relerr(dy, y64.grad))
    for n, gv, p in zip(names, grads, p64):
        errs[n] = relerr(gv, p.grad)
    assert all(e < 1e-4 for e in errs.values()), errs
    record("test_head_kernels_full_size_vs_float64", **{"err_" + k.replace(".", "_"): v for k, v in errs.items()})


def test_spectral_head_bf16_and_optimizer_step():
    """bf16 block kernels (the head itself is fp32 in both modes): 8 FusedAdamW steps reduce the loss; the first logits stay within
    the bar of the fp32 model's"""
    from maskedsst_amd.optim import FusedAdamW
    cfg = dict(bands=50, depth=2, n_classes=20, spectral_pos_embed=False)
    out = {}
    for prec in ("fp32", "bf16"):
        seed_all(5)
        enc = spectral_encoder(cfg, precision=prec).cuda()
        x = torch.randn(4, 50, 8, 8)
        label = torch.randint(-1, 20, (4, 8, 8))
        with torch.no_grad():
            out[prec] = enc(x.cuda())
    err = rel_l2(out["bf16"], out["fp32"])
    # bf16 operands of the blocks: 1.4e-4 rel-L2 measured on an MI355X; bar ~4x
    assert err < 6e-4, err
    opt = FusedAdamW(enc, lr=5e-4, weight_decay=5e-3)
    losses = []
    for _ in range(8):
        opt.zero_grad()
        loss = F.cross_entropy(enc(x.cuda()), label.cuda(), ignore_index=-1)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    record("test_spectral_head_bf16_and_optimizer_step", err=err)


def test_predict_scene_spectral_head():
    """predict_scene with a spectral-head model against the reference's notebook loop (fixture) and against the product's own
    model(window) loop"""
    g = load_golden("spechead_scene_50b_L2_Bs2_40x44.npz")
    cfg = g["cfg"]
    seed_all(5)
    enc = spectral_encoder(cfg)
    scene = torch.randn(cfg["Bs"], cfg["bands"], cfg["Hs"], cfg["Ws"])
    s = scene.double()
    np.testing.assert_allclose([s.sum().item(), s.abs().sum().item()], g["scene_fp"], rtol=1e-12)
    ref_classes = torch.from_numpy(g["classes"].astype(np.int64))
    ref_logits = torch.from_numpy(g["logits"])
    covered = ref_classes >= 0
    enc = enc.cuda()
    classes, logits = enc.predict_scene(scene.cuda(), return_logits=True)
    classes, logits = classes.cpu(), logits.cpu()
    assert torch.equal(classes < 0, ~covered)
    top = ref_logits.topk(2, dim=1).values
    sure = covered & (top[:, 0] - top[:, 1] > 1e-3)
    assert torch.equal(classes[sure], ref_classes[sure])
    err = rel_l2(logits.permute(0, 2, 3, 1)[covered], ref_logits.permute(0, 2, 3, 1)[covered])
    assert err < 1e-4, err
    w = cfg["image_size"]
    loop = torch.zeros_like(logits)
    sc = scene.cuda()
    with torch.no_grad():
        for x in range(0, cfg["Hs"] - w + 1, w):
            for y in range(0, cfg["Ws"] - w + 1, w):
                loop[:, :, x:x + w, y:y + w] = enc(sc.narrow(2, x, w).narrow(3, y, w)).cpu()
    err_loop = rel_l2(logits.permute(0, 2, 3, 1)[covered], loop.permute(0, 2, 3, 1)[covered])
    assert err_loop < 1e-5, err_loop
    record("test_predict_scene_spectral_head", err=err, err_loop=err_loop)


def test_simmim_pretraining_ignores_the_head():
    """a SimMIM-wrapped spectral-head encoder pre-trains exactly as a default-head one with the same weights: bitwise-equal loss
    and gradients of everything but the (unused) head"""
    from maskedsst_amd import SimMIMSpatialSpectral
    cfg = dict(bands=50, depth=2, n_classes=8)
    models = []
    for spectral in (False, True):
        seed_all(5)
        enc = spectral_encoder(cfg, spectral_mlp_head=spectral)
        models.append(SimMIMSpatialSpectral(encoder=enc, masking_ratio=0.7, mask_patch_size=4, tube_masking=True,
                                            to_pixels_per_spectral_block=True))
    dflt, spec = models
    with torch.no_grad():   # the same weights outside the head (the head's different size shifts the later draws)
        sd = spec.state_dict()
        for k, v in dflt.state_dict().items():
            if "mlp_head" not in k:
                sd[k].copy_(v)
    x = torch.randn(4, 50, 8, 8).cuda()
    seed_all(7)
    masks = dflt.draw_masks(4)
    losses, grads = [], []
    for m in (dflt, spec):
        m.cuda()
        loss = m(x, masks=masks)
        loss.backward()
        torch.cuda.synchronize()
        losses.append(loss.detach().clone())
        grads.append({k: p.grad.clone() for k, p in m.named_parameters() if "mlp_head" not in k and p.grad is not None})
    assert torch.equal(losses[0], losses[1])
    assert grads[0].keys() == grads[1].keys() and len(grads[0]) > 0
    assert all(torch.equal(grads[0][k], grads[1][k]) for k in grads[0])
    assert all(p.grad is None for k, p in spec.named_parameters() if "mlp_head" in k)


def test_scripts_spectral_head_checkpoint_handoff(tmp_path):
    """pretrain.py --spectral-mlp-head --save-dir -> finetune.py --spectral-mlp-head --checkpoint: strict load, then training"""
    import subprocess

    def run(cmd):
        e = dict(os.environ)
        e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
        r = subprocess.run(cmd, cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, f"{' '.join(cmd)}\n--- stdout\n{r.stdout[-4000:]}\n--- stderr\n{r.stderr[-4000:]}"
        return r.stdout

    save = str(tmp_path / "ck")
    run([sys.executable, "pretrain.py", "--batch-size", "8", "--tiles", "16", "--epochs", "1", "--pool-tiles", "8",
         "--precision", "fp32", "--spectral-mlp-head", "--save-dir", save])
    files = sorted(os.listdir(save))
    assert files, files
    sd = torch.load(os.path.join(save, files[-1]), map_location="cpu", weights_only=False)["model_state_dict"]
    assert sd["encoder.mlp_head.0.weight"].shape == (1920,)
    out = run([sys.executable, "finetune.py", "enmap", "--steps", "10", "--batch-size", "4", "--precision", "fp32",
               "--spectral-mlp-head", "--checkpoint", os.path.join(save, files[-1])])
    assert "<All keys matched successfully>" in out, out
    last = [l for l in out.splitlines() if l.startswith("step 10 ")]
    assert last and np.isfinite(float(last[0].split()[3])), out
