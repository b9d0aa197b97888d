"""GPU: the pixelwise centre-pixel classifier (ViTSpatialSpectral(pixelwise=True), msst_pix_head_fwd / _bwd,
msst_scene_centre_assemble) -- the classifier step against the oracle and the reference captures of tools/make_golden_pixelwise.py,
the head kernels alone at the EnMAP finetune size against float64 autograd (and bitwise reproducibility), bf16 training against the
oracle, dense per-pixel predict_scene, the scripts; and the default-head encoder at 7 x 7 (N = 49) against the oracle."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, oracle_cfg_from, seed_all, ROOT
from util import relerr, rel_l2, pix_head_ref

pytestmark = pytest.mark.gpu

CASES = ["pixwise_200b_L4_B2.npz", "pixwise_50b_L2_B2_specpos.npz", "pixwise_30b_L1_B3_img5_h2.npz"]


def pixelwise_encoder(cfg, n_classes=None, pixelwise=True, precision="fp32", image_size=None):
    from maskedsst_amd import ViTSpatialSpectral
    return ViTSpatialSpectral(
        image_size=image_size or cfg.get("image_size", 7), spatial_patch_size=1, spectral_patch_size=10,
        num_classes=n_classes or cfg["n_classes"], dim=96, depth=cfg["depth"], heads=cfg.get("heads", 8), mlp_dim=64,
        dropout=0.0, emb_dropout=0.0, channels=cfg["bands"], spectral_pos_embed=cfg.get("spectral_pos_embed", False),
        spectral_pos=torch.arange(cfg["bands"] // 10), blockwise_patch_embed=True, pixelwise=pixelwise, precision=precision)


def classify_ref(params, img, cfg):
    from oracle.model import encoder_embed, pos_table, transformer_forward
    ocfg = oracle_cfg_from(cfg)
    _, tok = encoder_embed(params, img, ocfg)
    y = transformer_forward(params, tok + pos_table(params, ocfg), ocfg)
    return pix_head_ref(y, params["encoder.mlp_head.0.weight"], params["encoder.mlp_head.0.bias"],
                        params["encoder.mlp_head.2.weight"], params["encoder.mlp_head.2.bias"], ocfg.S, ocfg.Nsq ** 2)


@pytest.mark.parametrize("name", CASES)
def test_pixelwise_step_fp32(name):
    g = load_golden(name)
    cfg = dict(g["cfg"], image_size=g["cfg"].get("image_size", 7))
    w = cfg["image_size"]
    seed_all(5)
    enc = pixelwise_encoder(cfg)
    x = torch.randn(cfg["B"], cfg["bands"], w, w)
    label = torch.randint(0, cfg["n_classes"], (cfg["B"], w, w))[:, w // 2, w // 2]
    params = {"encoder." + k: v.detach().clone().requires_grad_(True) for k, v in enc.state_dict().items()}
    ref_logits = classify_ref(params, x, cfg)
    F.cross_entropy(ref_logits, label, ignore_index=-1).backward()
    enc = enc.cuda()
    logits = enc(x.cuda())
    assert logits.shape == (cfg["B"], cfg["n_classes"])
    loss = F.cross_entropy(logits, label.cuda(), ignore_index=-1)
    loss.backward()
    torch.cuda.synchronize()
    err = relerr(logits, ref_logits)
    assert err < 1e-4, err
    assert relerr(logits, torch.from_numpy(g["logits"])) < 1e-4
    assert abs(loss.item() - float(g["loss"])) <= 1e-4 * abs(float(g["loss"]))
    bad = []
    for k, p in enc.named_parameters():
        e = relerr(p.grad, params["encoder." + k].grad)
        if not e < 3e-4:
            bad.append((k, e))
    assert not bad, bad
    gsq = sum(float((p.grad.double() ** 2).sum()) for p in enc.parameters())
    assert abs(gsq ** 0.5 - float(g["grad_l2"])) <= 1e-3 * float(g["grad_l2"])


@pytest.mark.parametrize("nc", [8, 20])
def test_pix_head_kernels_full_size_vs_float64(nc):
    """the head alone at B = 256, S = 20, N = 49: logits, dy and the four head gradients against float64 autograd; two backward
    calls bitwise equal; a 7-sample batch gives the full batch's first 7 logit rows bit for bit"""
    cfg = dict(bands=200, depth=1, n_classes=nc)
    seed_all(11)
    enc = pixelwise_encoder(cfg).cuda()
    with torch.no_grad():   # a non-trivial affine LayerNorm and bias
        enc.mlp_head[0].weight.copy_(1 + 0.5 * torch.randn(96))
        enc.mlp_head[0].bias.copy_(0.3 * torch.randn(96))
        enc.mlp_head[2].bias.copy_(torch.randn(nc))
    eng = enc.engine()
    eng.ensure()
    B, S, N = 256, 20, 49
    gen = torch.Generator(device="cuda").manual_seed(3)
    y = torch.randn(B, S * N, 96, device="cuda", generator=gen) * 2 + 0.5
    dl = torch.randn(B, nc, device="cuda", generator=gen)
    logits = eng.pix_head_fwd(y)
    names = ["mlp_head.0.weight", "mlp_head.0.bias", "mlp_head.2.weight", "mlp_head.2.bias"]
    dy = eng.pix_head_bwd(y, dl)
    grads = [eng.fp.view(n, eng.fp.grad).clone() for n in names]
    dy2 = eng.pix_head_bwd(y, dl)
    grads2 = [eng.fp.view(n, eng.fp.grad).clone() for n in names]
    logits2 = eng.pix_head_fwd(y)
    logits7 = eng.pix_head_fwd(y[:7].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(dy, dy2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))
    assert torch.equal(logits, logits2) and torch.equal(logits7, logits[:7])
    y64 = y.double().requires_grad_(True)
    p64 = [eng.fp.view(n).detach().double().requires_grad_(True) for n in names]
    ref = pix_head_ref(y64, *p64, S, N)
    ref.backward(dl.double())
    errs = dict(logits=relerr(logits, ref), dy=relerr(dy, y64.grad))
    for n, gv, p in zip(names, grads, p64):
        errs[n] = relerr(gv, p.grad)
    assert all(e < 1e-4 for e in errs.values()), errs


def test_single_sample_is_squeezed():
    """B = 1 returns [nc] (the reference's x.squeeze()), the same values as the sample's row of a larger batch"""
    cfg = dict(bands=50, depth=1, n_classes=8)
    seed_all(5)
    enc = pixelwise_encoder(cfg).cuda().eval()
    x = torch.randn(3, 50, 7, 7).cuda()
    with torch.no_grad():
        one, three = enc(x[:1]), enc(x)
    assert one.shape == (8,) and three.shape == (3, 8)
    assert relerr(one, three[0]) < 1e-5


def test_pixelwise_bf16_finetune_matches_oracle_accuracy():
    """a short bf16 finetune (Adam, a learnable synthetic centre-pixel task) reaches the accuracy of the same finetune run by the
    fp32 CPU oracle within 1 %"""
    cfg = dict(bands=50, depth=1, n_classes=4)
    seed_all(5)
    enc = pixelwise_encoder(cfg, precision="bf16")
    params = {"encoder." + k: v.detach().clone().requires_grad_(True) for k, v in enc.state_dict().items()}
    gen = torch.Generator().manual_seed(9)
    n_train, n_eval, B, steps = 512, 1024, 32, 40
    xs = torch.randn(n_train + n_eval, 50, 7, 7, generator=gen)
    # the class k raises band k of the window by 1 (a shape within the first spectral block: the tokenizer's LayerNorm over the
    # block keeps it); the fp32 oracle reaches 0.995 in these 40 steps
    ys = torch.randint(0, 4, (n_train + n_eval,), generator=gen)
    xs[torch.arange(len(ys)), ys] += 1.0
    xtr, ytr, xev, yev = xs[:n_train], ys[:n_train], xs[n_train:], ys[n_train:]
    enc = enc.cuda()
    opt = torch.optim.Adam(enc.parameters(), lr=1e-3)
    opt_ref = torch.optim.Adam(list(params.values()), lr=1e-3)
    names = [k for k, _ in enc.named_parameters()]
    assert set("encoder." + k for k in names) == set(params)
    for step in range(steps):
        i = torch.arange(step * B, (step + 1) * B) % n_train
        opt.zero_grad()
        F.cross_entropy(enc(xtr[i].cuda()), ytr[i].cuda()).backward()
        opt.step()
        opt_ref.zero_grad()
        F.cross_entropy(classify_ref(params, xtr[i], dict(cfg, image_size=7)), ytr[i]).backward()
        opt_ref.step()
    enc.eval()
    with torch.no_grad():
        pred = torch.cat([enc(xev[j:j + 256].cuda()).argmax(dim=1).cpu() for j in range(0, n_eval, 256)])
        pred_ref = classify_ref(params, xev, dict(cfg, image_size=7)).argmax(dim=1)
    acc, acc_ref = float((pred == yev).double().mean()), float((pred_ref == yev).double().mean())
    assert acc_ref > 0.5, acc_ref   # the task is learnt
    assert abs(acc - acc_ref) <= 0.01, (acc, acc_ref)


def test_predict_scene_pixelwise_matches_deephyperx_loop():
    """predict_scene of a pixelwise model against the reference's per-pixel loop (fixture: strides 1 and 2); the default stride is
    1; max_windows 1, 7 and all give bitwise-identical class maps"""
    g = load_golden("pixwise_scene_50b_L2_Bs2_20x22.npz")
    cfg = g["cfg"]
    seed_all(5)
    enc = pixelwise_encoder(cfg)
    scene = torch.randn(cfg["Bs"], cfg["bands"], cfg["Hs"], cfg["Ws"])
    s = scene.double()
    np.testing.assert_allclose([s.sum().item(), s.abs().sum().item()], g["scene_fp"], rtol=1e-12)
    enc = enc.cuda()
    sc = scene.cuda()
    w = cfg["image_size"]
    for stride in cfg["strides"]:
        ref_classes = torch.from_numpy(g[f"classes_s{stride}"].astype(np.int64))
        ref_logits = torch.from_numpy(g[f"logits_s{stride}"])
        centre = ref_classes >= 0
        maps = []
        for mw in (1, 7, None):
            classes, logits = enc.predict_scene(sc, stride=stride, return_logits=True, max_windows=mw)
            maps.append((classes.cpu(), logits.cpu()))
        # the centre assembly does not depend on the chunking; the block kernels pick their tiling by batch size, so the logits
        # of other chunk sizes may differ in the last bits (as tests/test_gpu_scene.py measures for the default head)
        for c_, l_ in maps[1:]:
            assert torch.equal(c_, maps[0][0])
            assert rel_l2(l_, maps[0][1]) < 1e-5
        classes, logits = maps[0]
        assert torch.equal(classes < 0, ~centre)
        assert (logits.permute(0, 2, 3, 1)[~centre] == 0).all()
        assert (classes[:, : w // 2] == -1).all() and (classes[:, :, -(w // 2):] == -1).all()
        top = ref_logits.topk(2, dim=1).values
        sure = centre & (top[:, 0] - top[:, 1] > 1e-3)
        assert torch.equal(classes[sure], ref_classes[sure])
        err = rel_l2(logits.permute(0, 2, 3, 1)[centre], ref_logits.permute(0, 2, 3, 1)[centre])
        assert err < 1e-4, (stride, err)
        if stride == 1:
            dense = classes
    assert torch.equal(enc.predict_scene(sc).cpu(), dense)   # stride None: 1 for a pixelwise model


def _rel_grads(enc, params):
    return {k: rel_l2(p.grad, params["encoder." + k].grad) for k, p in enc.named_parameters()}


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_default_head_7x7_matches_oracle(precision):
    """the default-head encoder at 7 x 7 (N = 49: the generic tokenizer, 49-token spatial sequences padded to 64-row tiles) against
    the oracle: the encoder output, the logits and every gradient through classify"""
    from oracle import classify_forward
    from oracle.model import encoder_embed, pos_table, transformer_forward
    cfg = dict(bands=50, depth=2, n_classes=8, image_size=7, spectral_pos_embed=False)
    seed_all(5)
    enc = pixelwise_encoder(cfg, pixelwise=False, precision=precision)
    x = torch.randn(3, 50, 7, 7)
    label = torch.randint(-1, 8, (3, 7, 7))
    params = {"encoder." + k: v.detach().clone().requires_grad_(True) for k, v in enc.state_dict().items()}
    ocfg = oracle_cfg_from(cfg)
    with torch.no_grad():
        _, tok = encoder_embed(params, x, ocfg)
        ref_feat = transformer_forward(params, tok + pos_table(params, ocfg), ocfg)
    ref_logits = classify_forward(params, x, ocfg)
    F.cross_entropy(ref_logits, label, ignore_index=-1).backward()
    enc = enc.cuda()
    with torch.no_grad():
        feat = enc.forward_features(x.cuda())
    logits = enc(x.cuda())
    assert logits.shape == (3, 8, 7, 7)
    F.cross_entropy(logits, label.cuda(), ignore_index=-1).backward()
    torch.cuda.synchronize()
    ef, el = rel_l2(feat, ref_feat), rel_l2(logits, ref_logits)
    eg = _rel_grads(enc, params)
    # fp32: the kernels' fp32 arithmetic; bf16: bf16 MFMA operands of the blocks (bars of the 8 x 8 bf16 tests' order)
    bar_f, bar_g = (1e-5, 1e-4) if precision == "fp32" else (1e-2, 5e-2)
    assert ef < bar_f and el < bar_f, (ef, el)
    worst = max(eg, key=eg.get)
    assert eg[worst] < bar_g, (worst, eg[worst])


def test_scripts_pixelwise_checkpoint_handoff(tmp_path):
    """pretrain.py --save-dir (8 x 8) -> finetune.py --pixelwise --checkpoint (7 x 7): load, training, dense scene validation"""
    import subprocess

    def run(cmd):
        e = dict(os.environ)
        e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
        r = subprocess.run(cmd, cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, f"{' '.join(cmd)}\n--- stdout\n{r.stdout[-4000:]}\n--- stderr\n{r.stderr[-4000:]}"
        return r.stdout

    save = str(tmp_path / "ck")
    run([sys.executable, "pretrain.py", "--batch-size", "8", "--tiles", "16", "--epochs", "1", "--pool-tiles", "8",
         "--precision", "fp32", "--save-dir", save])
    files = sorted(os.listdir(save))
    assert files, files
    out = run([sys.executable, "finetune.py", "enmap", "--steps", "10", "--batch-size", "4", "--precision", "bf16",
               "--pixelwise", "--checkpoint", os.path.join(save, files[-1]), "--val-scenes", "1", "--val-every", "10"])
    assert "<All keys matched successfully>" in out, out
    last = [l for l in out.splitlines() if l.startswith("step 10 ")]
    assert last and np.isfinite(float(last[0].split()[3])), out
    val = [l for l in out.splitlines() if l.startswith("val step 10 ")]
    assert val and np.isfinite(float(val[0].split()[4])), out
