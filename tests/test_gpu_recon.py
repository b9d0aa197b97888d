"""GPU: SimMIM reconstruction -- msst_recon_fwd (to_pixels over every token into the cube layout, per-band masked |pred - img| sums)
against float64 restatements, SimMIMSpatialSpectral.reconstruct against the CPU oracle on the committed fixtures' configurations,
its band errors against the model's own loss, its independence of the module's mode, and tools/recon_time.py."""
import json
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT, load_golden
from util import build_product, oracle_cfg, relerr, record

pytestmark = pytest.mark.gpu

U = 2.0 ** -24   # unit roundoff of fp32


# ---------------------------------------------------------------------------------------------------------------- 1. op level
SHAPES = [(1, 1, 1, 1), (2, 2, 64, 10), (3, 5, 36, 5), (2, 4, 36, 16), (2, 7, 16, 10), (1, 64, 4, 3)]   # (B, S, N, P)
_op_inputs = {}


def op_inputs(shape, per_block):
    """seeded y, img, mask and to_pixels tables of one shape with their float64 restatement, computed once and shared (read-only)
    by the blend cases: pred [B, S P, N], the elementwise bound, and the masked error sums / counts per band"""
    key = (shape, per_block)
    if key not in _op_inputs:
        B, S, N, P = shape
        g = torch.Generator().manual_seed(1000 * B + 100 * S + N + P)
        y = torch.randn(B, S * N, 96, generator=g)
        img = torch.randn(B, S * P, N, generator=g)
        nw = S if per_block else 1
        w, bias = torch.randn(nw, P, 96, generator=g) * 0.2, torch.randn(nw, P, generator=g)
        mask = torch.rand(B, S * N, generator=g) < 0.6
        mask[0, :N] = False          # an all-zero row: block 0 of sample 0 has nothing masked
        mask[-1, -N:] = True         # an all-one row: the last block of the last sample is masked whole
        if B > 1 and S > 1:
            mask[0, N:2 * N] = True
            mask[-1, :N] = False
        wd, bd = w.double().expand(S, P, 96), bias.double().expand(S, P)
        yd = y.double().view(B, S, N, 96)
        pred = (torch.einsum("bsnd,spd->bspn", yd, wd) + bd[None, :, :, None]).reshape(B, S * P, N)
        # a 97-term fp32 sum (bias + 96 products, any order, fused or not): |got - ref| <= gamma_97 sum |terms| <= 2 * 97 u sum |terms|
        bound = 2 * 97 * U * (torch.einsum("bsnd,spd->bspn", yd.abs(), wd.abs()) + bd.abs()[None, :, :, None]).reshape(B, S * P, N)
        m = mask.view(B, S, 1, N).expand(B, S, P, N).reshape(B, S * P, N)
        err = ((pred - img.double()).abs() * m).sum(-1)
        _op_inputs[key] = dict(y=y, img=img, w=w, b=bias, mask=mask, pred=pred, bound=bound, m=m, err=err,
                               err_bound=(bound * m).sum(-1), cnt=m.sum(-1).to(torch.int32))
    return _op_inputs[key]


@pytest.mark.parametrize("blend", [0, 1])
@pytest.mark.parametrize("per_block", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-S%d-N%d-P%d" % s)
def test_recon_fwd_against_float64(shape, per_block, blend):
    """the kernel alone on random inputs.  Bounds derived, not measured: an element of recon is a 97-term fp32 sum, so it lies within
    2 * 97 * 2^-24 * (|b| + sum_d |W| |y|) of the float64 value; a band's error sum adds |pred - img| of its masked pixels -- the
    difference is formed exactly (in double) and summed in double, so it lies within the SUM of those pixels' bounds (at most the
    count times the largest); the counts are integers: exact."""
    from maskedsst_amd.engine import recon_fwd
    B, S, N, P = shape
    d = op_inputs(shape, per_block)
    dev = "cuda"
    y, img, w, b = (d[k].to(dev) for k in ("y", "img", "w", "b"))
    mask_u8 = d["mask"].to(device=dev, dtype=torch.uint8)
    recon, err, cnt = recon_fwd(y, img, mask_u8, w, b, per_block, blend, S, N, P)
    recon2, none_e, none_c = recon_fwd(y, img, mask_u8, w, b, per_block, blend, S, N, P, stats=False)
    torch.cuda.synchronize()
    assert recon.shape == (B, S * P, N) and err.shape == cnt.shape == (B, S * P) and err.dtype == torch.float64 and cnt.dtype == torch.int32
    assert none_e is None and none_c is None and torch.equal(recon, recon2)   # null statistics pointers: the same bits
    recon, err, cnt = recon.cpu(), err.cpu(), cnt.cpu()
    m = d["m"]
    where = m if blend else torch.ones_like(m)          # the elements that hold predictions
    excess = ((recon.double() - d["pred"]).abs() - d["bound"])[where]
    worst = float(((recon.double() - d["pred"]).abs() / d["bound"])[where].max()) if where.any() else 0.0
    print(f"recon_fwd {shape} per_block={per_block} blend={blend}: worst |got - ref| / bound = {worst:.3e}")
    assert not (excess > 0).any(), float(excess.max())
    if blend:
        assert torch.equal(recon.view(torch.int32)[~m], d["img"].view(torch.int32)[~m])   # unmasked pixels: img bit for bit
    assert torch.equal(cnt, d["cnt"])
    eex = (err - d["err"]).abs() - d["err_bound"]
    assert not (eex > 0).any(), float(eex.max())
    assert (err[d["cnt"] == 0] == 0).all()
    worst_band = float(((err - d["err"]).abs() / d["err_bound"].clamp(min=1e-300)).max())
    record("recon_fwd_op", shape=list(shape), per_block=per_block, blend=blend, err_over_bound=worst, band_err_over_bound=worst_band)


# ------------------------------------------------------------------------------------------------- 2. end to end against the oracle
GOLDENS = ["simmim_tiny_20b_L1_B2_h2", "simmim_30b_L1_B2_img6_mps2_h2", "simmim_50b_L2_B4_sharedpix", "simmim_50b_L2_B4_nontube",
           "patch_P5_50b_L1_B2", "patch_P16_64b_L1_B3_img6_mps2_h2"]
_oracle = {}


def oracle_case(name):
    """(cfg, masks, float64 to_pixels of the oracle's enc_out over EVERY token in the cube layout, the oracle's pred): once per
    fixture, shared by both precisions.  The model and the masks come from the same seed every time (build_product seeds)."""
    if name not in _oracle:
        from oracle import simmim_forward
        cfg = load_golden(name + ".npz")["cfg"]
        model, params, x = build_product(cfg)
        masks = model.draw_masks(cfg["B"])
        ocfg = oracle_cfg(cfg)
        with torch.no_grad():
            ref = simmim_forward(params, x, ocfg, masks=masks)
        B, S, N, P = cfg["B"], ocfg.S, ocfg.N, cfg.get("spectral_patch", 10)
        if cfg.get("to_pixels_per_spectral_block", True):
            W = torch.stack([params[f"to_pixels.layers.{i}.weight"] for i in range(S)]).double()
            bias = torch.stack([params[f"to_pixels.layers.{i}.bias"] for i in range(S)]).double()
        else:
            W, bias = params["to_pixels.weight"].double().expand(S, P, 96), params["to_pixels.bias"].double().expand(S, P)
        e = ref["enc_out"].double().view(B, S, N, 96)
        full = (torch.einsum("bsnd,spd->bspn", e, W) + bias[None, :, :, None]).reshape(B, S * P, N)
        _oracle[name] = (cfg, masks, full, ref["pred"].double(), (S, N, P))
    return _oracle[name]


# the bars tests/test_gpu_forward.py::test_forward_stages applies to `pred` (max-norm relative, util.relerr) at each precision
@pytest.mark.parametrize("prec,tol", [("fp32", 1e-4), ("bf16", 9e-3)])
@pytest.mark.parametrize("name", GOLDENS)
def test_reconstruct_against_the_oracle(name, prec, tol):
    cfg, masks, full, ref_pred, (S, N, P) = oracle_case(name)
    model, _, x = build_product(cfg, precision=prec, device="cuda")
    B = cfg["B"]
    s = cfg.get("image_size", 8)
    rec = model.reconstruct(x.cuda(), masks, blend=False)
    recb = model.reconstruct(x.cuda(), masks[0])      # the bare bool mask, blended (the default)
    torch.cuda.synchronize()
    assert rec.cube.shape == rec.mask.shape == (B, S * P, s, s) and rec.cube.dtype == torch.float32 and rec.mask.dtype == torch.bool
    assert rec.band_err.shape == rec.band_cnt.shape == (B, S * P)
    assert rec.band_err.dtype == torch.float64 and rec.band_cnt.dtype == torch.int32
    cube = rec.cube.cpu().view(B, S * P, N)
    err_full = relerr(cube, full)
    # on the masked gather list the cube is the oracle's pred [B, K, P]: token t = c N + n -> bands c P .. c P + P - 1 at position n
    idx = masks[1].long()
    c, n = idx // N, idx % N
    band = c[..., None] * P + torch.arange(P)                                    # [B, K, P]
    got = cube[torch.arange(B)[:, None, None], band, n[..., None].expand_as(band)]
    err_pred = relerr(got, ref_pred)
    print(f"reconstruct {name} {prec}: relerr over all tokens {err_full:.3e}, on the gather list {err_pred:.3e}")
    assert err_full < tol, err_full
    assert err_pred < tol, err_pred
    # the mask is the token mask over the P bands of each token; blending changes only what is not masked, the tables not at all
    m = masks[0].view(B, S, 1, N).expand(B, S, P, N).reshape(B, S * P, s, s)
    assert torch.equal(rec.mask.cpu(), m) and torch.equal(recb.mask.cpu(), m)
    assert torch.equal(recb.cube.cpu()[m], rec.cube.cpu()[m])
    assert torch.equal(recb.cube.cpu().view(torch.int32)[~m], x.view(torch.int32)[~m])
    assert torch.equal(recb.band_err, rec.band_err) and torch.equal(recb.band_cnt, rec.band_cnt)
    assert torch.equal(rec.band_cnt.cpu(), m.view(B, S * P, N).sum(-1).to(torch.int32))
    record("reconstruct_oracle", name=name, prec=prec, err=err_full, err_pred=err_pred)


# ------------------------------------------------------------------------------------------------------------ 3. loss cross-check
def test_band_errors_sum_to_the_loss():
    """top-k masks (mask_patch_size 1): every row has exactly K trues and the index list IS the mask, so the loss of forward --
    mean |pred - target| over n = B K P values, / K -- is band_err.sum() / (B K P) / K.  Both run the same encoder kernels in eval
    mode (bit-identical y).  They differ in how the n non-negative terms are rounded and added: forward rounds each difference to
    fp32 and adds in fp32 (partials of <= 64 P terms, then double), reconstruct forms and adds them in double.  The fp32 summation
    bound of n non-negative terms, (n + 1) u relative (one rounding per term, at most n - 1 per chain of additions), covers any
    such order, and the loss is rounded to fp32 once more (+ u).  The two kernels also round a prediction's 97-term sum in
    different orders: each term moves by at most 2 * 97 u (|b| + sum |W| |y|), 97 / n of the bound per unit of
    (|b| + sum |W| |y|) / mean |pred - target| -- a few per cent of it at n = 8960."""
    cfg = load_golden("simmim_50b_L2_B4_mps1.npz")["cfg"]
    assert cfg.get("mask_patch_size") == 1
    model, _, x = build_product(cfg, precision="fp32", device="cuda")
    model.eval()
    B = cfg["B"]
    masks = model.draw_masks(B)
    K, P = masks[1].shape[1], model.pixel_values_per_patch
    assert (masks[0].sum(1) == K).all()
    assert torch.equal(torch.sort(masks[1], dim=1).values, torch.nonzero(masks[0])[:, 1].view(B, K))
    with torch.no_grad():
        loss = float(model(x.cuda(), masks=masks))
    rec = model.reconstruct(x.cuda(), masks)
    assert int(rec.band_cnt.sum()) == B * K * P
    n = B * K * P
    got = float(rec.band_err.sum()) / n / K
    rel = abs(got - loss) / abs(loss)
    print(f"band_err.sum() / (B K P) / K = {got:.9e}, forward = {loss:.9e}, relative difference {rel:.3e}, bound {(n + 2) * U:.3e}")
    assert rel <= (n + 2) * U, (got, loss, rel)
    record("reconstruct_loss_crosscheck", cfg=cfg, loss_err=rel)


# -------------------------------------------------------------------------------------------------------- 4. mode and determinism
def test_reconstruct_ignores_the_mode_and_is_deterministic():
    cfg = dict(bands=50, depth=2, B=4)
    model, _, x = build_product(cfg, precision="bf16", device="cuda")
    model.encoder.dropout_p = model.encoder.emb_dropout_p = 0.1   # build_product builds without dropout: switch both sites on
    masks = model.draw_masks(4)
    xg = x.cuda()
    model.train()
    a = model.reconstruct(xg, masks)
    assert model.training and model.encoder.training
    model.eval()
    b = model.reconstruct(xg, masks)
    c = model.reconstruct(xg, masks)
    assert not model.training and not model.encoder.training
    torch.cuda.synchronize()
    for other in (b, c):
        for p, q in zip(a, other):
            assert torch.equal(p, q)
    assert all(p.grad is None for p in model.parameters())
    assert not any(t.requires_grad for t in a)
    # ... and training mode does apply dropout to forward itself, so the equality above is not vacuous
    model.train()
    with torch.no_grad():
        l1, l2 = float(model(xg, masks=masks)), float(model(xg, masks=masks))
    assert l1 != l2


# -------------------------------------------------------------------------------------------------------------------- 5. script
def test_recon_time_script():
    """tools/recon_time.py in a fresh child process, at a small shape: exit 0, ONE JSON line with both methods' times"""
    e = dict(os.environ)
    e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, os.path.join("tools", "recon_time.py"), "--steps", "2", "--warmup", "1", "--batch", "4",
                        "--bands", "50", "--depth", "1"], cwd=ROOT, env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"--- stdout\n{r.stdout[-3000:]}\n--- stderr\n{r.stderr[-3000:]}"
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    row = json.loads(lines[0])
    assert row["tool"] == "recon_time" and row["batch"] == 4 and row["bands"] == 50 and row["steps"] == 2
    for k in ("reconstruct_ms", "eager_ms", "recon_kernel_ms", "eager_tail_ms"):
        assert row[k] > 0, (k, row)
    assert row["band_cnt_equal"] and row["max_abs_cube_diff"] < 1e-4 and row["max_rel_band_err_diff"] < 1e-4
