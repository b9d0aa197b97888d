"""GPU: input gradients -- d(loss)/d(img) through the HIP tokenizer backward (msst_tokenize_bwd_input, msst_head_bwd_target,
msst_tokenize_scene_bwd_input in maskedsst_amd/csrc/msst_input_grad.hip), the autograd path that hands it out, and the helpers of
maskedsst_amd.saliency.  Kernels alone against float64 restatements written here; end to end against the oracle's img.grad
(tests/input_grad_util.py: pinned to the reference's by tests/test_input_grad_host.py)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from util import relerr, rel_l2, record
from input_grad_util import (CASES, SIMMIM, CLASSIFIER, QUIRK, fixture, build_model, class_label, oracle_run, target_term_ref,
                             with_duplicates)
from tok_head_util import tok_params, tok_ref

pytestmark = pytest.mark.gpu
BADARG, UNSUPPORTED = -3, -2
# bf16 end to end, measured on the MI355X (profiles/input_grad_parity_measured.jsonl); each bar is 3.5 x its measured value, the
# project's convention.  The sanity condition of the kernel chain: rel_l2 of the order of BF16_DX0 = 6e-3 (tests/test_gpu_backward.py),
# img.grad being one more fp32 stage after dx0.
BF16_BARS = {
    "cls_50b_L2_B2_specpos/rel_l2": 6.8e-3,             # measured 1.934e-3
    "pixwise_30b_L1_B3_img5_h2/rel_l2": 4.5e-3,         # measured 1.281e-3
    "spechead_30b_L1_B2_img6_h2/rel_l2": 3.9e-3,        # measured 1.102e-3
    # SimMIM: img.grad is dominated by the loss's target term, +-1 / (B K P) / K per masked pixel, which bf16 only touches through the
    # sign flips; the token path under it is two orders smaller -- hence figures far below BF16_DX0
    "simmim_50b_L2_tube/one_minus_cos": 8.0e-8,         # measured 2.294e-8
    "simmim_50b_L2_tube/rel_l2": 7.5e-4,                # measured 2.142e-4 (the oracle's sign pattern fed to the backward)
    "simmim_50b_L2_B4_mps1/one_minus_cos": 1.7e-7,      # measured 4.928e-8
    "simmim_50b_L2_B4_mps1/rel_l2": 1.1e-3,             # measured 3.139e-4
}


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _measure(key, **kv):
    """one measured row, handed to tests.util.record (MSST_RECORD=1 appends it to the scratch parity file, the source of the
    committed profiles/input_grad_parity_measured.jsonl)"""
    record("input_grad_" + key, **kv)


# ---------------------------------------------------------------------------------------------- the kernel alone
def dev(q):
    return {k: v.float().cuda().contiguous() for k, v in q.items()}


def run_input_bwd(lib, d, img, dx0, B, S, N, P, mask=None, dtarget=None, drop=(0.0, 0)):
    dimg = torch.full_like(img, float("nan"))
    rc = lib.msst_tokenize_bwd_input(_p(img), _p(d["pre_g"]), _p(d["pre_b"]), _p(d["w"]), _p(d["b"]), _p(d["post_g"]), _p(d["post_b"]),
                                     _p(mask), _p(dx0), _p(dtarget), _p(dimg), B, S, N, P, drop[0], drop[1], _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return dimg


@pytest.mark.parametrize("N", [1, 25, 49, 64])
@pytest.mark.parametrize("P", [1, 5, 10, 16])
def test_tokenize_bwd_input_vs_float64(P, N):
    """rel_l2 <= 2e-5 against the float64 autograd of the restatement: fp32 arithmetic over 96- and P-term sums.  Mask none / random /
    all, with and without dtarget; all-masked without dtarget is exactly 0; two runs give equal bits."""
    from maskedsst_amd import _lib
    lib = _lib.load()
    gen = torch.Generator().manual_seed(100 * P + N)
    worst = 0.0
    for B in (1, 3):
        for S in (1, 5, 20):
            q = tok_params(S, P, gen)
            img = (torch.randn(B, S * P, N, generator=gen, dtype=torch.float64) * 1.5 + 0.3).requires_grad_(True)
            dx0 = torch.randn(B, S * N, 96, generator=gen, dtype=torch.float64)
            dtg = torch.randn(B, S * P, N, generator=gen, dtype=torch.float64)
            out = tok_ref(img, q, S, N, P)
            d = dev(q)
            img_d, dx0_d, dtg_d = img.detach().float().cuda(), dx0.float().cuda(), dtg.float().cuda()
            masks = {"none": None, "random": torch.rand(B, S * N, generator=gen) < 0.5, "all": torch.ones(B, S * N, dtype=torch.bool)}
            for mname, m in masks.items():
                keep = torch.ones(B, S * N, 1, dtype=torch.float64) if m is None else (~m).double().unsqueeze(-1)
                (want,) = torch.autograd.grad(out, img, dx0 * keep, retain_graph=True)
                m_d = None if m is None else m.to(torch.uint8).cuda()
                for with_t in (False, True):
                    got = run_input_bwd(lib, d, img_d, dx0_d, B, S, N, P, m_d, dtg_d if with_t else None)
                    again = run_input_bwd(lib, d, img_d, dx0_d, B, S, N, P, m_d, dtg_d if with_t else None)
                    assert torch.equal(got, again), (B, S, mname, with_t)
                    ref = want + dtg if with_t else want
                    if mname == "all" and not with_t:
                        assert float(got.abs().max()) == 0.0, (B, S)
                        continue
                    if P == 1 and not with_t:   # a one-pixel LayerNorm has no gradient: 0, which float64 autograd meets up to its rounding
                        assert float(got.abs().max()) == 0.0 and float(ref.abs().max()) <= 1e-9, (B, S, mname)
                        continue
                    err = rel_l2(got, ref)
                    worst = max(worst, err)
                    assert err <= 2e-5, (B, S, mname, with_t, err)
    record("input_grad_kernel", P=P, N=N, err=worst)


def test_dropout_regeneration():
    """emb_dropout_p = 0.3: the backward zeroes and scales dx0 exactly where msst_tokenize_fwd, run with the same (p, seed), dropped:
    the keep mask is read back from that forward (zero position table, nothing masked: a dropped element is an exact 0)"""
    from maskedsst_amd import _lib
    lib = _lib.load()
    B, S, N, P, p, seed = 3, 5, 64, 10, 0.3, 4711
    gen = torch.Generator().manual_seed(7)
    q = tok_params(S, P, gen)
    d = dev(q)
    img = (torch.randn(B, S * P, N, generator=gen, dtype=torch.float64) * 1.5).requires_grad_(True)
    dx0 = torch.randn(B, S * N, 96, generator=gen, dtype=torch.float64)
    img_d, dx0_d = img.detach().float().cuda(), dx0.float().cuda()
    zero_pos = torch.zeros(S * N, 96, device="cuda")
    zero_mask = torch.zeros(B, S * N, dtype=torch.uint8, device="cuda")
    tok = torch.empty(B, S * N, 96, device="cuda")
    rc = lib.msst_tokenize_fwd(_p(img_d), _p(d["pre_g"]), _p(d["pre_b"]), _p(d["w"]), _p(d["b"]), _p(d["post_g"]), _p(d["post_b"]),
                               _p(zero_pos), None, 0, _p(d["post_b"]), _p(zero_mask), _p(tok), B, S, N, P, p, seed, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    keep = (tok != 0).double().cpu()
    rate = 1.0 - float(keep.mean())
    assert abs(rate - p) < 0.01, rate
    thr = int(p * 65536.0 + 0.5)
    scale = 1.0 / (1.0 - thr / 65536.0)   # msst_api.hip make_drop: the exact inverse of the realised keep probability
    (want,) = torch.autograd.grad(tok_ref(img, q, S, N, P), img, dx0 * keep * scale)
    got = run_input_bwd(lib, d, img_d, dx0_d, B, S, N, P, None, None, drop=(p, seed))
    err = rel_l2(got, want)
    assert err <= 2e-5, err
    other = run_input_bwd(lib, d, img_d, dx0_d, B, S, N, P, None, None, drop=(p, seed + 1))
    assert rel_l2(other, want) > 0.1   # another seed: other masks


@pytest.mark.parametrize("variant", ["fixture", "duplicates"])
def test_head_bwd_target_gathers_with_a_sum(variant):
    from maskedsst_amd import _lib
    from maskedsst_amd.masking import inverse_csr
    lib = _lib.load()
    fx = fixture(QUIRK)
    S, N, P = fx["cfg"]["bands"] // 10, 64, 10
    idx = fx["idx"] if variant == "fixture" else with_duplicates(fx["idx"], S * N)
    B, K = idx.shape
    gen = torch.Generator().manual_seed(9)
    dpred = torch.sign(torch.randn(B, K, P, generator=gen))
    ptr, pos = inverse_csr(idx.numpy(), S * N)
    gout = torch.tensor([0.37], device="cuda")
    dpred_d, ptr_d, pos_d = dpred.cuda(), torch.from_numpy(ptr).cuda(), torch.from_numpy(pos).cuda()
    for g in (None, gout):
        out = torch.full((B, S * P, N), float("nan"), device="cuda")
        rc = lib.msst_head_bwd_target(_p(dpred_d), _p(ptr_d), _p(pos_d), _p(g), _p(out), B, S, N, P, K, _stream())
        assert rc == 0
        torch.cuda.synchronize()
        want = target_term_ref(dpred, idx, S, N, P, 1.0 if g is None else 0.37)
        assert float((out.double().cpu() - want).abs().max()) <= 1e-6 * float(want.abs().max())
    if variant == "duplicates":   # the token named three times really carries a sum
        t = int(idx[0, 0])
        assert float(want.reshape(B, S, P, N)[0, t // N, :, t % N].abs().max()) > 0


def test_scene_variant_matches_stacked_windows():
    from maskedsst_amd import _lib
    lib = _lib.load()
    Bs, C, Hs, Ws, win, S, P = 2, 50, 19, 17, 8, 5, 10
    N = win * win
    gen = torch.Generator().manual_seed(21)
    d = dev(tok_params(S, P, gen))
    tiles = torch.randn(Bs, C, Hs, Ws, generator=gen).cuda()
    nr, nq = Hs // win, Ws // win
    total = Bs * nr * nq
    dx0 = torch.randn(total, S * N, 96, generator=gen).cuda()
    args = lambda t, o, stride, win0, nwin: lib.msst_tokenize_scene_bwd_input(   # noqa: E731
        _p(t), _p(d["pre_g"]), _p(d["pre_b"]), _p(d["w"]), _p(d["b"]), _p(d["post_g"]), _p(d["post_b"]), _p(dx0[win0:]), _p(o), Bs, Hs, Ws,
        win, stride, win0, nwin, S, P, 0.0, 0, _stream())
    dscene = torch.full_like(tiles, float("nan"))
    assert args(tiles, dscene, 4, 0, total) == UNSUPPORTED
    assert args(tiles, dscene, 8, 0, total + 1) == BADARG and args(None, dscene, 8, 0, total) == BADARG
    torch.cuda.synchronize()
    assert bool(torch.isnan(dscene).all()), "a refused call wrote"
    # two calls of one batch: the first zeroes the border
    assert args(tiles, dscene, 8, 0, 3) == 0 and args(tiles, dscene, 8, 3, total - 3) == 0
    torch.cuda.synchronize()
    stacked = tiles[:, :, :nr * win, :nq * win].reshape(Bs, C, nr, win, nq, win).permute(0, 2, 4, 1, 3, 5).reshape(total, C, N).contiguous()
    dwin = run_input_bwd(lib, d, stacked, dx0, total, S, N, P)
    want = torch.zeros_like(tiles)
    want[:, :, :nr * win, :nq * win] = dwin.reshape(Bs, nr, nq, C, win, win).permute(0, 3, 1, 4, 2, 5).reshape(Bs, C, nr * win, nq * win)
    assert torch.equal(dscene, want)
    assert float(dscene[:, :, nr * win:].abs().max()) == 0.0 and float(dscene[:, :, :, nq * win:].abs().max()) == 0.0
    assert float(dscene[:, :, :nr * win, :nq * win].abs().min()) > 0.0


# ---------------------------------------------------------------------------------------------- end to end
def product_step(name, precision, want_input):
    """one backward of the product on the fixture's input -> (img.grad or None, {parameter name: grad}, loss)"""
    fx = fixture(name)
    model, _, x = build_model(name, precision)
    model = model.cuda().eval()
    x = x.cuda().requires_grad_(want_input)
    if name in SIMMIM:
        loss = model(x, masks=(fx["bool_mask"], fx["idx"]))
    else:
        loss = F.cross_entropy(model(x), class_label(fx).cuda(), ignore_index=-1)
    loss.backward()
    torch.cuda.synchronize()
    return x.grad, {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}, float(loss), model


@pytest.mark.parametrize("name", CASES)
def test_img_grad_fp32_matches_oracle(name):
    """relerr <= 2e-4, the bar of test_param_grads_fp32; and the parameter gradients of the same run are bit-identical to those of a
    run in which the input does not require a gradient (the new launches only read)"""
    ref = oracle_run(name)
    g, pg, loss, _ = product_step(name, "fp32", True)
    assert g is not None and g.shape == fixture(name)["x"].shape
    err = relerr(g, ref["img_grad"])
    assert abs(loss - ref["loss"]) <= 1e-4 * abs(ref["loss"])
    _, pg0, _, _ = product_step(name, "fp32", False)
    assert pg.keys() == pg0.keys() and len(pg) > 0
    assert all(torch.equal(pg[k], pg0[k]) for k in pg), [k for k in pg if not torch.equal(pg[k], pg0[k])]
    record("input_grad_fp32", case=name, err=err)
    assert err <= 2e-4, err


@pytest.mark.parametrize("name", CLASSIFIER)
def test_img_grad_bf16_classifier(name):
    ref = oracle_run(name)
    g, pg, _, _ = product_step(name, "bf16", True)
    _, pg0, _, _ = product_step(name, "bf16", False)
    assert all(torch.equal(pg[k], pg0[k]) for k in pg)
    err = rel_l2(g, ref["img_grad"])
    print(f"input_grad bf16 {name}: rel_l2 {err:.4e}")
    _measure("bf16_classifier", case=name, rel_l2=err)
    assert err <= BF16_BARS[name + "/rel_l2"], err


@pytest.mark.parametrize("name", SIMMIM)
def test_img_grad_bf16_simmim(name):
    """as test_param_grads_bf16: bf16 rounding flips the sign of the L1 entries with pred ~= target, so (1) end to end the cosine of
    the whole img.grad, (2) with the oracle's sign pattern fed to the backward kernels, rel_l2"""
    from maskedsst_amd.masking import inverse_csr
    ref, fx = oracle_run(name), fixture(name)
    g, _, _, model = product_step(name, "bf16", True)
    a, b = g.double().cpu().reshape(-1), ref["img_grad"].double().reshape(-1)
    one_minus_cos = 1.0 - float((a * b).sum() / (a.norm() * b.norm()))
    eng = model.engine()
    x = fx["x"].cuda()
    out = eng.simmim_forward_stages(x, fx["bool_mask"], fx["idx"])
    sgn = ref["sign"].cuda().contiguous()
    ptr, pos = inverse_csr(fx["idx"].numpy(), eng.S * eng.N)
    ptr, pos = torch.from_numpy(ptr).cuda(), torch.from_numpy(pos).cuda()
    dy = eng.head_bwd(out["enc_out"], sgn, ptr, pos)
    dx0 = eng.blocks_bwd(out["acts"], out["x1s"], dy)
    dimg = eng.tokenize_input_bwd(x, fx["bool_mask"].to(torch.uint8).cuda(), dx0, eng.head_bwd_target(sgn, ptr, pos))
    torch.cuda.synchronize()
    err = rel_l2(dimg, ref["img_grad"])
    print(f"input_grad bf16 {name}: 1 - cos {one_minus_cos:.4e}, rel_l2 with the oracle's signs {err:.4e}")
    _measure("bf16_simmim", case=name, one_minus_cos=one_minus_cos, rel_l2=err)
    assert one_minus_cos <= BF16_BARS[name + "/one_minus_cos"], one_minus_cos
    assert err <= BF16_BARS[name + "/rel_l2"], err


# ---------------------------------------------------------------------------------------------- what fails without the feature
def _frozen(model):
    for p in model.parameters():
        p.requires_grad_(False)
    return model.cuda().eval()


def _check_saliency(x, params):
    assert x.grad is not None and x.grad.shape == x.shape
    assert bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0
    assert all(p.grad is None for p in params)


def test_frozen_eval_model_gives_img_grad():
    """the ordinary saliency set-up: eval, every parameter frozen, img.requires_grad_()"""
    model, _, x = build_model("cls_50b_L2_B2_specpos")
    model = _frozen(model)
    params = list(model.parameters())
    x = x.cuda().requires_grad_(True)
    model(x)[:, 3].sum().backward()
    _check_saliency(x, params)
    tiles = torch.randn(2, 50, 19, 17, generator=torch.Generator().manual_seed(3)).cuda().requires_grad_(True)
    model.forward_windows(tiles).square().mean().backward()
    _check_saliency(tiles, params)
    assert float(tiles.grad[:, :, 16:].abs().max()) == 0.0 and float(tiles.grad[:, :, :, 16:].abs().max()) == 0.0
    x2 = x.detach().clone().requires_grad_(True)
    model.forward_features(x2).square().mean().backward()
    _check_saliency(x2, params)
    mim, _, xs = build_model(QUIRK)
    mim = _frozen(mim)
    xs = xs.cuda().requires_grad_(True)
    fx = fixture(QUIRK)
    mim(xs, masks=(fx["bool_mask"], fx["idx"])).backward()
    _check_saliency(xs, list(mim.parameters()))


def test_training_step_fills_img_grad():
    model, _, x = build_model("cls_50b_L2_B2_specpos")
    model = model.cuda().train()
    x = x.cuda().requires_grad_(True)
    F.cross_entropy(model(x), class_label(fixture("cls_50b_L2_B2_specpos")).cuda(), ignore_index=-1).backward()
    assert x.grad is not None and float(x.grad.abs().max()) > 0
    assert all(p.grad is not None for n, p in model.named_parameters())
    # linear evaluation with an input that requires a gradient: the full path
    for n, p in model.named_parameters():
        p.requires_grad_("mlp_head" in n)
        p.grad = None
    x2 = x.detach().clone().requires_grad_(True)
    model(x2).square().mean().backward()
    assert x2.grad is not None and float(x2.grad.abs().max()) > 0
    assert all((p.grad is not None) == ("mlp_head" in n) for n, p in model.named_parameters())


# ---------------------------------------------------------------------------------------------- helpers
def test_input_gradient_equals_manual_autograd():
    from maskedsst_amd import input_gradient, band_importance
    model, _, x = build_model("cls_50b_L2_B2_specpos")
    model = model.cuda().eval()
    x = x.cuda()
    xm = x.clone().requires_grad_(True)
    model(xm)[:, 3].sum().backward()
    for p in model.parameters():
        p.grad = None
    got = input_gradient(model, x, 3)
    assert torch.equal(got, xm.grad)
    assert all(p.requires_grad and p.grad is None for p in model.parameters()) and not model.training
    bi = band_importance(model, x, 3)
    assert bi.shape == (2, 50) and torch.equal(bi, (xm.grad * x).sum(dim=(2, 3)))


def test_integrated_gradients_completeness():
    """depth-1 classifier, 16 midpoint steps: the gap is below 5 % of |score(img) - score(baseline)| (O(1 / steps^2) for a smooth model).
    Input: the pixelwise fixture's, class 2, against a seeded random cube as baseline: the oracle's scores differ by 0.94, 0.17 and 0.59
    and its own gap is below 0.1 % of them (checked on the CPU).  Not the zero cube: the tokenizer's pre-norm LayerNorm makes the model
    invariant to the scale of a patch, so the score is constant along a ray from 0 and jumps at its origin -- no smooth path."""
    from maskedsst_amd import integrated_gradients
    name = "pixwise_30b_L1_B3_img5_h2"
    model, _, x = build_model(name)
    model = model.cuda().eval()
    x = x.cuda()
    base = torch.randn(x.shape, generator=torch.Generator().manual_seed(11)).cuda()
    with torch.no_grad():
        ends = (model(x)[:, 2] - model(base)[:, 2]).abs()
    attr, gap = integrated_gradients(model, x, 2, baseline=base, steps=16)
    assert attr.shape == x.shape
    frac = (gap / ends).cpu()
    record("input_grad_ig", case=name, gap=float(gap.max()), frac=float(frac.max()), ends=float(ends.min()))
    print(f"integrated gradients: gap {gap.tolist()} of {ends.tolist()}")
    assert float(ends.min()) > 0.1
    assert float(frac.max()) < 0.05, frac
