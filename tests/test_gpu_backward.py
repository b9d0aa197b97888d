"""GPU parity, backward: every parameter gradient of the HIP path vs autograd over the CPU oracle."""
import numpy as np
import pytest
import torch

from conftest import oracle_cfg_from
from util import build_product, relerr, record, ln1_rows_as_used, lse_restatement, saved_lse_rows

pytestmark = pytest.mark.gpu

CASES = [
    dict(bands=20, depth=1, B=2, heads=2),
    dict(bands=30, depth=1, B=3, heads=2, tube_masking=False),
    dict(bands=20, depth=1, B=2, heads=3),   # head counts other than 8: the 4-wave forward and the template attention backward
    dict(bands=20, depth=1, B=3, heads=4),   # (the tuned backward kernels at these head counts: test_attn_bwd_tuned_kernels_other_head_counts)
    dict(bands=10, depth=1, B=2, heads=2),   # one spectral token: 64 one-row sequences per spectral tile (the run-time key-tile form of the softmax phase)
    dict(bands=50, depth=2, B=4),
    dict(bands=50, depth=2, B=4, spectral_pos_embed=True),
    dict(bands=50, depth=2, B=4, to_pixels_per_spectral_block=False, mask_patch_size=1),
    dict(bands=200, depth=2, B=5),
]


# round 6: peaky attention rows (to_qkv.weight x4: logit std ~5, row maxima 0.5-0.8) through the kernels the 8-head fixtures do not
# reach -- the 4-wave forward, the one-head (odd head count) and two-head (2 / 4 heads) attention backward, the fp32 templates
PEAKY_SMALL = [
    dict(bands=20, depth=1, B=3, heads=4, qkv_scale=4),
    dict(bands=30, depth=1, B=3, heads=2, tube_masking=False, qkv_scale=4),
    dict(bands=20, depth=1, B=2, heads=3, qkv_scale=4),
    dict(bands=50, depth=2, B=4, qkv_scale=4),
]


def grads_pair(cfg, prec):
    from oracle import simmim_forward
    model, params, x = build_product(cfg, precision=prec, device="cuda")
    ocfg = oracle_cfg_from(cfg)
    masks = model.draw_masks(cfg["B"])
    for p in params.values():
        p.requires_grad_(True)
    ref = simmim_forward(params, x, ocfg, masks=masks)
    for k in ("enc_out", "tok_masked", "after_spatial"):
        ref[k].retain_grad()
    ref["loss"].backward()
    loss = model(x.cuda(), masks=masks)
    loss.backward()
    torch.cuda.synchronize()
    ref["x"] = x
    return model, params, ref, loss


# bf16 bars 3-4x measured on MI355X (profiles/r0N_parity_measured.jsonl), worst of the six cases:
# dx0 1.65e-3 rel-L2, worst parameter-gradient tensor 6.1e-3 rel-L2 (the tokenizer's pre-norm weight: a 10-element
# tensor at the end of the whole backward chain), loss 0.7e-4, 1 - cosine 1.2e-4 (B = 2: a handful of flipped L1 signs)
BF16_DX0 = 6e-3
BF16_GRAD = 2.1e-2
BF16_LOSS = 2.5e-4
BF16_COS = 0.99958


def rel_l2(a, b):
    a = a.detach().double().cpu().reshape(-1)
    b = b.detach().double().cpu().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.mark.parametrize("cfg", CASES + PEAKY_SMALL, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_param_grads_fp32(cfg):
    """fp32 MFMA mode: every gradient element within 2e-4 of the oracle (relative to the tensor max)."""
    tol = 2e-4
    model, params, ref, loss = grads_pair(cfg, "fp32")
    lr = ref["loss"].item()
    assert abs(loss.item() - lr) <= 1e-4 * abs(lr) + 1e-7
    bad = []
    for name, p in model.named_parameters():
        g_ref = params[name].grad
        if g_ref is None:
            assert p.grad is None, name
            continue
        assert p.grad is not None, name
        e = relerr(p.grad, g_ref)
        if not e < tol:
            bad.append((name, e))
    assert not bad, bad


@pytest.mark.parametrize("cfg", CASES + PEAKY_SMALL, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_param_grads_bf16(cfg):
    """bf16 MFMA mode.  The L1 loss gradient is sign(pred - target): bf16 rounding of the forward
    flips the sign of the few entries with pred ~= target, so element-wise comparison of the
    end-to-end gradient is not meaningful.  (1) end to end: loss and whole-gradient cosine; (2) kernels: with
    the oracle's sign pattern fed to the backward, dx0 and every gradient tensor in relative L2 against the
    oracle.  Bars: the BF16_* constants above (<= 2x measured)."""
    model, params, ref, loss = grads_pair(cfg, "bf16")
    lr = ref["loss"].item()
    # peaky rows: 3-4x the bf16 noise of the uniform-attention cases per block (tests/test_gpu_depth12.py: 1.3e-2 / 1.45e-2 per block)
    pk = 4.0 if "qkv_scale" in cfg else 1.0
    assert abs(loss.item() - lr) <= pk * BF16_LOSS * abs(lr)
    ga, gb = [], []
    for name, p in model.named_parameters():
        if params[name].grad is not None:
            ga.append(p.grad.detach().double().cpu().reshape(-1))
            gb.append(params[name].grad.double().reshape(-1))
    ga, gb = torch.cat(ga), torch.cat(gb)
    cos = float((ga * gb).sum() / (ga.norm() * gb.norm()))
    assert cos > 1.0 - pk * pk * (1.0 - BF16_COS), cos
    # (2) same sign pattern as the oracle
    from maskedsst_amd.masking import inverse_csr
    eng = model.engine()
    masks = model.last_masks
    x = ref["x"].cuda()
    out = eng.simmim_forward_stages(x, masks[0], masks[1])
    sgn = torch.sign(ref["pred"] - ref["target"]).detach().cuda().contiguous()
    ptr, pos = inverse_csr(masks[1].numpy(), eng.S * eng.N)
    dy = eng.head_bwd(out["enc_out"], sgn, torch.from_numpy(ptr).cuda(), torch.from_numpy(pos).cuda())
    dx0 = eng.blocks_bwd(out["acts"], out["x1s"], dy)
    eng.tokenize_bwd(x, masks[0].to(torch.uint8).cuda(), dx0)
    torch.cuda.synchronize()
    dx0_err = rel_l2(dx0, ref["tok_masked"].grad)
    flat = {id(p): n for n, p in eng.trainable()}
    errs = {}
    for name, p in model.named_parameters():
        g_ref = params[name].grad
        if g_ref is None:
            continue
        errs[name] = rel_l2(eng.fp.view(flat[id(p)], eng.fp.grad), g_ref)
    worst = max(errs, key=errs.get)
    record("param_grads_bf16", cfg=cfg, loss_err=abs(loss.item() - lr) / abs(lr), cos=cos, dx0_err=dx0_err,
           worst_grad=errs[worst], worst_grad_name=worst)
    assert dx0_err < (10.0 if pk > 1 else 1.0) * BF16_DX0, dx0_err    # (peaky: measured 1.8e-2 ... 2.5e-2 through the two blocks: 1.3e-2 per block)
    bad = [(n, e) for n, e in errs.items() if not e < pk * BF16_GRAD]
    assert not bad, bad


@pytest.mark.parametrize("drop", [(0.0, 0), (0.1, 1234)], ids=["nodrop", "drop0.1"])
@pytest.mark.parametrize("cfg", [dict(bands=200, depth=2, B=5), dict(bands=50, depth=2, B=4), dict(bands=10, depth=1, B=4)],
                         ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
@pytest.mark.parametrize("tuned", [0, 128], ids=["r4", "r3"])
def test_attn_bwd_kernels_agree(cfg, drop, tuned, monkeypatch):
    """The tuned bf16 attention backward kernels -- round 3, two heads per workgroup (msst_bwd4.hip; the default), round 3, one
    head per workgroup (msst_bwd3.hip: one GEMM per wave, 32x32x16 MFMAs, swizzled LDS tiles; MSST_DBG=128, and the fallback for
    an odd head count), both fed with the LN1 rows saved by the forward and the
    pre-dropped bf16 da rows left by the MLP half -- against the template kernel (msst_bwd.hip, MSST_DBG=16; re-reads
    x / dx1, renormalises, applies the to_out dropout itself): same bf16 operands and the same dropout masks up to summation
    order, so every gradient tensor must agree far inside the bf16-vs-oracle tolerance (spatial and spectral tiles, 64- and
    short-sequence masking, padding rows, a partial last tile, with and without dropout)."""
    model, params, x = build_product(cfg, precision="bf16", device="cuda")
    eng = model.engine()
    masks = model.draw_masks(cfg["B"])
    out = eng.simmim_forward_stages(x.cuda(), masks[0], masks[1], drop=drop)
    dy = torch.randn_like(out["enc_out"]) * 1e-3

    def run():
        dx0 = eng.blocks_bwd(out["acts"], out["x1s"], dy.clone(), drop=drop)
        torch.cuda.synchronize()
        return dx0.clone(), eng.fp.grad.clone()

    monkeypatch.setenv("MSST_DBG", str(tuned))
    dx_new, g_new = run()
    monkeypatch.setenv("MSST_DBG", "16")
    dx_old, g_old = run()
    monkeypatch.delenv("MSST_DBG")
    e_dx = rel_l2(dx_new, dx_old)
    # r3 / r2 round where the template rounds (measured 1.6e-4 dx, 1.6e-3 worst gradient tensor); r4 rounds the d(LN1 out)
    # partial of a head PAIR to bf16 (A's rows, then the sum) where the others round one partial per head: a bf16-level
    # difference (measured 7.6e-4 dx, 3.1e-3 worst gradient tensor), invisible against the oracle (test_param_grads_bf16)
    bar_dx, bar_g = (2.7e-3, 1.1e-2) if tuned == 0 else (8.5e-4, 6.5e-3)   # 3.5x the measured values above
    assert e_dx < bar_dx, e_dx
    bad, worst = [], 0.0
    for name, p in eng.trainable():
        a, b = eng.fp.view(name, g_new), eng.fp.view(name, g_old)
        if float(b.abs().max()) == 0.0:
            continue
        e = rel_l2(a, b)
        worst = max(worst, e)
        if not e < bar_g:
            bad.append((name, e))
    record("attn_bwd_kernels_agree", cfg=cfg, drop=list(drop), kernel={0: "r4", 128: "r3"}[tuned], dx=e_dx, worst_grad=worst)
    assert not bad, bad


def test_attn_bwd_two_head_vs_one_head_at_bench_batch(monkeypatch):
    """BASELINE.json's batch (256 cubes of 8x8x200: 80 tiles per workgroup, the multi-tile walk with both row buffers, the LDS-DMA
    row requests and the staggered copy-out in steady state) through one spatial and one spectral block: the two-head attention
    backward (msst_bwd4.hip) against the one-head kernel (msst_bwd3.hip) on the same saved rows and the same dropout masks.  The
    two differ only in where d(LN1 out) partials are rounded to bf16 (per head pair / per head)."""
    cfg = dict(bands=200, depth=1, B=256)
    model, params, x = build_product(cfg, precision="bf16", device="cuda")
    eng = model.engine()
    masks = model.draw_masks(cfg["B"])
    drop = (0.1, 4321)
    out = eng.simmim_forward_stages(x.cuda(), masks[0], masks[1], drop=drop)
    dy = torch.randn_like(out["enc_out"]) * 1e-3

    def run(flag):
        monkeypatch.setenv("MSST_DBG", str(flag))
        dx0 = eng.blocks_bwd(out["acts"], out["x1s"], dy.clone(), drop=drop)
        torch.cuda.synchronize()
        return dx0.clone(), eng.fp.grad.clone()

    dx4, g4 = run(0)
    dx3, g3 = run(128)
    monkeypatch.delenv("MSST_DBG")
    assert torch.isfinite(dx4).all() and torch.isfinite(g4).all()
    e_dx = rel_l2(dx4, dx3)
    worst = 0.0
    for name, p in eng.trainable():
        b = eng.fp.view(name, g3)
        if float(b.abs().max()) == 0.0:
            continue
        worst = max(worst, rel_l2(eng.fp.view(name, g4), b))
    record("attn_bwd_two_head_vs_one_head_b256", dx=e_dx, worst_grad=worst)
    assert e_dx < 1e-3, e_dx        # measured 2.9e-4
    assert worst < 8e-3, worst    # measured 2.3e-3


@pytest.mark.parametrize("heads", [2, 3, 4, 6])
def test_attn_bwd_tuned_kernels_other_head_counts(heads, monkeypatch):
    """Head counts other than 8 run the 4-wave forward, which also saves its bf16 LN1 rows: they are checked against LN1(x)
    computed in torch, then the two-head attention backward (even head counts: one, two and three head pairs per tile chunk) or
    the one-head kernel (3 heads) runs on them against the template kernel (which re-reads x and renormalises)."""
    cfg = dict(bands=50, depth=1, B=3, heads=heads)
    model, params, x = build_product(cfg, precision="bf16", device="cuda")
    eng = model.engine()
    masks = model.draw_masks(cfg["B"])
    drop = (0.1, 99)
    out = eng.simmim_forward_stages(x.cuda(), masks[0], masks[1], drop=drop)
    dy = torch.randn_like(out["enc_out"]) * 1e-3
    for i, (sname, l) in enumerate(eng._layers()):
        saved = getattr(out["x1s"][i], "_msst_xn", None)
        assert saved is not None
        g = eng.fp.view(f"{sname}.{l}.ln1_g", eng.fp.flat).float()
        b = eng.fp.view(f"{sname}.{l}.ln1_b", eng.fp.flat).float()
        want = torch.nn.functional.layer_norm(out["acts"][i].float(), (96,), g, b, 1e-5)
        assert rel_l2(saved.float().reshape(want.shape), want) < 4e-3   # bf16 rounding of the rows: 2^-9 / sqrt(3) = 1.1e-3 expected

    def run(flag):
        monkeypatch.setenv("MSST_DBG", str(flag))
        dx0 = eng.blocks_bwd(out["acts"], out["x1s"], dy.clone(), drop=drop)
        torch.cuda.synchronize()
        return dx0.clone(), eng.fp.grad.clone()

    dx_new, g_new = run(0)
    dx_old, g_old = run(16)
    monkeypatch.delenv("MSST_DBG")
    e_dx = rel_l2(dx_new, dx_old)
    worst = 0.0
    for name, p in eng.trainable():
        ref = eng.fp.view(name, g_old)
        if float(ref.abs().max()) == 0.0:
            continue
        worst = max(worst, rel_l2(eng.fp.view(name, g_new), ref))
    record("attn_bwd_tuned_other_head_counts", heads=heads, dx=e_dx, worst_grad=worst)
    assert e_dx > 0.0, "the tuned kernel did not run (identical to the template)"
    # measured: two-head kernel 4.0e-4 / 2.4e-3 (one bf16 partial per head pair), one-head kernel 1.3e-5 / 1.3e-4 (the template's rounding points)
    bar_dx, bar_g = (1.4e-3, 8.4e-3) if heads % 2 == 0 else (1e-4, 5e-4)   # 3.5x measured (even) / 4-8x (odd)
    assert e_dx < bar_dx, e_dx
    assert worst < bar_g, worst


CHAIN_CASES = [
    dict(bands=200, depth=2, B=5),                               # 100 row tiles, four partials (8 heads)
    dict(bands=50, depth=2, B=4),
    dict(bands=30, depth=2, B=3, heads=2, image_size=6, mask_patch_size=2),   # one partial; 324 tokens: a partial last row tile
    dict(bands=50, depth=1, B=3, heads=4),                       # two partials
    dict(bands=50, depth=2, B=3, heads=6),                       # three partials
    dict(bands=200, depth=1, B=256),                             # BASELINE.json's batch: 20 tiles per workgroup of the fused launch
]


@pytest.mark.parametrize("drop", [(0.0, 0), (0.1, 777)], ids=["nodrop", "drop0.1"])
@pytest.mark.parametrize("cfg", CHAIN_CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_chained_backward_matches_unchained(cfg, drop, monkeypatch):
    """msst_block_bwd_chain (round 4: LN1 backward of block i + MLP-half backward of block i - 1 as ONE launch, dx of block i
    kept in LDS; msst_bwd5.hip) against msst_block_bwd (the two halves as separate HBM-roofline kernels): the same arithmetic
    on the same bf16 operands and dropout masks.  What differs is fp32 summation order (the 8-lane row sums of the LN half, 256
    instead of 512 MLP slabs); a last-bit difference in dx flips the bf16 rounding of an MFMA operand now and then, so the two
    agree to 1e-7 for some dy and to 1e-4 for others (measured: dx0 2e-8 ... 9.3e-5, worst gradient tensor 8.7e-4; deterministic
    per input, tools/diag_chain.py holds both against the fp32-mode backward: 1.213e-3 each) -- the bars are those of the
    other same-rounding-point kernel pairs (test_attn_bwd_kernels_agree), far inside the bf16-vs-oracle ones."""
    model, params, x = build_product(cfg, precision="bf16", device="cuda")
    eng = model.engine()
    masks = model.draw_masks(cfg["B"])
    out = eng.simmim_forward_stages(x.cuda(), masks[0], masks[1], drop=drop)
    dy = torch.randn_like(out["enc_out"]) * 1e-3

    def run(chain):
        monkeypatch.setenv("MSST_BWD_CHAIN", chain)
        eng.fp.grad.zero_()
        dx0 = eng.blocks_bwd(out["acts"], out["x1s"], dy.clone(), drop=drop)
        torch.cuda.synchronize()
        return dx0.clone(), eng.fp.grad.clone()

    dx_c, g_c = run("1")
    dx_u, g_u = run("0")
    monkeypatch.delenv("MSST_BWD_CHAIN")
    assert torch.isfinite(dx_c).all() and torch.isfinite(g_c).all()
    e_dx = rel_l2(dx_c, dx_u)
    worst, bad = 0.0, []
    for name, p in eng.trainable():
        b = eng.fp.view(name, g_u)
        if float(b.abs().max()) == 0.0:
            continue
        e = rel_l2(eng.fp.view(name, g_c), b)
        worst = max(worst, e)
        if not e < 8e-3:          # (measured <= 3.4e-3 with xhat from the saved bf16 rows on the chained side; 8.7e-4 before)
            bad.append((name, e))
    record("chained_backward_matches_unchained", cfg=cfg, drop=list(drop), dx=e_dx, worst_grad=worst)
    assert e_dx < 1.5e-3, e_dx    # (round 6: the chained form takes xhat of LN1 from the saved bf16 rows, MSST_LN1_FROM_XN: measured <= 5.8e-4)
    assert not bad, bad


DEFER_CASES = [
    dict(bands=200, depth=2, B=5),
    dict(bands=50, depth=3, B=4),                                # runs of three calls per stack
    dict(bands=30, depth=2, B=3, heads=2, image_size=6, mask_patch_size=2),
    dict(bands=50, depth=1, B=3, heads=4),                       # one call per run: the spectral run's fused MLP half belongs to the spatial block
]


@pytest.mark.parametrize("drop", [(0.0, 0), (0.1, 777)], ids=["nodrop", "drop0.1"])
@pytest.mark.parametrize("cfg", DEFER_CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_deferred_slab_reduction_is_bit_identical(cfg, drop, monkeypatch):
    """msst_block_bwd_reduce (one slab reduction per run of same-mode blocks: MSST_BWD_DEFER_REDUCE) against the reduction at
    the end of every msst_block_bwd_chain call: the same slabs summed in the same order -- every gradient bit for bit, and the
    hooks that announce finished blocks fire once per block in backward order either way."""
    model, params, x = build_product(cfg, precision="bf16", device="cuda")
    eng = model.engine()
    masks = model.draw_masks(cfg["B"])
    out = eng.simmim_forward_stages(x.cuda(), masks[0], masks[1], drop=drop)
    dy = torch.randn_like(out["enc_out"]) * 1e-3
    assert eng._grad_stride(len(eng._layers())) is not None, "flat gradient layout is not a constant stride per block"

    def run(defer):
        monkeypatch.setenv("MSST_BWD_DEFER", defer)
        eng.fp.grad.zero_()
        fired = []
        old = eng._fire
        eng._fire = lambda name: fired.append(name)
        try:
            dx0 = eng.blocks_bwd(out["acts"], out["x1s"], dy.clone(), drop=drop)
        finally:
            eng._fire = old
        torch.cuda.synchronize()
        return dx0.clone(), eng.fp.grad.clone(), fired

    dx_d, g_d, f_d = run("1")
    dx_i, g_i, f_i = run("0")   # (the default)
    monkeypatch.delenv("MSST_BWD_DEFER")
    assert f_d == f_i and len(f_d) == len(eng._layers())
    assert torch.equal(dx_d, dx_i)
    assert float(g_d.abs().max()) > 0.0
    bad = [name for name, p in eng.trainable() if not torch.equal(eng.fp.view(name, g_d), eng.fp.view(name, g_i))]
    assert not bad, bad


@pytest.mark.parametrize("cfg", [dict(bands=200, depth=2, B=5), dict(bands=50, depth=2, B=4)], ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_bf16_x1_rows(cfg, monkeypatch):
    """MSST_X1_BF16 (round 4): the forward saves the mid-block residual x1 as bf16 rows instead of fp32, the MLP-half backward
    (standalone and fused with LN1) widens them.  The saved rows are the rounded CENTRED fp32 ones (round 5); the gradients move by what
    the LN2 statistics of rounded rows move them -- a bf16-level difference, held against the fp32-row backward here and, like
    every bf16 path, against the oracle in test_gpu_dropout / test_gpu_depth12 (which run with bf16 rows by default)."""
    drop = (0.1, 777)
    model, params, x = build_product(cfg, precision="bf16", device="cuda")
    eng = model.engine()
    masks = model.draw_masks(cfg["B"])

    def run(flag):
        monkeypatch.setenv("MSST_X1_BF16", flag)
        out = eng.simmim_forward_stages(x.cuda(), masks[0], masks[1], drop=drop)
        torch.manual_seed(11)
        dy = torch.randn_like(out["enc_out"]) * 1e-3
        eng.fp.grad.zero_()
        dx0 = eng.blocks_bwd(out["acts"], out["x1s"], dy, drop=drop)
        torch.cuda.synchronize()
        return out, dx0.clone(), eng.fp.grad.clone()

    o16, dx16, g16 = run("1")
    o32, dx32, g32 = run("0")
    monkeypatch.delenv("MSST_X1_BF16")
    assert all(t.dtype == torch.bfloat16 for t in o16["x1s"]) and all(t.dtype == torch.float32 for t in o32["x1s"])
    assert torch.equal(o16["enc_out"], o32["enc_out"])                      # the forward itself does not change
    for a, b in zip(o16["x1s"], o32["x1s"]):
        # round 5: the bf16 rows are bf16(x1 - row mean) -- LN2, the only reader, does not see a per-row constant, and the rounding
        # error is then relative to the row's spread instead of its offset (test_bf16_x1_rows_with_a_large_row_offset)
        c = b - b.mean(dim=-1, keepdim=True)
        assert float((a.float() - c).abs().max()) <= 2.0 ** -8 * float(c.abs().max()) + 1e-5
    e_dx = rel_l2(dx16, dx32)
    worst, bad = 0.0, []
    for name, p in eng.trainable():
        b = eng.fp.view(name, g32)
        if float(b.abs().max()) == 0.0:
            continue
        e = rel_l2(eng.fp.view(name, g16), b)
        worst = max(worst, e)
        if not e < 1.8e-2:
            bad.append((name, e))
    record("bf16_x1_rows", cfg=cfg, dx=e_dx, worst_grad=worst)
    # measured (profiles/r04_parity_measured.jsonl): dx 0.95e-3 / 1.1e-3, worst gradient tensor 4.9e-3 / 5.2e-3 -- the size of every
    # other bf16 rounding-point difference; against the oracle the as-benchmarked gradients do not move (worst 5.18e-3 -> 5.20e-3,
    # median 2.66e-3 -> 2.67e-3).  Bars at 3.5x measured.
    assert e_dx < 4e-3, e_dx
    assert not bad, bad


LSE_CASES = [dict(bands=200, depth=2, B=5), dict(bands=50, depth=2, B=4), dict(bands=30, depth=1, B=3, image_size=6, mask_patch_size=2),
             dict(bands=200, depth=1, B=256),
             # round 6: peaky attention rows (to_qkv.weight x4: logit std ~5, max ~30, row maximum of p 0.5-0.8; tests/test_gpu_depth12.py)
             dict(bands=200, depth=2, B=5, qkv_scale=4), dict(bands=50, depth=2, B=4, qkv_scale=4), dict(bands=50, depth=12, B=8, qkv_scale=4)]


@pytest.mark.parametrize("drop", [(0.0, 0), (0.1, 777)], ids=["nodrop", "drop0.1"])
@pytest.mark.parametrize("cfg", LSE_CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_saved_softmax_statistics(cfg, drop, monkeypatch):
    """Round 5: the role-split forward saves lse = log2 of every query's softmax denominator (exponent domain of the kernels,
    max folded in) per (tile, head, row); the two-head attention backward then computes p = exp2(s c - lse) directly instead
    of its own max / sum / reciprocal (reference softmax: vit_spatial_spectral.py:71-73).
    (1) the saved values against a torch restatement from the saved LN1 rows and the bf16 weights the kernels used;
    (2) the backward with the saved statistics against the backward that normalises by itself (MSST_LSE=0) on the same rows
        and masks: same rounding points for q / k / v, p differs by the fp32 summation order of the two kernels' scores;
    (3) round 6: BOTH backwards against the oracle's autograd through the same blocks (same tokens in, same dy, the kernels' dropout
        masks) -- with saved statistics the rows of p no longer sum to 1 by construction, so the question is whether the lse path
        sits further from the exact gradient than the self-normalising one, in particular on peaky rows (qkv_scale cases)."""
    model, params, x = build_product(cfg, precision="bf16", device="cuda")
    eng = model.engine()
    masks = model.draw_masks(cfg["B"])

    def run(flag):
        monkeypatch.setenv("MSST_LSE", flag)
        out = eng.simmim_forward_stages(x.cuda(), masks[0], masks[1], drop=drop)
        torch.manual_seed(11)
        dy = torch.randn_like(out["enc_out"]) * 1e-3
        eng.fp.grad.zero_()
        dx0 = eng.blocks_bwd(out["acts"], out["x1s"], dy, drop=drop)
        torch.cuda.synchronize()
        run.dy = dy
        return out, dx0.clone(), eng.fp.grad.clone()

    o1, dx1, g1 = run("1")
    o0, dx0, g0 = run("0")
    monkeypatch.delenv("MSST_LSE")
    assert all(getattr(t, "_msst_lse", None) is not None for t in o1["x1s"]) and all(getattr(t, "_msst_lse", None) is None for t in o0["x1s"])
    assert torch.equal(o1["enc_out"], o0["enc_out"])   # the forward's arithmetic does not change
    # (1) block 0 (spatial): sequences = (b, c), 64 // N sequences per tile, rows in token order
    H, S, N = eng.enc.heads, eng.S, eng.N
    B = cfg["B"]
    # operands as the forward rounded them: IEEE half (MSST_FWD_HALF, the default: LN1 rows straight from the fp32 statistics) or
    # bf16 (the saved LN1 rows ARE its operands)
    pre = "encoder.spatial_spectral_transformer.1.layers.0.0."
    xn, low = ln1_rows_as_used(o1["tok_masked"], params[pre + "norm.weight"].cuda(), params[pre + "norm.bias"].cuda(), o1["x1s"][0], eng.fwd_half)
    ref = lse_restatement(xn.reshape(B * S, N, 96), params[pre + "fn.to_qkv.weight"].cuda(), H, low)      # log2 sum 2^s, [B S, H, N]
    lse = o1["x1s"][0]._msst_lse
    TS = 64 // N
    nseq = B * S
    ntiles = (nseq + TS - 1) // TS
    assert lse.numel() == ntiles * H * 64 + B * S * N          # [tiles][heads][64] lse | [tokens] rstd of LN1 (MSST_VERSION 104)
    got, rstd_got = saved_lse_rows(lse, H, N, nseq)
    x_in = o1["tok_masked"].float().reshape(B * S * N, 96)
    rstd_ref = torch.rsqrt(x_in.var(dim=-1, unbiased=False) + 1e-5)
    assert float(((rstd_got - rstd_ref).abs() / rstd_ref).max()) < 1e-5
    err = float((got.double() - ref).abs().max())
    # bf16 q / k (three significant digits) in scores of magnitude ~1: measured ~4e-3; the scores of the peaky cases are 16x larger
    assert err < 2e-2 * float(cfg.get("qkv_scale", 1)) ** 2, err
    # (2)
    e_dx = rel_l2(dx1, dx0)
    worst, bad = 0.0, []
    for name, p in eng.trainable():
        b = eng.fp.view(name, g0)
        if float(b.abs().max()) == 0.0:
            continue
        e = rel_l2(eng.fp.view(name, g1), b)
        worst = max(worst, e)
        if not e < 6.3e-3:
            bad.append((name, e))
    # (3) the oracle's autograd through the same blocks
    from oracle import transformer_forward
    from dropout import make_drop_fn
    ocfg = oracle_cfg_from(cfg)
    blk = {k: v.clone().requires_grad_(True) for k, v in params.items() if "spatial_spectral_transformer" in k}
    tok = o1["tok_masked"].detach().float().cpu().requires_grad_(True)
    y = transformer_forward(blk, tok, ocfg, drop_fn=make_drop_fn(drop[0], drop[1], ocfg.S, ocfg.N, ocfg.heads) if drop[0] else None)
    y.backward(run.dy.cpu())
    flat = {id(q): n for n, q in eng.trainable()}
    vs_oracle = {}
    for tag, dxk, gk in (("lse", dx1, g1), ("own", dx0, g0)):
        ge = {pn: rel_l2(eng.fp.view(flat[id(q)], gk), blk[pn].grad) for pn, q in model.named_parameters() if pn in blk}
        vs_oracle[tag] = dict(dx=rel_l2(dxk, tok.grad), worst_grad=max(ge.values()), median_grad=float(np.median(list(ge.values()))))
    peaky = "qkv_scale" in cfg
    record("saved_softmax_statistics", cfg=cfg, drop=list(drop), lse_abs_err=err, dx=e_dx, worst_grad=worst,
           oracle_lse_dx=vs_oracle["lse"]["dx"], oracle_own_dx=vs_oracle["own"]["dx"],
           oracle_lse_worst_grad=vs_oracle["lse"]["worst_grad"], oracle_own_worst_grad=vs_oracle["own"]["worst_grad"])
    # the lse path may not sit further from the exact gradient than the self-normalising one (measured: equal to three digits in
    # every case, peaky ones included -- dx 5.78e-2 vs 5.77e-2 at depth 2 x4; 10 % / 20 % slack for rounding luck)
    assert vs_oracle["lse"]["dx"] < 1.1 * vs_oracle["own"]["dx"] + 1e-4, vs_oracle
    assert vs_oracle["lse"]["worst_grad"] < 1.2 * vs_oracle["own"]["worst_grad"] + 1e-4, vs_oracle
    if not peaky:
        assert e_dx < 1.5e-3, e_dx
        assert not bad, bad
    else:
        # peaky rows: the two backwards differ by the fp32 summation order of their scores, amplified by the model (measured: dx
        # 7.3e-3, worst gradient 9.4e-3 at depth 2; 1.6e-2 / 2.1e-2 through the 24 blocks of the depth-12 fixture shape)
        assert e_dx < 6e-2, e_dx
        assert worst < 8e-2, (worst, bad[:3])


XN_CASES = [dict(bands=200, depth=2, B=5), dict(bands=50, depth=3, B=4), dict(bands=30, depth=2, B=3, image_size=6, mask_patch_size=2),
            dict(bands=200, depth=2, B=256), dict(bands=20, depth=2, B=3, heads=4), dict(bands=50, depth=12, B=8, qkv_scale=4)]


@pytest.mark.parametrize("drop", [(0.0, 0), (0.1, 4242)], ids=["nodrop", "drop0.1"])
@pytest.mark.parametrize("cfg", XN_CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_ln1_backward_from_saved_rows(cfg, drop, monkeypatch):
    """Round 6 (MSST_LN1_FROM_XN): the fused LN1 + MLP launch of the chained backward takes xhat of LN1 (reference
    vit_spatial_spectral.py:22-29) from the forward's saved bf16 LN1 rows -- xhat = (row - beta) / gamma -- and rstd from the tail of
    the statistics buffer, instead of re-reading and re-normalising the fp32 block input.  Against the same backward on the fp32 rows
    (MSST_LN1_XN=0), same operands and masks: dx0 and every gradient tensor at the bf16 level; and against the oracle's autograd
    through the same blocks it may not sit further away than the fp32-row form (10 % slack).  LN1 parameters off their initial
    values (gamma 0.5 .. 1.5, beta +-0.3), as after training."""
    from oracle import transformer_forward
    from dropout import make_drop_fn
    model, params, x = build_product(cfg, precision="bf16", device="cuda")
    torch.manual_seed(3)
    with torch.no_grad():
        for n, q in model.named_parameters():
            if n.endswith(".0.norm.weight"):
                q.copy_(0.5 + torch.rand(96)); params[n].copy_(q.cpu())
            if n.endswith(".0.norm.bias"):
                q.copy_(0.6 * torch.rand(96) - 0.3); params[n].copy_(q.cpu())
    eng = model.engine()
    masks = model.draw_masks(cfg["B"])
    out = eng.simmim_forward_stages(x.cuda(), masks[0], masks[1], drop=drop)
    torch.manual_seed(11)
    dy = torch.randn_like(out["enc_out"]) * 1e-3

    def run(flag):
        monkeypatch.setenv("MSST_LN1_XN", flag)
        eng.fp.grad.zero_()
        dx0 = eng.blocks_bwd(out["acts"], out["x1s"], dy.clone(), drop=drop)
        torch.cuda.synchronize()
        return dx0.clone(), eng.fp.grad.clone(), eng.last_bwd_ln1_from_xn

    dx_n, g_n, used_n = run("1")
    dx_x, g_x, used_x = run("0")
    monkeypatch.delenv("MSST_LN1_XN")
    H = cfg.get("heads", 8)
    assert used_n == (H == 8) and not used_x     # the role-split forward (8 heads) saves rstd; other head counts keep the fp32 rows
    e_dx = rel_l2(dx_n, dx_x)
    worst = 0.0
    for name, q in eng.trainable():
        b = eng.fp.view(name, g_x)
        if float(b.abs().max()) > 0.0:
            worst = max(worst, rel_l2(eng.fp.view(name, g_n), b))
    ocfg = oracle_cfg_from(cfg)
    blk = {k: v.clone().requires_grad_(True) for k, v in params.items() if "spatial_spectral_transformer" in k}
    tok = out["tok_masked"].detach().float().cpu().requires_grad_(True)
    y = transformer_forward(blk, tok, ocfg, drop_fn=make_drop_fn(drop[0], drop[1], ocfg.S, ocfg.N, ocfg.heads) if drop[0] else None)
    y.backward(dy.cpu())
    flat = {id(q): n for n, q in eng.trainable()}
    vs = {}
    for tag, dxk, gk in (("xn", dx_n, g_n), ("x", dx_x, g_x)):
        ge = {pn: rel_l2(eng.fp.view(flat[id(q)], gk), blk[pn].grad) for pn, q in model.named_parameters() if pn in blk}
        vs[tag] = dict(dx=rel_l2(dxk, tok.grad), worst_grad=max(ge.values()), ln1=max(v for k, v in ge.items() if ".0.norm." in k))
    record("ln1_backward_from_saved_rows", cfg=cfg, drop=list(drop), dx=e_dx, worst_grad=worst,
           oracle_xn_dx=vs["xn"]["dx"], oracle_x_dx=vs["x"]["dx"], oracle_xn_worst_grad=vs["xn"]["worst_grad"],
           oracle_x_worst_grad=vs["x"]["worst_grad"], oracle_xn_ln1_grad=vs["xn"]["ln1"], oracle_x_ln1_grad=vs["x"]["ln1"])
    if H == 8:
        # measured on MI355X: dx <= 9.4e-4, worst gradient tensor <= 4.0e-3 (the x4 depth-12 shape, which amplifies: 1.6e-2 / 2.0e-2);
        # against the oracle the two forms are equal to three digits in dx (1.10e-3 both) and within +-15 % on their worst tensor
        bar_dx, bar_g = (6e-2, 8e-2) if "qkv_scale" in cfg else (3e-3, 1.2e-2)
        assert e_dx < bar_dx and worst < bar_g, (e_dx, worst)
        assert vs["xn"]["dx"] < 1.1 * vs["x"]["dx"] + 1e-4 and vs["xn"]["worst_grad"] < 1.3 * vs["x"]["worst_grad"] + 1e-4, vs


def test_ln1_from_saved_rows_guard(monkeypatch):
    """The division by gamma is refused when it would amplify the rows' bf16 rounding (max |beta / gamma| > 12, or a gamma of 0): the
    engine then keeps the fp32 block input for LN1's backward -- no flag, same results as MSST_LN1_XN=0 bit for bit."""
    cfg = dict(bands=50, depth=2, B=4)
    model, params, x = build_product(cfg, precision="bf16", device="cuda")
    with torch.no_grad():
        for n, q in model.named_parameters():
            if n.endswith("layers.1.0.norm.weight"):
                q[5] = 0.0
    eng = model.engine()
    masks = model.draw_masks(cfg["B"])
    out = eng.simmim_forward_stages(x.cuda(), masks[0], masks[1])
    dy = torch.randn_like(out["enc_out"]) * 1e-3
    res = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("MSST_LN1_XN", flag)
        eng.fp.grad.zero_()
        dx0 = eng.blocks_bwd(out["acts"], out["x1s"], dy.clone())
        torch.cuda.synchronize()
        assert not eng.last_bwd_ln1_from_xn
        res[flag] = (dx0.clone(), eng.fp.grad.clone())
    assert torch.equal(res["1"][0], res["0"][0]) and torch.equal(res["1"][1], res["0"][1])
    assert torch.isfinite(res["1"][1]).all()


def test_bf16_x1_rows_with_a_large_row_offset(monkeypatch):
    """bf16 x1 rows are the default, and the backward recomputes the LN2 statistics from them; a residual stream with
    |row mean| >> row std (a trained or deep model: the parity tests here run at random initialisation, |x| ~ std; tests/test_gpu_trained_state.py holds such
    a stream against float64) would lose
    them to the rounding -- 2^-9 |x| / std -- if the rows were rounded as they are.  They are saved CENTRED (msst_fwd3.hip, ln2()),
    so the offset does not matter: tokens + 30 (|mean| / std ~ 30) give the same agreement with the fp32-row backward as tokens."""
    cfg, drop = dict(bands=50, depth=2, B=4), (0.1, 777)
    model, params, x = build_product(cfg, precision="bf16", device="cuda")
    eng = model.engine()
    eng.prep_weights()
    x0 = eng.tokenize(x.cuda(), None)
    res = {}
    for off in (0.0, 30.0):
        for flag in ("1", "0"):
            monkeypatch.setenv("MSST_X1_BF16", flag)
            acts, x1s = eng.blocks_fwd(x0 + off, save=True, drop=drop)
            torch.manual_seed(11)
            dy = torch.randn_like(acts[-1]) * 1e-3
            eng.fp.grad.zero_()
            dx0 = eng.blocks_bwd(acts, x1s, dy, drop=drop)
            torch.cuda.synchronize()
            res[(off, flag)] = (dx0.clone(), eng.fp.grad.clone(), x1s[0].dtype)
    monkeypatch.delenv("MSST_X1_BF16")
    errs = {}
    for off in (0.0, 30.0):
        (dx16, g16, t16), (dx32, g32, t32) = res[(off, "1")], res[(off, "0")]
        assert t16 == torch.bfloat16 and t32 == torch.float32
        worst = 0.0
        for name, p in eng.trainable():
            b = eng.fp.view(name, g32)
            if float(b.abs().max()) > 0.0:
                worst = max(worst, rel_l2(eng.fp.view(name, g16), b))
        errs[off] = (rel_l2(dx16, dx32), worst)
    record("bf16_x1_rows_large_offset", dx_plain=errs[0.0][0], dx_offset30=errs[30.0][0], worst_grad_plain=errs[0.0][1], worst_grad_offset30=errs[30.0][1])
    assert errs[30.0][0] < 4e-3 and errs[30.0][1] < 1.8e-2, errs          # the bars of test_bf16_x1_rows
    assert errs[30.0][0] < 3 * errs[0.0][0] + 1e-4 and errs[30.0][1] < 3 * errs[0.0][1] + 1e-4, errs   # ... and no worse with the offset than without
