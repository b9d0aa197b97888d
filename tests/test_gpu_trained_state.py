"""The block kernels in a trained state, teacher-forced against float64.

The sweeps of tests/test_gpu_seq_lengths.py, test_gpu_launch_geometry.py and test_gpu_backward.py build their models with
tests/util.py::build_product and run them at random initialisation: every LayerNorm has gamma = 1 and beta = 0, the residual stream
has |x| ~ std.  A kernel that forgets gamma in a dx path, applies it on the wrong side of the mean subtraction or drops beta when it
rebuilds xhat computes the same bits there as a right one -- and each role kernel carries that arithmetic in a copy of its own (fp32
template forward / backward, 4-wave forward, role-split forward with half and bf16 operands, bf16 MLP half, LN1 backward, the fused
LN1 + MLP launch of the chain).  This file runs the same comparison (the inputs, the float64 oracle, the helpers and the bars of
test_gpu_seq_lengths.py) in the three states of tests/trained_util.py -- `affine`: signed gammas, betas and biases like a trained
model's in both LayerNorms of every block; `stream`: per-channel scales, two massive channels and +-30 per sample on the block input;
`both` -- at the four smallest shapes at which the tile packing differs (trained_util.SHAPES):

  test_blocks_teacher_forced              the six families of test_gpu_launch_geometry.FAMILIES x state, one block against
                                          oracle.model.block in float64; bf16 with 8 heads also the saved lse / rstd
  test_variants_with_their_own_layernorm  MSST_FWD_HALF=0, MSST_X1_BF16=0, MSST_DBG=16 / 64 / 128 at spectral 22 and spatial 64, states
                                          affine and both; each run shows that its variant ran
  test_production_pair                    blocks_fwd + blocks_bwd of the depth-1 model against float64 autograd through both blocks:
                                          chained with MSST_LN1_FROM_XN (asserted on), MSST_LN1_XN=0, MSST_BWD_CHAIN=0
  test_whole_step_fp32                    one SimMIM step in fp32 with every parameter of the model off its initial value

Bars: none comes from the code under test.  FP32_BARS, BF16_BARS[8] / ["4wave"] / ["production"] and 1e-5 for rstd unchanged (the bf16
ones are 3.5x the worst init-state value over 64 lengths; the trained states use up to 1.8x of that, below).  The variants take the
bar of their forward's operand format (VARIANTS).  The saved lse is an absolute error that grows with the scores: its bar is
LSE_BARS[qkv scale] x max(1, r), r = the largest |score| of the case's float64 restatement over the same case's at the init state
(score_ratio: the reference alone; r = 0.85 .. 1.27 here).  tests/test_trained_state_host.py pins on the CPU that float32 arithmetic
reaches a quarter of FP32_BARS in every state.  max |beta / gamma| <= 0.6 and the half-operand bound stay far inside the engine's
guards, so the fast paths run: eng.fwd_half and eng.last_bwd_ln1_from_xn are asserted.

Every error goes to util.record (trained_state_teacher_forced, trained_state_variant, trained_state_production,
trained_state_step_fp32); the measured rows are profiles/trained_state_parity_measured.jsonl.  The whole file (41 tests) runs in 6 s on
one MI355X (5.97 s measured, 2.1 s of it the first test's library start; every other test below 0.2 s).

Worst errors measured on MI355X (relative L2 for bf16, max-norm relative for fp32; increment / dx - dy / worst parameter gradient):
  bf16, 8 heads               7.8e-4 (stream, spectral 22)  1.53e-2 (both, spectral 22)   2.51e-2 (stream, spatial 25: LN1 gamma)
  bf16, 8 heads, dropout 0.1  8.2e-4 (both, spectral 22)    1.49e-2 (both, spectral 22)   1.87e-2 (stream, spectral 22: LN1 gamma)
  bf16, 2 heads               5.8e-3 (affine, spatial 25)   1.38e-2 (affine, spatial 25)  2.59e-2 (both, spectral 22: LN1 gamma)
  bf16, 3 heads               6.2e-3 (stream, spatial 25)   1.68e-2 (both, spectral 22)   1.92e-2 (both, spectral 22: to_qkv)
  fp32, 8 heads               8.9e-6 (stream, spatial 64)   4.7e-6 (both, spatial 25)     7.6e-6 (stream, spectral 22: LN1 gamma)
  fp32, 3 heads               9.1e-6 (stream, spectral 20)  5.4e-6 (both, spectral 22)    3.3e-6 (stream, spatial 25: to_qkv)
  MSST_FWD_HALF=0             5.9e-3                        1.54e-2                       2.11e-2   (all five: both, spectral 22;
  MSST_X1_BF16=0              7.7e-4                        1.54e-2                       2.00e-2    worst gradient LN1 gamma)
  MSST_DBG=16                 5.9e-3                        1.52e-2                       2.25e-2
  MSST_DBG=64                 5.9e-3                        1.53e-2                       2.32e-2
  MSST_DBG=128                7.7e-4                        1.53e-2                       2.29e-2
  production pair             1.07e-3 (affine, spectral 22) 1.79e-2 (affine, spatial 25)  2.08e-2 (both, spatial 25: spectral LN1 gamma)
                              -- the same to three digits chained with LN1 from the saved rows, with MSST_LN1_XN=0 and unchained
  whole step, fp32            loss 9.4e-8, worst gradient 4.1e-7 (the tokenizer's pre_norm.weight)
  saved statistics (bf16, 8 heads): lse 4.7e-4 absolute on plain rows (stream, spectral 20; bar 1.2e-3), 9.1e-3 on peaky rows (stream,
  spectral 22; r = 1.03, bar 2.37e-2); rstd 2.3e-7
(The fp32 increment of the stream states is the float32 spacing of y, stored at magnitude ~100, against an increment of ~1: the host
test measures the same 8.9e-6 for float32 on the CPU.)

Mutations this file catches, each applied alone to a scratch copy of the kernels (arithmetic only, every address unchanged).  With every
one of them all 15 tests of tests/test_gpu_seq_lengths.py pass -- at gamma = 1, beta = 0 they are no-ops: the gap this file closes.
  (a) msst_bwd5.hip: xhat of LN1 rebuilt as row / gamma,      test_production_pair, states affine and both, all four shapes (8 tests), the
      without - beta (MSST_LN1_FROM_XN)                       default backward only: worst gradient (LN1 gamma) 0.13 .. 0.32
  (b) msst_bwd5.hip, fused LN1 + MLP launch: LN2's gamma      the same 8 tests, the default backward and MSST_LN1_XN=0: dx - dy up to 0.62,
      dropped from the dx1 path                               worst gradient up to 0.16 (MSST_BWD_CHAIN=0 does not run the launch)
  (b') msst_bwd.hip, MLP half: the same                       31 tests: every teacher-forced family, every variant, the production pair (the
                                                              MLP half of its last block; both blocks with MSST_BWD_CHAIN=0) in states
                                                              affine and both, and the whole step: dx - dy up to 1.7, worst gradient 0.34
  (c) msst_fwd3.hip: LN2's beta not added before the MLP      18 tests: bf16 8 heads with and without dropout, MSST_FWD_HALF=0, MSST_X1_BF16=0,
                                                              MSST_DBG=128, the production pair, states affine and both: increment 0.023 ..
                                                              0.080, bars 2.9e-3 .. 2.2e-2 (MSST_DBG=16 / 64 run other forwards: pass)
  (d) msst_bwd.hip, fp32 LN1 backward: dx from dy instead     5 tests: fp32 with 8 and 3 heads in states affine and both, and the whole step:
      of gamma * dy                                           dx - dy up to 1.9, gradients of the step up to 2.3
The `stream` state alone catches none of them, as it should: it is there for the residual stream (centred bf16 x1 rows, LN statistics of
rows with |mean| >> std and channels of unequal size), where the kernels hold at the bars above.
"""
import os

import pytest
import torch

from conftest import oracle_cfg_from
from util import build_product, oracle_cfg, relerr, rel_l2, record, lse_restatement
from test_gpu_seq_lengths import (BF16_BARS, FP32_BARS, LSE_BARS, Q, case_cfg, tokens_with_offsets, to_seq, make_model, block_prefix,
                                  block_inputs, block_reference, block_kernels, block_errors, check_saved_statistics)
from test_gpu_launch_geometry import FAMILIES, report
from trained_util import STATES, SHAPES, SHAPE_IDS, SNAME, MAX_RATIO, affine_edit, make_affine, state_inputs, max_beta_over_gamma

pytestmark = pytest.mark.gpu

AFFINE_STATES = ("affine", "both")
VARIANT_SHAPES = [(1, 22), (0, 64)]
# variant -> (environment, bars).  The bars follow the forward's operand format, as in the sweeps: BF16_BARS[8] was taken with IEEE-half
# operands (11 significant bits), BF16_BARS["4wave"] with bf16 ones (8 bits) -- so a role-split forward told to multiply bf16 operands
# and the two other bf16 forwards are held to the latter; the backward variants on a half-operand forward to the former
VARIANTS = {
    "fwd_half0": ({"MSST_FWD_HALF": "0"}, BF16_BARS["4wave"]),
    "x1_bf16_0": ({"MSST_X1_BF16": "0"}, BF16_BARS[8]),
    "dbg16": ({"MSST_DBG": "16"}, BF16_BARS["4wave"]),
    "dbg64": ({"MSST_DBG": "64"}, BF16_BARS["4wave"]),
    "dbg128": ({"MSST_DBG": "128"}, BF16_BARS[8]),
}
# the production pair: the default, LN1's backward on the fp32 rows, the unchained backward
BACKWARDS = {"default": {}, "ln1_xn0": {"MSST_LN1_XN": "0"}, "chain0": {"MSST_BWD_CHAIN": "0"}}


def shape_of(cfg):
    return cfg["B"], cfg["bands"] // cfg["spectral_patch"], cfg["image_size"] ** 2


def score_ratio(params, cfg, i, x, x_init):
    """r of the lse bar: the largest |score| of this case's float64 restatement (lse_restatement's s, on LN1 rows computed in float64
    from the state's parameters and input) over the same at the init state (gamma = 1, beta = 0, the untransformed input).  The
    reference alone: nothing the kernels wrote enters"""
    B, S, N = shape_of(cfg)
    mode = 0 if i == 0 else 1
    pre = block_prefix(i)
    w = params[pre + "0.fn.to_qkv.weight"]

    def largest(t, g, b):
        xn = torch.nn.functional.layer_norm(t.double().reshape(-1, 96), (96,), g.double(), b.double(), 1e-5).float()
        return lse_restatement(to_seq(xn.reshape(B, S * N, 96), mode, B, S, N), w, cfg["heads"], torch.float16, scores=True)[1]
    return largest(x, params[pre + "0.norm.weight"], params[pre + "0.norm.bias"]) / largest(x_init, torch.ones(96), torch.zeros(96))


def against_bars(tag, r, bars, lse_bar=None):
    bad = [tag + ("bar", q, r[q], bars[q]) for q in Q if not r[q] < bars[q]]
    if lse_bar is not None:
        if not r["lse_abs_err"] < lse_bar:
            bad.append(tag + ("bar", "lse_abs_err", r["lse_abs_err"], lse_bar))
        if not r["rstd_err"] < 1e-5:
            bad.append(tag + ("bar", "rstd_err", r["rstd_err"], 1e-5))
    return bad


def block_case(state, mode, L, prec, heads):
    """model in `state`, block index, the state's input, the init-state input and the output gradient of one shape"""
    cfg = case_cfg(mode, L, heads)
    model, params, eng = make_model(cfg, prec, edit=affine_edit(state))
    if state in AFFINE_STATES:
        assert max_beta_over_gamma(params) <= MAX_RATIO
    i = 0 if mode == 0 else 1
    x_init, dy = block_inputs(cfg, eng.S, eng.N, i)
    return cfg, model, params, eng, i, state_inputs(state, x_init), x_init, dy


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_blocks_teacher_forced(family, state):
    """one block forward (_fwd_block) and backward (block_bwd_single) per shape against oracle.model.block in float64 with the
    kernels' dropout masks: increment, dx - dy, worst parameter gradient; bf16 with 8 heads also the saved lse / rstd.  The six
    families of test_gpu_launch_geometry.py on their bars, unchanged"""
    prec, heads, drop, stats, bars, _ = FAMILIES[family]
    bad = []
    for mode, L in SHAPES:
        cfg, model, params, eng, i, x, x_init, dy = block_case(state, mode, L, prec, heads)
        B, S, N = shape_of(cfg)
        xc = x.cuda()
        y, x1, dx = block_kernels(eng, cfg, i, prec, xc, dy.cuda().contiguous(), drop=drop)   # (asserts eng.fwd_half for bf16, 8 heads)
        ref = block_reference(params, cfg, S, N, i, x, dy, drop=drop)
        r = block_errors(model, eng, i, prec, x, dy, ref, y, dx)
        lse_bar = None
        if stats:
            r["lse_abs_err"], r["rstd_err"] = check_saved_statistics(eng, params, xc, x1, i, mode, B, S, N, cfg["qkv_scale"])
            r["score_ratio"] = score_ratio(params, cfg, i, x, x_init)
            lse_bar = LSE_BARS[cfg["qkv_scale"]] * max(1.0, r["score_ratio"])
        print(family, state, SNAME[mode], L, r)
        bad += against_bars((SNAME[mode], L), r, bars, lse_bar)
        record("trained_state_teacher_forced", family=family, state=state, mode=mode, L=L, cfg=cfg, **r)
        del model, eng
    assert not bad, report(bad)


@pytest.mark.parametrize("state", AFFINE_STATES)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_variants_with_their_own_layernorm(variant, state, monkeypatch):
    """the kernels that carry their own copy of the LayerNorm arithmetic and that the default selection never runs at 8 heads in
    bf16: bf16 operands in the role-split forward (MSST_FWD_HALF=0), fp32 x1 rows (MSST_X1_BF16=0: the backward's LN2 on them), the
    generic templates (MSST_DBG=16), the 4-wave forward (64), the one-head attention backward (128) -- each against the same float64
    reference, and each shown to have run: by what its forward saved, or by bits that differ from the default run's"""
    from maskedsst_amd.engine import _kernel_flags
    env, bars = VARIANTS[variant]
    bad = []
    for mode, L in VARIANT_SHAPES:
        cfg, model, params, eng, i, x, x_init, dy = block_case(state, mode, L, "bf16", 8)
        B, S, N = shape_of(cfg)
        xc, dyc = x.cuda(), dy.cuda().contiguous()
        y0, x10, dx0 = block_kernels(eng, cfg, i, "bf16", xc, dyc)
        g0 = eng.fp.grad.clone()
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        try:
            flags = _kernel_flags() & ~(128 << 8)      # (128 selects a backward kernel; the forward stays the role-split one)
            y, x1, dx = block_kernels(eng, cfg, i, "bf16", xc, dyc, flags=flags, x1_bf16=os.environ.get("MSST_X1_BF16", "1") != "0",
                                      half=os.environ.get("MSST_FWD_HALF", "1") != "0")
        finally:
            for k in env:
                monkeypatch.delenv(k)
        same_fwd = torch.equal(y, y0)
        same_bwd = torch.equal(dx, dx0) and torch.equal(eng.fp.grad, g0)
        if variant == "fwd_half0":      # (block_kernels: eng.fwd_half is off, bf16 x1 rows, statistics)
            assert x1.dtype == torch.bfloat16 and not eng.fwd_half and not same_fwd
        elif variant == "x1_bf16_0":    # the same forward arithmetic, fp32 rows kept, another backward
            assert x1.dtype == torch.float32 and x10.dtype == torch.bfloat16 and x1._msst_lse is not None and same_fwd and not same_bwd
        elif variant == "dbg16":
            assert x1._msst_xn is None and x1._msst_lse is None and not same_fwd and not same_bwd
        elif variant == "dbg64":
            assert x1._msst_xn is not None and x1._msst_lse is None and not same_fwd
        else:
            assert x1.dtype == torch.bfloat16 and same_fwd and not same_bwd
        ref = block_reference(params, cfg, S, N, i, x, dy)
        r = block_errors(model, eng, i, "bf16", x, dy, ref, y, dx)
        print(variant, state, SNAME[mode], L, r)
        bad += against_bars((SNAME[mode], L), r, bars)
        record("trained_state_variant", variant=variant, state=state, mode=mode, L=L, cfg=cfg, **r)
        del model, eng
    assert not bad, report(bad)


@pytest.mark.parametrize("mode,L", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("state", STATES)
def test_production_pair(state, mode, L, monkeypatch):
    """blocks_fwd (the stack launch, bit-identical to the per-block launches) and blocks_bwd on the depth-1 model against float64
    autograd through both blocks: the chained backward with LN1 from the saved rows (the first absolute check of MSST_LN1_FROM_XN
    with gamma != 1 and beta != 0), then with MSST_LN1_XN=0 and with MSST_BWD_CHAIN=0 -- all on BF16_BARS["production"]"""
    from oracle import transformer_forward
    cfg = case_cfg(mode, L, 8)
    model, params, eng = make_model(cfg, "bf16", edit=affine_edit(state))
    assert max_beta_over_gamma(params) <= MAX_RATIO
    B, S, N = cfg["B"], eng.S, eng.N
    x0 = state_inputs(state, tokens_with_offsets(B, S, N, None, seed=3000 + L))
    dy = torch.randn(x0.shape, generator=torch.Generator().manual_seed(4000 + L))
    runs, stacked = {}, []
    real_stack = eng._fwd_stack
    eng._fwd_stack = lambda *a: stacked.append(real_stack(*a)) or stacked[-1]
    for flag in ("1", "0"):
        monkeypatch.setenv("MSST_FWD_STACK", flag)
        stacked.clear()
        acts, x1s = eng.blocks_fwd(x0.cuda(), save=True)
        runs[flag] = (acts, x1s, list(stacked))
    monkeypatch.delenv("MSST_FWD_STACK")
    del eng._fwd_stack
    (a1, s1, l1), (a0, s0, l0) = runs["1"], runs["0"]
    assert l1 == [True, True] and l0 == [] and eng.fwd_half, (l1, l0)
    for j in (1, 2):
        assert torch.equal(a1[j], a0[j]), ("stacked forward differs", j)
    for t1, t0 in zip(s1, s0):
        assert torch.equal(t1, t0) and torch.equal(t1._msst_xn, t0._msst_xn) and torch.equal(t1._msst_lse, t0._msst_lse)
    p64 = {k: v.double().requires_grad_(True) for k, v in params.items() if "spatial_spectral_transformer" in k}
    xs = x0.double().requires_grad_(True)
    y64 = transformer_forward(p64, xs, oracle_cfg(cfg))
    y64.backward(dy.double())
    inc_err = rel_l2(a1[2].double().cpu() - x0.double(), y64.detach() - x0.double())
    flat = {id(p): n for n, p in eng.trainable()}
    names = {pn: flat[id(p)] for pn, p in model.named_parameters() if pn in p64}
    calls = []
    for form in ("_blocks_bwd_chained", "_blocks_bwd_unchained"):
        setattr(eng, form, (lambda real, form: lambda *a: calls.append(form) or real(*a))(getattr(eng, form), form))
    bad, got = [], {}
    for tag, env in BACKWARDS.items():
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        calls.clear()
        try:
            eng.fp.grad.zero_()
            dx0 = eng.blocks_bwd(a1, s1, dy.cuda())      # (a fresh copy each time: the unchained loop writes into it)
            torch.cuda.synchronize()
        finally:
            for k in env:
                monkeypatch.delenv(k)
        # the form under test ran
        assert calls == ["_blocks_bwd_unchained" if tag == "chain0" else "_blocks_bwd_chained"], (tag, calls)
        assert eng.last_bwd_ln1_from_xn == (tag == "default"), tag
        got[tag] = (dx0.clone(), eng.fp.grad.clone())
        if tag != "default":
            assert not torch.equal(got[tag][0], got["default"][0]), (tag, "the bits of the default backward")
        ge = {pn: rel_l2(eng.fp.view(nm, eng.fp.grad), p64[pn].grad) for pn, nm in names.items()}
        worst = max(ge, key=ge.get)
        r = dict(inc_err=inc_err, dx=rel_l2(dx0.double().cpu() - dy.double(), xs.grad - dy.double()), worst_grad=ge[worst],
                 worst_grad_name=worst)
        print("production", state, SNAME[mode], L, tag, r)
        bad += against_bars((tag,), r, BF16_BARS["production"])
        record("trained_state_production", backward=tag, state=state, mode=mode, L=L, cfg=cfg, **r)
    assert not bad, report(bad)


def test_whole_step_fp32():
    """one SimMIM step in fp32 with EVERY parameter off its initial value (the blocks' recipe for the tokenizer's two LayerNorms
    and for the embedding and to_pixels biases; noise on the position table and the mask token): loss and every gradient against
    oracle.simmim_forward in float64 at the tolerances of test_gpu_backward.py::test_param_grads_fp32"""
    from oracle import simmim_forward
    cfg = dict(bands=50, depth=2, B=4)
    model, params, x = build_product(cfg, precision="fp32", device="cuda")
    wrote = make_affine(model, params, everything=True)
    for part in ("pre_norm.weight", "post_norm.bias", "blockwise_embed.0.bias", "pos_embedding", "mask_token", "to_pixels.layers.0.bias",
                 "1.layers.0.0.norm.weight", "3.layers.1.1.norm.bias", "3.layers.1.1.fn.net.3.bias"):
        assert any(part in n for n in wrote), part
    for n, p in model.named_parameters():
        assert torch.equal(p.detach().cpu(), params[n]), n
    masks = model.draw_masks(cfg["B"])
    p64 = {k: v.double().requires_grad_(True) for k, v in params.items()}
    ref = simmim_forward(p64, x.double(), oracle_cfg_from(cfg), masks=masks)
    ref["loss"].backward()
    loss = model(x.cuda(), masks=masks)
    loss.backward()
    torch.cuda.synchronize()
    lr = ref["loss"].item()
    loss_err = abs(loss.item() - lr) / abs(lr)
    errs = {}
    for name, p in model.named_parameters():
        g_ref = p64[name].grad
        if g_ref is None:
            assert p.grad is None, name
            continue
        assert p.grad is not None, name
        errs[name] = relerr(p.grad, g_ref)
    worst = max(errs, key=errs.get)
    print("step fp32", loss_err, worst, errs[worst])
    record("trained_state_step_fp32", cfg=cfg, loss_err=loss_err, worst_grad=errs[worst], worst_grad_name=worst)
    assert abs(loss.item() - lr) <= 1e-4 * abs(lr) + 1e-7, (loss.item(), lr)
    bad = [(n, e) for n, e in errs.items() if not e < 2e-4]
    assert not bad, bad
