"""The block kernels at every attention sequence length L from 1 to 64, teacher-forced against float64.

The kernels are specialised on L (spatial blocks: L = N pixels, spectral blocks: L = S spectral tokens): a 64-row tile packs
TS = 64 // L whole sequences and pads the rest, the role-split forward builds a per-row key mask and skips score tiles outside a
band, the two-head attention backward derives the key tiles each wave needs from the row map, and the saved softmax statistics
and the attention-dropout hash are addressed by (tile, head, row).  Every case here builds a depth-1 model (one spatial and one
spectral block, as tests/util.py:build_product does), hands one block's kernels and oracle.model.block on float64 copies of the
parameters the same input x and the same output gradient dy, and compares

  * the block's increment y - x (the residual would hide an attention error of a few percent),
  * the increment of the input gradient dx - dy,
  * every parameter gradient of the block.

Inputs make a leak visible: every token of a sequence carries the same random offset (at the scale of the token noise), so a key
or value read from a neighbouring sequence or a padding row moves the increment far past the bars.  Half the cases use peaky rows
(to_qkv.weight x4, the qkv_scale convention of the depth-12 fixtures): spectral lengths with L // 2 odd, spatial sides that are odd.

Bars: fp32 -- the teacher-forced bars of tests/test_gpu_depth12.py (max-norm relative error 1e-4 forward, 2e-4 backward);
bf16 -- relative L2 at ~3.5x the worst value measured over the sweep; the saved lse -- 3.5x the worst absolute error measured, per
qkv scale.  And per (family, block, quantity, qkv scale) no length may sit more than 3x above the median over the lengths (no
additive floor; measured: at most 1.9x): a bug at one length shows up as an outlier even under a loose bar.  Every error goes to
util.record, under names the strict parity tier compares (inc_err, dx, worst_grad, lse_abs_err, rstd_err); the committed baseline
rows are profiles/r06_seq_lengths_parity_measured.jsonl.  The whole file runs in about 10 s on one MI355X (9.4 s measured).

Worst errors measured on MI355X (relative L2 for bf16, max-norm relative for fp32; increment / dx - dy / worst parameter gradient):
  bf16, 8 heads, spectral     7.7e-4 (L 38)         1.34e-2 (L 51)            1.45e-2 (L 50)
  bf16, 8 heads, spatial      7.8e-4 (L 49)         1.32e-2 (L 49)            1.19e-2 (L 49)
  bf16, 8 heads, dropout 0.1  8.2e-4 (spatial 49)   1.32e-2 (spatial 49)      1.23e-2 (spectral 31)
  bf16, 2 / 3 heads           6.3e-3 (spatial 49)   1.40e-2 (spectral 31)     1.44e-2 (spatial 9)
  bf16, production backward   1.16e-3 (spectral 51) 1.70e-2 (spectral 51)     1.95e-2 (spectral 26)
  fp32, 8 heads               1.4e-6 (spectral 54)  1.8e-6 (spectral 6)       1.9e-6 (spectral 31)
  fp32, 2 / 3 heads           1.3e-6 (spatial 49)   2.1e-6 (spatial 49)       1.6e-6 (spatial 49)
  1 and 16 heads (spectral 22, 33, spatial 25): bf16 5.8e-3 / 1.23e-2 / 1.13e-2, fp32 1.6e-6 / 1.4e-6 / 1.4e-6
  saved statistics (bf16, 8 heads): lse 3.5e-4 absolute on plain rows (spectral 1), 6.4e-3 on peaky rows (spectral 58); rstd 1.7e-7
Mutations this file catches, each applied alone to the kernels: the lengths at which test_bf16_8_heads_every_length fails (the
production sweeps fail at the same lengths or more -- each of their models also runs a short spatial or spectral block):
  key mask one key longer (msst_fwd3.hip)            spectral L 1 - 62, spatial 1 - 49 (no-op at L >= 63); lse off by up to 38
  `band` without the row-map check (msst_fwd3.hip)   spectral L 25 - 31 and 33 - 63, spatial 25, 36, 49 (the band holds at L <= 21 and
                                                     32); increment up to 0.41
  `khi` one key short (msst_bwd4.hip)                spectral L 3, 7, 11, 17, 33, 49, spatial 49 (sequences ending on a tile's first key);
                                                     dx - dy up to 0.17
  `kvalid` one key wider (msst_bwd4.hip)             46 of the 64 spectral lengths, spatial 1, 4, 9, 25, 49; dx - dy up to 1.6
"""
import numpy as np
import pytest
import torch

from util import build_product, oracle_cfg, relerr, rel_l2, record, ln1_rows_as_used, lse_restatement, saved_lse_rows

pytestmark = pytest.mark.gpu

SPECTRAL_L = list(range(1, 65))
BOUNDARY_L = [1, 2, 3, 4, 5, 15, 16, 17, 21, 22, 31, 32, 33, 48, 49, 63, 64]
SIDES = [1, 2, 3, 4, 5, 6, 7, 8]          # spatial blocks: L = side^2
SPATIAL_S = 5                              # odd: spatial tiles with TS > 1 end partly filled
OTHER_P = {40: 5, 50: 4}                   # 200 bands at band_patch_size 5 / 4; every other S: P = 10
DROP = (0.1, 4242)
OUTLIER = 3.0
Q = ("inc_err", "dx", "worst_grad")        # increment y - x, dx - dy, worst parameter-gradient tensor

# bf16 bars (relative L2), 3.5x the worst value measured on MI355X over the sweep (worst: block, L)
BF16_BARS = {
    # role-split forward (half operands) + two-head backward on saved statistics, with and without dropout 0.1:
    # 8.2e-4 (spatial 49, dropout), 1.34e-2 (spectral 51), 1.45e-2 (spectral 50)
    8: dict(inc_err=2.9e-3, dx=4.7e-2, worst_grad=5.1e-2),
    # 4-wave forward (bf16 operands) + two-head (2, 16) or one-head (1, 3) backward: 6.3e-3 (spatial 49, 3 heads), 1.40e-2 (spectral 31,
    # 2 heads), 1.44e-2 (spatial 9, 2 heads)
    "4wave": dict(inc_err=2.2e-2, dx=4.9e-2, worst_grad=5.1e-2),
    # blocks_fwd + chained blocks_bwd through both blocks: 1.16e-3 (spectral 51), 1.70e-2 (spectral 51), 1.95e-2 (spectral 26)
    "production": dict(inc_err=4.1e-3, dx=6e-2, worst_grad=6.8e-2),
}
FP32_BARS = dict(inc_err=1e-4, dx=2e-4, worst_grad=2e-4)
# saved lse, absolute, per qkv scale: 3.5x the worst measured -- 3.5e-4 on plain rows (spectral 1), 6.4e-3 on peaky ones (spectral 58)
LSE_BARS = {1: 1.2e-3, 4: 2.3e-2}


def qkv_scale_of(L):
    return 4 if (L // 2) % 2 else 1        # decorrelated from the parity of L (which picks N) -- half the lengths peaky


def pick_B(per_b, L, tokens_per_b, partial=True, min_tokens=256, min_tiles=2):
    """batch: at least min_tiles attention tiles (64 // L whole sequences each) and min_tiles 64-row tiles of the row-local kernels,
    >= min_tokens tokens and (partial) the last attention tile partly filled whenever a tile holds more than one sequence.  (The
    defaults ask for two attention tiles; their 256 tokens are four row tiles.)"""
    TS = 64 // L
    assert not (partial and TS > 1 and per_b % TS == 0), (per_b, L)   # every batch would fill its last tile
    B = 1
    while not (-(-(B * per_b) // TS) >= min_tiles and -(-(B * tokens_per_b) // 64) >= min_tiles
               and (not partial or TS == 1 or (B * per_b) % TS) and B * tokens_per_b >= min_tokens):
        B += 1
    return B


def spectral_cfg(S, heads, partial=True, **size):
    """N = 4 (sequence bases by shift) for even S, N = 9 (by division) for odd S -- unless N sequences fill whole tiles
    (TS = 2: no power of two can end partly filled; TS = 3, 4, 9): then the other one.  size: pick_B's min_tokens / min_tiles"""
    P = OTHER_P.get(S, 10)
    TS = 64 // S
    N = 4 if S % 2 == 0 else 9
    if partial and TS > 1 and N % TS == 0:
        N = 13 - N
    side = int(round(N ** 0.5))
    B = pick_B(N, S, S * N, partial, **size)
    return dict(bands=P * S, spectral_patch=P, image_size=side, depth=1, B=B, heads=heads, mask_patch_size=1,
                qkv_scale=qkv_scale_of(S))


def spatial_cfg(side, heads, **size):
    """peaky rows at the odd sides (1, 3, 5, 7), plain ones at the even sides"""
    N = side * side
    B = pick_B(SPATIAL_S, N, SPATIAL_S * N, **size)
    return dict(bands=10 * SPATIAL_S, spectral_patch=10, image_size=side, depth=1, B=B, heads=heads, mask_patch_size=1,
                qkv_scale=4 if side % 2 else 1)


def case_cfg(mode, L, heads, partial=True, **size):
    return spatial_cfg(int(round(L ** 0.5)), heads, **size) if mode == 0 else spectral_cfg(L, heads, partial, **size)


def tokens_with_offsets(B, S, N, mode, seed):
    """[B, S N, 96] tokens (order b (c h w)): unit noise + one random offset per sequence of `mode` (None: both kinds)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, S, N, 96, generator=g)
    if mode in (0, None):
        x = x + torch.randn(B, S, 1, 96, generator=g)      # spatial sequences (b, c)
    if mode in (1, None):
        x = x + torch.randn(B, 1, N, 96, generator=g)      # spectral sequences (b, n)
    return x.reshape(B, S * N, 96).contiguous()


def to_seq(t, mode, B, S, N):
    return t.reshape(B * S, N, 96) if mode == 0 else t.reshape(B, S, N, 96).transpose(1, 2).reshape(B * N, S, 96)


def from_seq(t, mode, B, S, N):
    return t.reshape(B, S * N, 96) if mode == 0 else t.reshape(B, N, S, 96).transpose(1, 2).reshape(B, S * N, 96)


def make_model(cfg, prec, edit=None):
    """edit(model, params): changes the parameters (the model's and the oracle's copies alike) before the engine exists"""
    from maskedsst_amd.engine import _kernel_flags
    # the families here are chosen by precision and head count alone: a kernel-selection override (MSST_DBG) would swap the
    # kernels under test for others -- refuse to run rather than check the wrong path
    assert _kernel_flags() == 0, "MSST_DBG selects kernels other than the families these tests name"
    model, params, _ = build_product(cfg, precision=prec, device="cuda")
    if edit is not None:
        edit(model, params)
    eng = model.engine()
    eng.prep_weights()
    return model, params, eng


def block_prefix(i):
    return f"encoder.spatial_spectral_transformer.{'1' if i == 0 else '3'}.layers.0."


def check_saved_statistics(eng, params, x, x1, i, mode, B, S, N, qkv_scale):
    """the saved per-row lse (padding rows skipped) and the rstd tail against the restatement shared with
    tests/test_gpu_backward.py::test_saved_softmax_statistics -> (lse abs error, rstd rel error)"""
    H = eng.enc.heads
    L = N if mode == 0 else S
    nseq = B * S if mode == 0 else B * N
    lse = x1._msst_lse
    assert lse.numel() == -(-nseq // (64 // L)) * H * 64 + B * S * N
    pre = block_prefix(i)
    xn, low = ln1_rows_as_used(x, params[pre + "0.norm.weight"].cuda(), params[pre + "0.norm.bias"].cuda(), x1, eng.fwd_half)
    ref = lse_restatement(to_seq(xn, mode, B, S, N), params[pre + "0.fn.to_qkv.weight"].cuda(), H, low)
    got, rstd = saved_lse_rows(lse, H, L, nseq)
    e_lse = float((got.double() - ref).abs().max())
    rstd_ref = torch.rsqrt(x.double().reshape(-1, 96).var(dim=-1, unbiased=False) + 1e-5)
    e_rstd = float(((rstd.double() - rstd_ref).abs() / rstd_ref).max())
    return e_lse, e_rstd


def block_inputs(cfg, S, N, i):
    """block i's input x (offsets per sequence of its mode) and output gradient dy, on the host"""
    x = tokens_with_offsets(cfg["B"], S, N, 0 if i == 0 else 1, seed=1000 + i)
    dy = torch.randn(x.shape, generator=torch.Generator().manual_seed(2000 + i))
    return x, dy


def block_reference(params, cfg, S, N, i, x, dy, drop=None, dtype=torch.float64):
    """oracle.model.block on float64 copies of block i's parameters, with the kernels' dropout masks -> the increment y - x, dx - dy
    (token order of x) and the parameter gradients by name.  dtype: the arithmetic of the oracle (float32: tests/test_trained_state_host.py)"""
    import oracle.model as om
    from dropout import block_masks
    B, H = cfg["B"], cfg["heads"]
    mode = 0 if i == 0 else 1
    drop = drop or (0.0, 0)
    pre = block_prefix(i)
    p64 = {k: v.to(dtype).requires_grad_(True) for k, v in params.items() if k.startswith(pre)}
    xs = to_seq(x.to(dtype), mode, B, S, N).requires_grad_(True)
    masks = None
    if drop[0]:
        masks = {k: v.to(dtype) for k, v in block_masks(drop[0], drop[1], i, mode, B, S, N, H).items()}
    y = om.block(xs, p64, pre, H, masks)
    y.backward(to_seq(dy.to(dtype), mode, B, S, N))
    return dict(inc=from_seq(y.detach(), mode, B, S, N) - x.to(dtype), dxi=from_seq(xs.grad, mode, B, S, N) - dy.to(dtype),
                grads={k: v.grad for k, v in p64.items()})


def block_kernels(eng, cfg, i, prec, xc, dyc, drop=None, ws=None, flags=0, x1_bf16=None, want_lse=None, half=True):
    """block i's forward (_fwd_block, saving) and backward (block_bwd_single, its parameter gradients into the zeroed flat buffer)
    on device tensors -> (y, x1, dx); asserts that the family's kernels ran.  flags: the forward's kernel-selection flags
    (engine._kernel_flags(); the backward reads MSST_DBG itself); x1_bf16 / want_lse: what the role-split forward saves (default:
    bf16 x1 rows and the statistics, as blocks_fwd asks for); half: whether its operands are expected to be IEEE half"""
    drop = drop or (0.0, 0)
    bf = prec == "bf16"
    role_split = bf and cfg["heads"] == 8 and flags == 0
    x1_bf16 = role_split if x1_bf16 is None else (role_split and x1_bf16)
    want_lse = role_split if want_lse is None else (role_split and want_lse)
    acts, x1s = [xc], []
    eng._fwd_block(acts, x1s, i, True, drop, x1_bf16, want_lse, flags)
    x1 = x1s[0]
    # the path under test ran: role-split forward (bf16 x1 rows, saved statistics, half operands), 4-wave forward (saved LN1 rows,
    # no statistics), template forward (fp32, or bf16 under MSST_KERNEL_GENERIC: neither)
    if role_split:
        assert x1.dtype == (torch.bfloat16 if x1_bf16 else torch.float32) and (x1._msst_lse is not None) == want_lse
        assert x1._msst_xn is not None and bool(eng.fwd_half) == half
    elif bf and not flags & (16 << 8):
        assert x1.dtype == torch.float32 and x1._msst_xn is not None and x1._msst_lse is None
    else:
        assert x1.dtype == torch.float32 and x1._msst_xn is None and x1._msst_lse is None
    eng.fp.grad.zero_()
    dx = eng.block_bwd_single(i, xc, x1, dyc, drop=drop, ws=ws)
    torch.cuda.synchronize()
    return acts[1], x1, dx


def block_errors(model, eng, i, prec, x, dy, ref, y, dx):
    """the kernels' y, dx and flat-buffer gradients of block i against block_reference's -> dict of errors"""
    pre = block_prefix(i)
    err = rel_l2 if prec == "bf16" else relerr
    out = dict(inc_err=err(y.double().cpu() - x.double(), ref["inc"]), dx=err(dx.double().cpu() - dy.double(), ref["dxi"]))
    flat = {id(p): n for n, p in eng.trainable()}
    worst, worst_name = 0.0, ""
    for pname, p in model.named_parameters():
        if pname.startswith(pre):
            e = err(eng.fp.view(flat[id(p)], eng.fp.grad), ref["grads"][pname])
            if e > worst:
                worst, worst_name = e, pname[len(pre):]
    out.update(worst_grad=worst, worst_grad_name=worst_name)
    return out


def run_block(model, params, eng, cfg, i, prec, drop=None, stats=False):
    """block i of the depth-1 model: kernels vs float64 autograd on the same x and dy -> dict of errors"""
    S, N = eng.S, eng.N
    x, dy = block_inputs(cfg, S, N, i)
    xc = x.cuda()
    y, x1, dx = block_kernels(eng, cfg, i, prec, xc, dy.cuda().contiguous(), drop=drop)
    ref = block_reference(params, cfg, S, N, i, x, dy, drop=drop)
    out = block_errors(model, eng, i, prec, x, dy, ref, y, dx)
    if stats:
        out["lse_abs_err"], out["rstd_err"] = check_saved_statistics(eng, params, xc, x1, i, 0 if i == 0 else 1, cfg["B"], S, N,
                                                                     cfg["qkv_scale"])
    return out


def sweep(cases, prec, heads, drop=None, stats=False, family=None):
    """cases: [(mode, L)] -> {(mode, L): (qkv scale, errors)}; records one row per case"""
    res = {}
    for mode, L in cases:
        cfg = case_cfg(mode, L, heads)
        model, params, eng = make_model(cfg, prec)
        r = run_block(model, params, eng, cfg, 0 if mode == 0 else 1, prec, drop=drop, stats=stats)
        res[(mode, L)] = (cfg["qkv_scale"], r)
        record("seq_lengths_teacher_forced", family=family, mode=mode, L=L, cfg=cfg, **r)
        del model, eng
    return res


def assert_sweep(res, bars):
    bad = []
    for (mode, L), (sc, r) in res.items():
        for q in Q:
            if not r[q] < bars[q]:
                bad.append(("bar", mode, L, q, r[q], bars[q]))
        if "lse_abs_err" in r:
            if not r["lse_abs_err"] < LSE_BARS[sc]:
                bad.append(("bar", mode, L, "lse_abs_err", r["lse_abs_err"], LSE_BARS[sc]))
            if not r["rstd_err"] < 1e-5:
                bad.append(("bar", mode, L, "rstd_err", r["rstd_err"], 1e-5))
    # outliers: per (block, quantity, qkv scale), no length more than 3x the median over the lengths
    for mode in (0, 1):
        for scale in (1, 4):
            keys = [k for k, (sc, _) in res.items() if k[0] == mode and sc == scale]
            if len(keys) < 3:
                continue
            for q in Q:
                med = float(np.median([res[k][1][q] for k in keys]))
                for k in keys:
                    if res[k][1][q] > OUTLIER * med:
                        bad.append(("outlier", mode, k[1], q, res[k][1][q], med))
    assert not bad, bad


SPECTRAL = [(1, L) for L in SPECTRAL_L]
SPATIAL = [(0, s * s) for s in SIDES]
BOUNDARY = [(1, L) for L in BOUNDARY_L]


@pytest.mark.parametrize("mode", [1, 0], ids=["spectral", "spatial"])
def test_bf16_8_heads_every_length(mode):
    """The benchmarked path: role-split forward with half operands, saved LN1 rows, bf16 x1 rows and softmax statistics, two-head
    attention backward on the saved statistics -- at every L, plus the saved lse / rstd against their restatements."""
    res = sweep(SPECTRAL if mode == 1 else SPATIAL, "bf16", 8, stats=True, family="bf16_h8")
    assert_sweep(res, BF16_BARS[8])


@pytest.mark.parametrize("mode", [1, 0], ids=["spectral", "spatial"])
def test_fp32_8_heads_every_length(mode):
    """The fp32 template kernels at every L, on the teacher-forced fp32 bars"""
    res = sweep(SPECTRAL if mode == 1 else SPATIAL, "fp32", 8, family="fp32_h8")
    assert_sweep(res, FP32_BARS)


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("heads", [2, 3])
def test_other_head_counts_boundary_lengths(heads, prec):
    """2 heads (4-wave forward, tuned two-head backward) and 3 heads (4-wave forward, one-head backward) in bf16; the fp32 templates
    at both -- at the lengths where the tile packing changes, and at every spatial side"""
    res = sweep(BOUNDARY + SPATIAL, prec, heads, family=f"{prec}_h{heads}")
    assert_sweep(res, BF16_BARS["4wave"] if prec == "bf16" else FP32_BARS)


def test_bf16_8_heads_dropout_boundary_lengths():
    """attention / projection / MLP dropout 0.1 at the boundary lengths and every spatial side; the kernels' masks are fed to the
    oracle through tests/dropout.block_masks, which restates the (tile, head, row, key) addressing of the attention mask"""
    res = sweep(BOUNDARY + SPATIAL, "bf16", 8, drop=DROP, family="bf16_h8_drop0.1")
    assert_sweep(res, BF16_BARS[8])


def production_case(mode_L, monkeypatch):
    """blocks_fwd + blocks_bwd on the depth-1 model (chained backward, LN1 from the saved rows) against float64 autograd through
    both blocks; the stacked and the per-block forward bit-identical -> (qkv scale, errors)"""
    from oracle import transformer_forward
    mode, L = mode_L
    # (spectral: N by the parity of L alone, so that L = 22 .. 32 also run the shift path -- with full tiles)
    cfg = case_cfg(mode, L, 8, partial=False)
    model, params, eng = make_model(cfg, "bf16")
    B, S, N = cfg["B"], eng.S, eng.N
    x0 = tokens_with_offsets(B, S, N, None, seed=3000 + L)
    dy = torch.randn(x0.shape, generator=torch.Generator().manual_seed(4000 + L))
    runs = {}
    stacked = []
    real_stack = eng._fwd_stack
    eng._fwd_stack = lambda *a: stacked.append(real_stack(*a)) or stacked[-1]
    for flag in ("1", "0"):
        monkeypatch.setenv("MSST_FWD_STACK", flag)
        stacked.clear()
        acts, x1s = eng.blocks_fwd(x0.cuda(), save=True)
        runs[flag] = (acts, x1s, list(stacked))
    monkeypatch.delenv("MSST_FWD_STACK")
    (a1, s1, l1), (a0, s0, l0) = runs["1"], runs["0"]
    assert l1 == [True, True] and l0 == [], (l1, l0)     # both stacks through msst_block_fwd_stack, then both per block
    for j in (1, 2):
        assert torch.equal(a1[j], a0[j]), ("stacked forward differs", j)
    for t1, t0 in zip(s1, s0):
        assert torch.equal(t1, t0) and torch.equal(t1._msst_xn, t0._msst_xn) and torch.equal(t1._msst_lse, t0._msst_lse)
    eng.fp.grad.zero_()
    dx0 = eng.blocks_bwd(a1, s1, dy.cuda())
    torch.cuda.synchronize()
    assert eng.last_bwd_ln1_from_xn
    p64 = {k: v.double().requires_grad_(True) for k, v in params.items() if "spatial_spectral_transformer" in k}
    xs = x0.double().requires_grad_(True)
    y = transformer_forward(p64, xs, oracle_cfg(cfg))
    y.backward(dy.double())
    flat = {id(p): n for n, p in eng.trainable()}
    ge = {pn: rel_l2(eng.fp.view(flat[id(p)], eng.fp.grad), p64[pn].grad) for pn, p in model.named_parameters() if pn in p64}
    worst = max(ge, key=ge.get)
    r = dict(inc_err=rel_l2(a1[2].double().cpu() - x0.double(), y.detach() - x0.double()),
             dx=rel_l2(dx0.double().cpu() - dy.double(), xs.grad - dy.double()), worst_grad=ge[worst], worst_grad_name=worst)
    record("seq_lengths_production", mode=mode, L=L, cfg=cfg, **r)
    return cfg["qkv_scale"], r


@pytest.mark.parametrize("mode", [1, 0], ids=["spectral", "spatial"])
def test_bf16_production_backward_every_length(mode, monkeypatch):
    """the forward / backward pair bench.py times, per L: stacked role-split forward (bit-identical to per-block launches), chained
    backward with MSST_LN1_FROM_XN, dx0 and every block parameter gradient against float64 autograd through both blocks"""
    res = {}
    for case in (SPECTRAL if mode == 1 else SPATIAL):
        res[case] = production_case(case, monkeypatch)
    assert_sweep(res, BF16_BARS["production"])


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("heads", [1, 16])
def test_heads_1_and_16(heads, prec):
    """head counts the constructor accepts that nothing else runs: two spectral lengths (33: one sequence and padding per tile;
    22: two sequences per tile, the last one partly filled) and one spatial side (25 pixels: two sequences per tile).  Both match
    the oracle, so neither is refused."""
    res = sweep([(1, 33), (1, 22), (0, 25)], prec, heads, family=f"{prec}_h{heads}")
    bars = BF16_BARS["4wave"] if prec == "bf16" else FP32_BARS
    bad = [(k, q, r[q]) for k, (_, r) in res.items() for q in Q if not r[q] < bars[q]]
    assert not bad, bad
