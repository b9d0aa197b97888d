"""GPU: SimMIM pre-training on windows read from resident tiles.  The three entry points msst_tokenize_at_fwd_masked,
msst_tokenize_at_bwd_masked and msst_head_at_fwd through the C ABI with ctypes, bit for bit against msst_tokenize_fwd / msst_tokenize_bwd /
msst_head_fwd on the stacked copy of the listed windows (the head also against a float64 restatement, at the bar
tests/test_gpu_tok_head_kernels.py holds msst_head_fwd to); SimMIMSpatialSpectral.forward_at / forward_windows bit for bit against
forward(stacked windows, masks) with its backward, both precisions, dropout on; against the oracle at the bars of
tests/test_gpu_forward.py::test_forward_stages; three AdamW steps; and pretrain.py --resident-tiles against the default loader."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import ROOT, seed_all
from util import oracle_cfg, rel_l2

pytestmark = pytest.mark.gpu

D = 96
BADARG, UNSUPPORTED = -3, -2   # include/msst.h: MSST_ERR_BADARG, MSST_ERR_UNSUPPORTED
BAR, BAND = 2e-5, 1e-4         # tests/tok_head_util.py: the head's bar against float64, and the band inside which a sign may differ
# tests/test_gpu_forward_at.py::KERNEL_CASES restated: (name, P, S, window, stride, Bs, Hs, Ws, pos_split); P = 10 and window 8 run the
# fp32-MFMA tokenizer kernels, everything else the generic ones; pos_split != 0: the two-table position form
KERNEL_CASES = [
    ("fast_learned", 10, 2, 8, 8, 2, 16, 16, 0),
    ("fast_split", 10, 2, 8, 8, 2, 16, 16, 64),
    ("w7_cutoff2", 10, 2, 7, 7, 2, 16, 16, 0),
    ("w7_cutoff2_split", 10, 2, 7, 7, 2, 16, 16, 48),
    ("w4_9x13", 10, 2, 4, 4, 2, 9, 13, 0),
    ("w4_stride3", 10, 2, 4, 3, 1, 9, 13, 0),
    ("P5", 5, 3, 8, 8, 2, 16, 16, 0),
    ("P16_w4", 16, 2, 4, 4, 2, 9, 13, 32),
]
IDS = [c[0] for c in KERNEL_CASES]
FULL, EMPTY = 3, 7   # rows of the table whose window is masked entirely / not at all


def _V(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def listed_origins(Bs, Hs, Ws, window):
    """tests/test_gpu_forward_at.py::listed_origins restated: 13 rows (scene, y0, x0), built from the shapes alone: the first window of
    the first scene, the last window of the last scene (the last row and column a window may touch), exact duplicates of both, windows
    one pixel apart in x and in y, every corner, and the scenes interleaved out of order"""
    my, mx, last = Hs - window, Ws - window, Bs - 1
    assert my >= 3 and mx >= 3
    rows = [(0, 0, 0), (last, my, mx), (0, my // 2, mx // 2), (0, my // 2, mx // 2 + 1), (last, my // 2 + 1, mx // 2), (0, 0, 0),
            (last, 0, mx), (0, my, 0), (last, 1, 1), (0, my - 1, mx - 1), (last, my, mx), (0, 3 % (my + 1), 5 % (mx + 1)), (last, 2, 0)]
    assert all(0 <= s < Bs and 0 <= y <= my and 0 <= x <= mx for s, y, x in rows)
    return torch.tensor(rows, dtype=torch.int32)


def stack_at(scene, origins, window):
    return torch.stack([scene[s, :, y:y + window, x:x + window] for s, y, x in origins.tolist()]).contiguous()


def _same(a, b):
    """bitwise equal and free of the NaN prefill"""
    return a is b is None or (torch.equal(a, b) and bool(torch.isfinite(a).all()))


def _kernel_inputs(P, S, window, Bs, Hs, Ws, split):
    gen = torch.Generator(device="cuda").manual_seed(1000 * P + 10 * window + split)
    r = lambda *shape: torch.randn(*shape, device="cuda", generator=gen)   # noqa: E731
    N = window * window
    w = dict(pre_g=1 + 0.3 * r(P), pre_b=0.2 * r(P), w_emb=0.4 * r(S, D, P), b_emb=0.1 * r(S, D), post_g=1 + 0.3 * r(D), post_b=0.2 * r(D),
             mask_token=r(D))
    if split:
        w["pos_a"], w["pos_b"] = r(N, split), r(S, D - split)
    else:
        w["pos_a"], w["pos_b"] = r(S * N, D), None
    scene = r(Bs, S * P, Hs, Ws)
    mask = (torch.rand(13, S * N, device="cuda", generator=gen) < 0.7).to(torch.uint8)   # window coordinates, 1 = masked
    mask[FULL], mask[EMPTY] = 1, 0
    return w, scene, mask.contiguous()


def _tok_args(w):
    return [_V(w[k]) for k in ("pre_g", "pre_b", "w_emb", "b_emb", "post_g", "post_b")]


def _tok_fwd(lib, w, img, mask, split):
    B, C, win, _ = img.shape
    P = w["pre_g"].numel()
    S, N = C // P, win * win
    out = _nan(B, S * N, D)
    rc = lib.msst_tokenize_fwd(_V(img), *_tok_args(w), _V(w["pos_a"]), _V(w["pos_b"]), split, _V(w["mask_token"]), _V(mask), _V(out),
                               B, S, N, P, 0.0, 0, _stream())
    assert rc == 0
    return out


def _tok_at_fwd_masked(lib, w, scene, origins, mask, window, split, out=None, bad=None):
    Bs, C, Hs, Ws = scene.shape
    P = w["pre_g"].numel()
    S, N, nwin = C // P, window * window, origins.shape[0]
    assert origins.is_cuda and origins.dtype == torch.int32 and origins.is_contiguous() and mask.shape == (nwin, S * N)
    out = _nan(nwin, S * N, D) if out is None else out
    bad = bad or {}
    rc = lib.msst_tokenize_at_fwd_masked(_V(scene), _V(bad.get("table", origins)), *_tok_args(w), _V(w["pos_a"]), _V(w["pos_b"]), split,
                                         _V(w["mask_token"]), _V(mask), _V(out), Bs, Hs, Ws, bad.get("window", window),
                                         bad.get("nwin", nwin), S, bad.get("P", P), _stream())
    if bad:
        return rc, out
    assert rc == 0, rc
    return out


def _grad_bufs(P, S, N, split):
    g = dict(dpre_g=_nan(P), dpre_b=_nan(P), dw_emb=_nan(S, D, P), db_emb=_nan(S, D), dpost_g=_nan(D), dpost_b=_nan(D), dmask_token=_nan(D))
    g["dpos_a"], g["dpos_b"] = (_nan(N, split), _nan(S, D - split)) if split else (_nan(S * N, D), None)
    return g


def _grad_args(g):
    return [_V(g[k]) for k in ("dpre_g", "dpre_b", "dw_emb", "db_emb", "dpost_g", "dpost_b", "dpos_a", "dpos_b")]


def _slab(P, S, N, nchunk):
    return _nan(S * nchunk * (N * D + D * P + 4 * D + 32) + S * N * D)


def _tok_bwd(lib, w, img, mask, dx0, nchunk, split):
    B, C, win, _ = img.shape
    P = w["pre_g"].numel()
    S, N = C // P, win * win
    g = _grad_bufs(P, S, N, split)
    rc = lib.msst_tokenize_bwd(_V(img), *_tok_args(w), _V(mask), _V(dx0), _V(_slab(P, S, N, nchunk)), nchunk, *_grad_args(g), split,
                               _V(g["dmask_token"]), B, S, N, P, 0.0, 0, _stream())
    assert rc == 0
    return g


def _tok_at_bwd_masked(lib, w, scene, origins, mask, window, dx0, nchunk, split, g=None, bad=None):
    Bs, C, Hs, Ws = scene.shape
    P = w["pre_g"].numel()
    S, N, nwin = C // P, window * window, origins.shape[0]
    assert origins.is_cuda and origins.dtype == torch.int32 and origins.is_contiguous() and dx0.shape[0] == nwin == mask.shape[0]
    g = _grad_bufs(P, S, N, split) if g is None else g
    bad = bad or {}
    rc = lib.msst_tokenize_at_bwd_masked(_V(scene), _V(bad.get("table", origins)), *_tok_args(w), _V(mask), _V(dx0),
                                         _V(_slab(P, S, N, nchunk)), nchunk, *_grad_args(g), split, _V(g["dmask_token"]), Bs, Hs, Ws,
                                         bad.get("window", window), bad.get("nwin", nwin), S, bad.get("P", P), _stream())
    if bad:
        return rc, g
    assert rc == 0, rc
    return g


@pytest.mark.parametrize("case", KERNEL_CASES, ids=IDS)
def test_masked_listed_tokenizer_forward_is_the_stacked_forward(case):
    from maskedsst_amd import _lib
    lib = _lib.load()
    _, P, S, window, _, Bs, Hs, Ws, split = case
    w, scene, mask = _kernel_inputs(P, S, window, Bs, Hs, Ws, split)
    table = listed_origins(Bs, Hs, Ws, window)
    assert table.shape[0] == 13
    stacked = stack_at(scene, table, window)
    for nwin in (1, 5, 13):
        want = _tok_fwd(lib, w, stacked[:nwin].contiguous(), mask[:nwin].contiguous(), split)
        got = _tok_at_fwd_masked(lib, w, scene, table[:nwin].cuda(), mask[:nwin].contiguous(), window, split)
        torch.cuda.synchronize()
        assert _same(got, want), (case[0], nwin)
    N = window * window
    pos = w["pos_a"] if not split else torch.cat([w["pos_a"].repeat(S, 1), w["pos_b"].repeat_interleave(N, 0)], dim=1)
    assert torch.equal(got[FULL], w["mask_token"] + pos)                     # every token of the fully masked window is the mask token
    assert not bool((got[EMPTY] == w["mask_token"] + pos).all(dim=1).any())   # none of the unmasked one
    zero = torch.zeros_like(mask)
    assert torch.equal(_tok_at_fwd_masked(lib, w, scene, table.cuda(), zero, window, split)[EMPTY], got[EMPTY])
    both = (mask[5] == 0) & (mask[0] == 0)   # rows 0 and 5 list the same window: equal tokens wherever neither is masked
    assert bool(both.any()) and torch.equal(got[5][both], got[0][both])


@pytest.mark.parametrize("case", KERNEL_CASES, ids=IDS)
def test_masked_listed_tokenizer_backward_is_the_stacked_backward(case):
    from maskedsst_amd import _lib
    lib = _lib.load()
    _, P, S, window, _, Bs, Hs, Ws, split = case
    w, scene, mask = _kernel_inputs(P, S, window, Bs, Hs, Ws, split)
    table = listed_origins(Bs, Hs, Ws, window)
    stacked = stack_at(scene, table, window)
    gen = torch.Generator(device="cuda").manual_seed(77)
    dx0 = torch.randn(13, S * window * window, D, device="cuda", generator=gen)
    # (nwin, nchunk): the whole table in one chunk, over an uneven chunking and with nchunk = nwin; fewer windows; one window alone
    for nwin, nchunk in ((13, 1), (13, 3), (13, 13), (5, 3), (5, 5), (1, 1)):
        d, m = dx0[:nwin].contiguous(), mask[:nwin].contiguous()
        want = _tok_bwd(lib, w, stacked[:nwin].contiguous(), m, d, nchunk, split)
        got = _tok_at_bwd_masked(lib, w, scene, table[:nwin].cuda(), m, window, d, nchunk, split)
        torch.cuda.synchronize()
        for k in want:
            assert _same(got[k], want[k]), (case[0], nwin, nchunk, k)
        assert float(got["dmask_token"].abs().max()) > 0
    # the fully masked window alone: all of its gradient goes to the mask token and the position table
    one = slice(FULL, FULL + 1)
    got = _tok_at_bwd_masked(lib, w, scene, table[one].cuda(), mask[one].contiguous(), window, dx0[one].contiguous(), 1, split)
    torch.cuda.synchronize()
    assert all(float(got[k].abs().max()) == 0.0 for k in ("dpre_g", "dpre_b", "dw_emb", "db_emb", "dpost_g", "dpost_b"))
    assert rel_l2(got["dmask_token"], dx0[FULL].double().sum(0)) <= BAR


# ------------------------------------------------------------------------------------------ head
def _head_inputs(P, S, window, K, per_block):
    gen = torch.Generator(device="cuda").manual_seed(31 * P + window + 7 * K + per_block)
    T = S * window * window
    y = torch.randn(13, T, D, device="cuda", generator=gen)
    idx = torch.stack([torch.randperm(T, device="cuda", generator=gen)[:K] for _ in range(13)]).to(torch.int32).contiguous()
    nb = S if per_block else 1
    return y, idx, 0.2 * torch.randn(nb, P, D, device="cuda", generator=gen), 0.1 * torch.randn(nb, P, device="cuda", generator=gen)


def _head_bufs(nwin, K, P):
    return dict(dpred=_nan(nwin, K, P), pred=_nan(nwin, K, P), partial=_nan(nwin * ((K + 63) // 64)), loss=_nan(1))


def _head_fwd(lib, y, img, idx, w_pix, b_pix, per_block, S, P):
    B, K = idx.shape
    o = _head_bufs(B, K, P)
    rc = lib.msst_head_fwd(_V(y), _V(img), _V(idx), _V(w_pix), _V(b_pix), per_block, _V(o["dpred"]), _V(o["pred"]), _V(o["partial"]),
                           _V(o["loss"]), B, S, img.shape[-1] ** 2, P, K, _stream())
    assert rc == 0
    return o


def _head_at_fwd(lib, y, scene, origins, idx, w_pix, b_pix, per_block, window, S, P, want_pred=True, o=None, bad=None):
    Bs, _, Hs, Ws = scene.shape
    nwin, K = idx.shape
    assert origins.is_cuda and origins.dtype == torch.int32 and origins.is_contiguous() and origins.shape[0] == nwin
    o = _head_bufs(nwin, K, P) if o is None else o
    bad = bad or {}
    rc = lib.msst_head_at_fwd(_V(bad.get("y", y)), _V(scene), _V(bad.get("table", origins)), _V(idx), _V(w_pix), _V(b_pix), per_block,
                              _V(o["dpred"]), _V(o["pred"] if want_pred else None), _V(o["partial"]), _V(o["loss"]), Bs, Hs, Ws,
                              bad.get("window", window), bad.get("nwin", nwin), S, bad.get("P", P), K, _stream())
    if bad:
        return rc, o
    assert rc == 0, rc
    return o


def _head_ref64(y, stacked, idx, w_pix, b_pix, per_block, S, P):
    """msst_head_fwd restated in float64 (reference vit_simmim_original.py:314-338): gather, per-block Linear(96 -> P), target = the raw
    pixels of the masked patch, mean |.| / K"""
    B, K = idx.shape
    N = stacked.shape[-1] ** 2
    ix = idx.long().cpu()
    enc = y.double().cpu()[torch.arange(B)[:, None], ix]                       # [B, K, 96]
    blk = (ix // N) if per_block else torch.zeros_like(ix)
    pred = torch.einsum("bkd,bkpd->bkp", enc, w_pix.double().cpu()[blk]) + b_pix.double().cpu()[blk]
    patches = stacked.double().cpu().reshape(B, S, P, N).permute(0, 1, 3, 2).reshape(B, S * N, P)   # token c N + n: its P pixels
    target = patches[torch.arange(B)[:, None], ix]
    return pred, target, (pred - target).abs().mean() / K


@pytest.mark.parametrize("per_block", [0, 1])
@pytest.mark.parametrize("case", KERNEL_CASES, ids=IDS)
def test_listed_head_forward_is_the_stacked_head_forward(case, per_block):
    from maskedsst_amd import _lib
    lib = _lib.load()
    _, P, S, window, _, Bs, Hs, Ws, _ = case
    _, scene, _ = _kernel_inputs(P, S, window, Bs, Hs, Ws, 0)
    table = listed_origins(Bs, Hs, Ws, window)
    stacked = stack_at(scene, table, window)
    T = S * window * window
    for K in (int(0.7 * T), 1):
        assert K % 64 != 0
        y, idx, w_pix, b_pix = _head_inputs(P, S, window, K, per_block)
        for nwin in (13, 2):
            args = (y[:nwin].contiguous(), idx[:nwin].contiguous(), w_pix, b_pix, per_block)
            want = _head_fwd(lib, args[0], stacked[:nwin].contiguous(), *args[1:], S, P)
            got = _head_at_fwd(lib, args[0], scene, table[:nwin].cuda(), *args[1:], window, S, P)
            nopred = _head_at_fwd(lib, args[0], scene, table[:nwin].cuda(), *args[1:], window, S, P, want_pred=False)
            torch.cuda.synchronize()
            for k in ("loss", "dpred", "pred", "partial"):
                assert _same(got[k], want[k]), (case[0], per_block, K, nwin, k)
            assert all(torch.equal(nopred[k], got[k]) for k in ("loss", "dpred", "partial")) and bool(torch.isnan(nopred["pred"]).all())
        # ... and against float64, at the bar msst_head_fwd is held to
        pred64, target, loss64 = _head_ref64(y, stacked, idx, w_pix, b_pix, per_block, S, P)
        full = _head_at_fwd(lib, y, scene, table.cuda(), idx, w_pix, b_pix, per_block, window, S, P)
        torch.cuda.synchronize()
        err_pred, err_loss = rel_l2(full["pred"], pred64), abs(float(full["loss"]) - float(loss64)) / abs(float(loss64))
        print(case[0], per_block, K, f"pred {err_pred:.2e} loss {err_loss:.2e}")
        assert err_pred <= BAR and err_loss <= BAR, (case[0], per_block, K, err_pred, err_loss)
        diff = pred64 - target
        clear = diff.abs() >= BAND
        assert torch.equal(full["dpred"].double().cpu()[clear], torch.sign(diff)[clear])
        assert bool(((full["dpred"] == 1) | (full["dpred"] == -1) | (full["dpred"] == 0)).all())


def test_the_three_calls_check_their_arguments_and_write_nothing():
    """with real buffers on the device: a refused call leaves every output at its NaN prefill"""
    from maskedsst_amd import _lib
    lib = _lib.load()
    _, P, S, window, _, Bs, Hs, Ws, split = KERNEL_CASES[0]
    w, scene, mask = _kernel_inputs(P, S, window, Bs, Hs, Ws, split)
    table = listed_origins(Bs, Hs, Ws, window).cuda()
    N, T = window * window, S * window * window
    dx0 = torch.randn(13, T, D, device="cuda")
    y, idx, w_pix, b_pix = _head_inputs(P, S, window, int(0.7 * T), 1)
    bads = [(dict(table=None), BADARG), (dict(nwin=-1), BADARG), (dict(window=9), UNSUPPORTED), (dict(P=17), UNSUPPORTED)]
    for bad, code in bads:
        out = _nan(13, T, D)
        rc, _ = _tok_at_fwd_masked(lib, w, scene, table, mask, window, split, out=out, bad=bad)
        g = _grad_bufs(P, S, N, split)
        rc_b, _ = _tok_at_bwd_masked(lib, w, scene, table, mask, window, dx0, 3, split, g=g, bad=bad)
        o = _head_bufs(13, idx.shape[1], P)
        rc_h, _ = _head_at_fwd(lib, y, scene, table, idx, w_pix, b_pix, 1, window, S, P, o=o, bad=bad)
        torch.cuda.synchronize()
        assert (rc, rc_b, rc_h) == (code, code, code), (bad, rc, rc_b, rc_h)
        assert bool(torch.isnan(out).all()) and all(bool(torch.isnan(v).all()) for v in g.values() if v is not None)
        assert all(bool(torch.isnan(v).all()) for v in o.values()), bad
    o = _head_bufs(13, idx.shape[1], P)
    rc_h, _ = _head_at_fwd(lib, y, scene, table, idx, w_pix, b_pix, 1, window, S, P, o=o, bad=dict(y=None))
    torch.cuda.synchronize()
    assert rc_h == BADARG and all(bool(torch.isnan(v).all()) for v in o.values())


# ------------------------------------------------------------------------------------------ model level
TILE_HW = (16, 16)
# (name, image_size, spectral patch P, mask_patch_size, tube_masking, to_pixels_per_spectral_block, spectral_pos_embed): the three mask
# modes, both to_pixels forms, both position-table forms; gen6: the generic tokenizer kernels (6 x 6 windows, 5-band patches, S = 4)
MODELS = {
    "tube": (8, 10, 4, True, True, False),
    "nontube_shared_specpos": (8, 10, 4, False, False, True),
    "mps1_specpos": (8, 10, 1, False, True, True),
    "gen6_tube_shared": (6, 5, 2, True, False, False),
    "gen6_nontube_specpos": (6, 5, 2, False, True, True),
}


def _mim(name, precision="fp32", dropout=0.0):
    from maskedsst_amd import ViTSpatialSpectral, SimMIMSpatialSpectral
    s, P, mps, tube, per_block, specpos = MODELS[name]
    seed_all(5)
    enc = ViTSpatialSpectral(
        image_size=s, spatial_patch_size=1, spectral_patch_size=P, num_classes=5, dim=96, depth=1, heads=2, mlp_dim=64, dropout=dropout,
        emb_dropout=dropout, channels=20, spectral_pos_embed=specpos, spectral_pos=torch.arange(20 // P), blockwise_patch_embed=True,
        precision=precision)
    return SimMIMSpatialSpectral(encoder=enc, masking_ratio=0.7, mask_patch_size=mps, tube_masking=tube,
                                 to_pixels_per_spectral_block=per_block)


def _cfg(name):
    s, P, mps, tube, per_block, specpos = MODELS[name]
    return dict(bands=20, depth=1, heads=2, image_size=s, spectral_patch=P, mask_patch_size=mps, tube_masking=tube, masking_ratio=0.7,
                to_pixels_per_spectral_block=per_block, spectral_pos_embed=specpos, n_classes=5)


def _tiles_and_table(name):
    s = MODELS[name][0]
    g = torch.Generator().manual_seed(21)
    return s, torch.randn(2, 20, *TILE_HW, generator=g), listed_origins(2, *TILE_HW, s)


def _grads(mim):
    return {k: q.grad.clone() for k, q in mim.named_parameters() if q.grad is not None}


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(MODELS))
def test_forward_at_is_forward_of_the_stacked_windows(name, precision):
    mim = _mim(name, precision, dropout=0.1).cuda()
    s, tiles, table = _tiles_and_table(name)
    tiles = tiles.cuda()
    stacked = stack_at(tiles, table, s)
    masks = mim.draw_masks(13)
    assert tuple(masks[0].shape) == (13, mim.encoder.num_patches)
    mim.eval()
    with torch.no_grad():
        a, b = mim.forward_at(tiles, table.cuda(), masks), mim(stacked, masks)
        assert mim.last_masks is masks
        others = [mim.forward_at(tiles, table, masks), mim.forward_at(tiles, table, masks, check=False), mim.forward_at(tiles, table.long(), masks)]
    assert a.shape == b.shape == () and torch.equal(a, b) and bool(torch.isfinite(a))
    assert all(torch.equal(o, a) for o in others)
    mim.train()
    with torch.no_grad():   # training mode without a graph: the dropout is on, nothing is saved
        torch.manual_seed(11)
        c = mim.forward_at(tiles, table, masks)
        torch.manual_seed(11)
        d = mim(stacked, masks)
    assert torch.equal(c, d) and not torch.equal(c, a)
    runs = []
    for fwd in (lambda: mim.forward_at(tiles, table.cuda(), masks), lambda: mim(stacked, masks),
                lambda: mim.forward_at(tiles, table, masks, check=False)):
        mim.zero_grad(set_to_none=True)
        torch.manual_seed(11)   # pins the step's dropout seeds
        loss = fwd()
        (loss * 3.0).backward()
        torch.cuda.synchronize()
        runs.append((loss.detach().clone(), _grads(mim)))
    (l_t, g_t), (l_s, g_s), (l_2, g_2) = runs
    assert torch.equal(l_t, l_s) and torch.equal(l_t, c)   # the same dropout masks as the graphless run, and dropout was on
    want = sorted(g_s)   # every parameter the stacked step gives a gradient
    assert sorted(g_t) == sorted(g_2) == want and "mask_token" in want and any(k.startswith("to_pixels") for k in want)
    bad = [k for k in want if not (torch.equal(g_t[k], g_s[k]) and bool(torch.isfinite(g_t[k]).all()))]
    assert not bad, bad
    assert torch.equal(l_2, l_t) and not [k for k in want if not torch.equal(g_2[k], g_t[k])]   # a second backward: the same bits
    assert float(g_t["mask_token"].abs().max()) > 0 and sum(float(g_t[k].abs().max()) > 0 for k in want) > len(want) // 2
    assert tiles.grad is None
    with pytest.raises(RuntimeError, match="accumulation"):   # the hand-off of _SimMIMLossFn: gradients are views of the flat buffer
        mim.forward_at(tiles, table, masks).backward()


@pytest.mark.parametrize("name", ["tube", "gen6_nontube_specpos"])
def test_forward_at_draws_the_masks_forward_draws(name):
    """masks=None: draw_masks(n) from the generators as they stand, kept in last_masks -- the stacked forward's draw"""
    mim = _mim(name).cuda().eval()
    s, tiles, table = _tiles_and_table(name)
    tiles = tiles.cuda()
    with torch.no_grad():
        seed_all(9)
        a = mim.forward_at(tiles, table)
        drawn = mim.last_masks
        seed_all(9)
        b = mim(stack_at(tiles, table, s))
    assert torch.equal(a, b) and torch.equal(torch.as_tensor(drawn[0]), torch.as_tensor(mim.last_masks[0]))
    assert tuple(drawn[0].shape) == (13, mim.encoder.num_patches)


@pytest.mark.parametrize("name", ["tube", "gen6_tube_shared"])
def test_forward_windows_is_forward_at_over_the_grid(name):
    from maskedsst_amd.config import Dotdict
    from maskedsst_amd.scene import scene_windows
    from maskedsst_amd.utils import stack_image_batch
    mim = _mim(name, dropout=0.1).cuda().train()
    s = MODELS[name][0]
    tiles = torch.randn(2, 20, 17, 17, generator=torch.Generator().manual_seed(4)).cuda()   # 17 % 8 = 1, 17 % 6 = 5: a cut-off
    grid = torch.tensor([(b, y, x) for b in range(2) for y, x in scene_windows(17, 17, s, s)], dtype=torch.int32)
    stacked, _ = stack_image_batch(Dotdict(dict(image_size=s)), tiles, torch.zeros(2, 17, 17, dtype=torch.long))
    n = 2 * (17 // s) ** 2
    assert grid.shape[0] == stacked.shape[0] == n
    runs = []
    for fwd in (lambda: mim.forward_windows(tiles), lambda: mim.forward_at(tiles, grid), lambda: mim(stacked.contiguous())):
        mim.zero_grad(set_to_none=True)
        seed_all(13)   # the masks and the dropout seeds
        loss = fwd()
        assert tuple(mim.last_masks[0].shape) == (n, mim.encoder.num_patches)
        loss.backward()
        torch.cuda.synchronize()
        runs.append((loss.detach().clone(), _grads(mim)))
    for l, g in runs[1:]:
        assert torch.equal(l, runs[0][0]) and bool(torch.isfinite(l))
        assert not [k for k in g if not torch.equal(g[k], runs[0][1][k])]
    masks = mim.draw_masks(n)
    with torch.no_grad():
        seed_all(1)
        a = mim.forward_windows(tiles, masks)
        seed_all(1)
        b = mim.forward_at(tiles, grid, masks)
    assert torch.equal(a, b) and mim.last_masks is masks


@pytest.mark.parametrize("name,precision", [("tube", "fp32"), ("tube", "bf16"), ("mps1_specpos", "fp32"), ("mps1_specpos", "bf16"),
                                            ("nontube_shared_specpos", "fp32"), ("gen6_tube_shared", "fp32"), ("gen6_nontube_specpos", "fp32")])
def test_forward_at_vs_oracle(name, precision):
    """the oracle runs on the copied windows with the same masks: the loss at the bars of tests/test_gpu_forward.py::test_forward_stages
    (1e-4 relative in fp32, 2.5e-4 relative in bf16).  The bf16 bar was measured on 8 x 8 windows of 10-band patches, so the 6 x 6 / 5-band
    models are held to the fp32 bar alone."""
    from oracle import simmim_forward
    mim = _mim(name, precision)
    params = {k: v.detach().clone() for k, v in mim.state_dict().items()}
    s, tiles, table = _tiles_and_table(name)
    masks = mim.draw_masks(13)
    with torch.no_grad():
        ref = simmim_forward(params, stack_at(tiles, table, s), oracle_cfg(_cfg(name)), masks=masks)["loss"].item()
        got = mim.cuda().eval().forward_at(tiles.cuda(), table, masks).item()
    print(name, precision, got, ref, abs(got - ref) / abs(ref))
    assert abs(got - ref) <= (1e-4 * abs(ref) + 1e-7 if precision == "fp32" else 2.5e-4 * abs(ref)), (got, ref)


@pytest.mark.parametrize("name,precision", [("tube", "bf16"), ("gen6_nontube_specpos", "fp32")])
def test_three_adamw_steps_through_forward_at(name, precision):
    from maskedsst_amd.optim import FusedAdamW
    s, tiles, table = _tiles_and_table(name)
    tiles = tiles.cuda()
    stacked = stack_at(tiles, table, s)
    results = []
    for at in (True, False):
        mim = _mim(name, precision, dropout=0.1).cuda().train()
        before = {k: q.detach().clone() for k, q in mim.named_parameters()}
        opt = FusedAdamW(mim, lr=1e-3, weight_decay=0.05, grad_clamp=1.0)
        seed_all(7)   # the masks and the dropout seeds of the three steps
        losses = []
        for _ in range(3):
            opt.zero_grad()
            loss = mim.forward_at(tiles, table) if at else mim(stacked)
            loss.backward()
            opt.step()
            losses.append(loss.detach().clone())
        torch.cuda.synchronize()
        after = {k: q.detach().clone() for k, q in mim.named_parameters()}
        # (the encoder's classification head takes no part in pre-training: no gradient, no step)
        still = [k for k in after if torch.equal(after[k], before[k]) and not k.startswith("encoder.mlp_head.")]
        assert not still, still
        results.append((torch.stack(losses), after))
    (l_at, p_at), (l_st, p_st) = results
    print(name, precision, l_at.tolist(), l_st.tolist())
    assert torch.equal(l_at, l_st) and bool(torch.isfinite(l_at).all()) and len(set(l_at.tolist())) == 3
    bad = [k for k in p_at if not (torch.equal(p_at[k], p_st[k]) and bool(torch.isfinite(p_at[k]).all()))]
    assert not bad, bad


# ------------------------------------------------------------------------------------------ pretrain.py
def _run(cmd, timeout=600):
    e = dict(os.environ)
    e.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
    r = subprocess.run(cmd, cwd=ROOT, env=e, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, f"{' '.join(cmd)}\n--- stdout\n{r.stdout[-4000:]}\n--- stderr\n{r.stderr[-4000:]}"
    return r.stdout


def _pretrain(tmp_path, tag, *extra):
    """3 steps of pretrain.py (depth 1, batch 8, the script's fixed seed), a loss line per step -> (printed losses, checkpoint)"""
    cfg = tmp_path / "pretrain_config.yaml"
    if not cfg.exists():
        text = open(os.path.join(ROOT, "configs", "pretrain_config.yaml")).read()
        assert "logging_freq: 10" in text
        cfg.write_text(text.replace("logging_freq: 10", "logging_freq: 1"))
    save = str(tmp_path / tag)
    out = _run([sys.executable, "pretrain.py", "--synthetic", "--config", str(cfg), "--batch-size", "8", "--tiles", "24", "--epochs", "1",
                "--max-steps", "3", "--depth", "1", "--pool-tiles", "8", "--val-tiles", "1", "--save-dir", save, *extra])
    losses = re.findall(r"^epoch 0 step (\d) loss (\S+) ", out, re.M)
    assert [int(n) for n, _ in losses] == [1, 2, 3], out
    ck = torch.load(os.path.join(save, "model_ViTSpatialSpectral_ep0.pth"), map_location="cpu", weights_only=False)
    return [v for _, v in losses], ck


def test_pretrain_resident_tiles_prints_the_losses_of_the_host_loader(tmp_path):
    host, ck_h = _pretrain(tmp_path, "host")
    res, ck_r = _pretrain(tmp_path, "resident", "--resident-tiles")
    print(host, res)
    assert res == host and all(torch.isfinite(torch.tensor(float(v))) for v in res)
    assert torch.equal(ck_r["losses"], ck_h["losses"]) and ck_h["losses"].numel() == 3   # ... and bit for bit, not to the printed digits
    assert torch.equal(ck_r["input"], ck_h["input"]) and tuple(ck_r["input"].shape) == (8, 200, 8, 8)   # the last step's windows
    sd_h, sd_r = ck_h["model_state_dict"], ck_r["model_state_dict"]
    assert sorted(sd_h) == sorted(sd_r) and not [k for k in sd_h if not torch.equal(sd_h[k], sd_r[k])]


def test_pretrain_resident_tiles_crop_sample_trains(tmp_path):
    res, ck = _pretrain(tmp_path, "sample", "--resident-tiles", "--crop", "sample")
    assert all(torch.isfinite(torch.tensor(float(v))) for v in res) and bool(torch.isfinite(ck["losses"]).all())
    win = ck["input"]
    assert tuple(win.shape) == (8, 200, 8, 8)
    r = subprocess.run([sys.executable, "pretrain.py", "--crop", "sample"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--resident-tiles" in r.stderr   # the host loader cuts one position per batch
