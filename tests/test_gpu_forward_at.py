"""GPU: windows at listed scene positions.  The listed-origins tokenizer kernels (msst_tokenize_at_fwd / msst_tokenize_at_bwd) bit for bit
against msst_tokenize_fwd / msst_tokenize_bwd on the stacked copy of the listed windows and, for a table that lists a regular grid in grid
order, against msst_tokenize_scene_fwd_train / msst_tokenize_scene_bwd; ViTSpatialSpectral.forward_at bit for bit against forward(stacked
windows) for the three heads, both precisions, full finetune and linear evaluation, with dropout on; against the oracle at the
classification path's bars; predict_at; and utils.train_step_at against the same step on the stacked copy."""
import ctypes
import importlib.util
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, oracle_cfg_from, seed_all
from util import pix_head_ref, rel_l2, relerr, spectral_head_ref

pytestmark = pytest.mark.gpu

D = 96
# tests/test_gpu_shifting_window.py::KERNEL_CASES restated: (name, P, S, window, stride, Bs, Hs, Ws, pos_split); P = 10 and window 8 run
# the fp32-MFMA kernels, everything else the generic ones
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


def _V(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def listed_origins(Bs, Hs, Ws, window):
    """13 rows (scene, y0, x0), built from the shapes alone: the first window of the first scene, the last window of the last scene (the
    last row and column a window may touch), exact duplicates of both, windows one pixel apart in x and in y, every corner, and the scenes
    interleaved out of order.  13 is no multiple of anything the kernels count in."""
    my, mx, last = Hs - window, Ws - window, Bs - 1
    assert my >= 3 and mx >= 3
    rows = [(0, 0, 0), (last, my, mx), (0, my // 2, mx // 2), (0, my // 2, mx // 2 + 1), (last, my // 2 + 1, mx // 2), (0, 0, 0),
            (last, 0, mx), (0, my, 0), (last, 1, 1), (0, my - 1, mx - 1), (last, my, mx), (0, 3 % (my + 1), 5 % (mx + 1)), (last, 2, 0)]
    assert all(0 <= s < Bs and 0 <= y <= my and 0 <= x <= mx for s, y, x in rows)
    return torch.tensor(rows, dtype=torch.int32)


def stack_at(scene, origins, window):
    return torch.stack([scene[s, :, y:y + window, x:x + window] for s, y, x in origins.tolist()]).contiguous()


def _kernel_inputs(P, S, window, Bs, Hs, Ws, split):
    gen = torch.Generator(device="cuda").manual_seed(1000 * P + 10 * window + split)
    r = lambda *shape: torch.randn(*shape, device="cuda", generator=gen)   # noqa: E731
    N = window * window
    w = dict(pre_g=1 + 0.3 * r(P), pre_b=0.2 * r(P), w_emb=0.4 * r(S, D, P), b_emb=0.1 * r(S, D), post_g=1 + 0.3 * r(D), post_b=0.2 * r(D))
    if split:
        w["pos_a"], w["pos_b"] = r(N, split), r(S, D - split)
    else:
        w["pos_a"], w["pos_b"] = r(S * N, D), None
    return w, r(Bs, S * P, Hs, Ws)


def _tok_fwd(lib, w, img, split, p, seed):
    B, C, win, _ = img.shape
    P = w["pre_g"].numel()
    S, N = C // P, win * win
    out = torch.full((B, S * N, D), float("nan"), device="cuda")
    mask = torch.zeros(B * S * N, dtype=torch.uint8, device="cuda")
    rc = lib.msst_tokenize_fwd(_V(img), _V(w["pre_g"]), _V(w["pre_b"]), _V(w["w_emb"]), _V(w["b_emb"]), _V(w["post_g"]), _V(w["post_b"]),
                               _V(w["pos_a"]), _V(w["pos_b"]), split, _V(w["post_b"]), _V(mask), _V(out), B, S, N, P, p, seed, _stream())
    assert rc == 0
    return out


def _tok_at_fwd(lib, w, scene, origins, window, split, p, seed):
    Bs, C, Hs, Ws = scene.shape
    P = w["pre_g"].numel()
    S, N, nwin = C // P, window * window, origins.shape[0]
    assert origins.is_cuda and origins.dtype == torch.int32 and origins.is_contiguous()
    out = torch.full((nwin, S * N, D), float("nan"), device="cuda")
    rc = lib.msst_tokenize_at_fwd(_V(scene), _V(origins), _V(w["pre_g"]), _V(w["pre_b"]), _V(w["w_emb"]), _V(w["b_emb"]), _V(w["post_g"]),
                                  _V(w["post_b"]), _V(w["pos_a"]), _V(w["pos_b"]), split, _V(out), Bs, Hs, Ws, window, nwin, S, P, p, seed,
                                  _stream())
    assert rc == 0
    return out


def _tok_scene_fwd(lib, w, scene, window, stride, nwin, split, p, seed):
    Bs, C, Hs, Ws = scene.shape
    P = w["pre_g"].numel()
    S, N = C // P, window * window
    out = torch.full((nwin, S * N, D), float("nan"), device="cuda")
    rc = lib.msst_tokenize_scene_fwd_train(_V(scene), _V(w["pre_g"]), _V(w["pre_b"]), _V(w["w_emb"]), _V(w["b_emb"]), _V(w["post_g"]),
                                           _V(w["post_b"]), _V(w["pos_a"]), _V(w["pos_b"]), split, _V(out), Bs, Hs, Ws, window, stride,
                                           0, nwin, S, P, p, seed, _stream())
    assert rc == 0
    return out


def _grad_bufs(P, S, N, split):
    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")   # noqa: E731
    g = dict(dpre_g=nan(P), dpre_b=nan(P), dw_emb=nan(S, D, P), db_emb=nan(S, D), dpost_g=nan(D), dpost_b=nan(D))
    g["dpos_a"], g["dpos_b"] = (nan(N, split), nan(S, D - split)) if split else (nan(S * N, D), None)
    return g


def _slab(P, S, N, nchunk):
    return torch.full((S * nchunk * (N * D + D * P + 4 * D + 32) + S * N * D,), float("nan"), device="cuda")


def _tok_bwd(lib, w, img, dx0, nchunk, split, p, seed):
    B, C, win, _ = img.shape
    P = w["pre_g"].numel()
    S, N = C // P, win * win
    g = _grad_bufs(P, S, N, split)
    mask = torch.zeros(B * S * N, dtype=torch.uint8, device="cuda")
    rc = lib.msst_tokenize_bwd(_V(img), _V(w["pre_g"]), _V(w["pre_b"]), _V(w["w_emb"]), _V(w["b_emb"]), _V(w["post_g"]), _V(w["post_b"]),
                               _V(mask), _V(dx0), _V(_slab(P, S, N, nchunk)), nchunk, _V(g["dpre_g"]), _V(g["dpre_b"]), _V(g["dw_emb"]),
                               _V(g["db_emb"]), _V(g["dpost_g"]), _V(g["dpost_b"]), _V(g["dpos_a"]), _V(g["dpos_b"]), split, None,
                               B, S, N, P, p, seed, _stream())
    assert rc == 0
    return g


def _tok_at_bwd(lib, w, scene, origins, window, dx0, nchunk, split, p, seed):
    Bs, C, Hs, Ws = scene.shape
    P = w["pre_g"].numel()
    S, N, nwin = C // P, window * window, origins.shape[0]
    assert origins.is_cuda and origins.dtype == torch.int32 and origins.is_contiguous() and dx0.shape[0] == nwin
    g = _grad_bufs(P, S, N, split)
    rc = lib.msst_tokenize_at_bwd(_V(scene), _V(origins), _V(w["pre_g"]), _V(w["pre_b"]), _V(w["w_emb"]), _V(w["b_emb"]), _V(w["post_g"]),
                                  _V(w["post_b"]), _V(dx0), _V(_slab(P, S, N, nchunk)), nchunk, _V(g["dpre_g"]), _V(g["dpre_b"]),
                                  _V(g["dw_emb"]), _V(g["db_emb"]), _V(g["dpost_g"]), _V(g["dpost_b"]), _V(g["dpos_a"]), _V(g["dpos_b"]),
                                  split, Bs, Hs, Ws, window, nwin, S, P, p, seed, _stream())
    assert rc == 0
    return g


def _tok_scene_bwd(lib, w, scene, window, stride, nwin, dx0, nchunk, split, p, seed):
    Bs, C, Hs, Ws = scene.shape
    P = w["pre_g"].numel()
    S, N = C // P, window * window
    g = _grad_bufs(P, S, N, split)
    rc = lib.msst_tokenize_scene_bwd(_V(scene), _V(w["pre_g"]), _V(w["pre_b"]), _V(w["w_emb"]), _V(w["b_emb"]), _V(w["post_g"]),
                                     _V(w["post_b"]), _V(dx0), _V(_slab(P, S, N, nchunk)), nchunk, _V(g["dpre_g"]), _V(g["dpre_b"]),
                                     _V(g["dw_emb"]), _V(g["db_emb"]), _V(g["dpost_g"]), _V(g["dpost_b"]), _V(g["dpos_a"]), _V(g["dpos_b"]),
                                     split, Bs, Hs, Ws, window, stride, 0, nwin, S, P, p, seed, _stream())
    assert rc == 0
    return g


def _grid_origins(Bs, Hs, Ws, window, stride):
    from maskedsst_amd.scene import scene_windows
    return torch.tensor([(b, y, x) for b in range(Bs) for y, x in scene_windows(Hs, Ws, window, stride)], dtype=torch.int32)


def _same(a, b):
    """bitwise equal and free of the NaN prefill"""
    return a is b is None or (torch.equal(a, b) and bool(torch.isfinite(a).all()))


@pytest.mark.parametrize("case", KERNEL_CASES, ids=IDS)
def test_listed_tokenizer_forward_is_the_stacked_forward(case):
    from maskedsst_amd import _lib
    lib = _lib.load()
    _, P, S, window, stride, Bs, Hs, Ws, split = case
    w, scene = _kernel_inputs(P, S, window, Bs, Hs, Ws, split)
    table = listed_origins(Bs, Hs, Ws, window)
    assert table.shape[0] == 13
    stacked = stack_at(scene, table, window)
    grid = _grid_origins(Bs, Hs, Ws, window, stride)
    for p, seed in ((0.0, 0), (0.1, 12345)):
        for nwin in (1, 5, table.shape[0]):
            want = _tok_fwd(lib, w, stacked[:nwin].contiguous(), split, p, seed)
            got = _tok_at_fwd(lib, w, scene, table[:nwin].cuda(), window, split, p, seed)
            torch.cuda.synchronize()
            assert _same(got, want), (case[0], p, nwin)
            if not p and nwin == table.shape[0]:
                assert torch.equal(got[5], got[0]) and torch.equal(got[10], got[1])   # the duplicates
                assert not torch.equal(got[3], got[2])                                # one pixel apart
        if p:
            dropped = float((got == 0).float().mean())
            assert 0.05 < dropped < 0.15, dropped   # the dropout is on: a tenth of the elements are zero
        # the table of the regular grid, in grid order: the scene entry point's bits
        want = _tok_scene_fwd(lib, w, scene, window, stride, grid.shape[0], split, p, seed)
        got = _tok_at_fwd(lib, w, scene, grid.cuda(), window, split, p, seed)
        torch.cuda.synchronize()
        assert _same(got, want), (case[0], p, "grid")


@pytest.mark.parametrize("case", KERNEL_CASES, ids=IDS)
def test_listed_tokenizer_backward_is_the_stacked_backward(case):
    from maskedsst_amd import _lib
    lib = _lib.load()
    _, P, S, window, stride, Bs, Hs, Ws, split = case
    w, scene = _kernel_inputs(P, S, window, Bs, Hs, Ws, split)
    table = listed_origins(Bs, Hs, Ws, window)
    stacked = stack_at(scene, table, window)
    grid = _grid_origins(Bs, Hs, Ws, window, stride)
    gen = torch.Generator(device="cuda").manual_seed(77)
    dx0 = torch.randn(max(table.shape[0], grid.shape[0]), S * window * window, D, device="cuda", generator=gen)
    # (nwin, nchunk): nchunk below and equal to nwin = 5, one window alone, and the whole table over an uneven chunking
    for p, seed in ((0.0, 0), (0.1, 12345)):
        for nwin, nchunk in ((5, 1), (5, 2), (5, 5), (1, 1), (table.shape[0], 3)):
            d = dx0[:nwin].contiguous()
            want = _tok_bwd(lib, w, stacked[:nwin].contiguous(), d, nchunk, split, p, seed)
            got = _tok_at_bwd(lib, w, scene, table[:nwin].cuda(), window, d, nchunk, split, p, seed)
            torch.cuda.synchronize()
            for k in want:
                assert _same(got[k], want[k]), (case[0], p, nwin, nchunk, k)
        d = dx0[:grid.shape[0]].contiguous()
        want = _tok_scene_bwd(lib, w, scene, window, stride, grid.shape[0], d, 3, split, p, seed)
        got = _tok_at_bwd(lib, w, scene, grid.cuda(), window, d, 3, split, p, seed)
        torch.cuda.synchronize()
        for k in want:
            assert _same(got[k], want[k]), (case[0], p, "grid", k)


# ------------------------------------------------------------------------------------------ model level
HEADS = {"default": dict(), "spectral": dict(spectral_mlp_head=True), "pixelwise": dict(pixelwise=True)}
SCENE_HW = (13, 15)   # Hs != Ws, neither a multiple of a window


def _encoder(head, precision="fp32", dropout=0.0, depth=1, heads=2, n_classes=5):
    from maskedsst_amd import ViTSpatialSpectral
    return ViTSpatialSpectral(
        image_size=7 if head == "pixelwise" else 8, spatial_patch_size=1, spectral_patch_size=10, num_classes=n_classes, dim=96,
        depth=depth, heads=heads, mlp_dim=64, dropout=dropout, emb_dropout=dropout, channels=20, spectral_pos_embed=False,
        spectral_pos=torch.arange(2), blockwise_patch_embed=True, precision=precision, **HEADS[head])


def _scene_and_table(head):
    s = 7 if head == "pixelwise" else 8
    scene = torch.randn(2, 20, *SCENE_HW)
    return s, scene, listed_origins(2, *SCENE_HW, s)


@pytest.mark.parametrize("linear_eval", [False, True], ids=["full", "linear_eval"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("head", list(HEADS))
def test_forward_at_is_forward_of_the_stacked_windows(head, precision, linear_eval):
    seed_all(5)
    enc = _encoder(head, precision, dropout=0.1).cuda()
    if linear_eval:
        for n, q in enc.named_parameters():
            q.requires_grad_("mlp_head" in n)
    s, scene, table = _scene_and_table(head)
    scene = scene.cuda()
    stacked = stack_at(scene, table, s)
    n = table.shape[0]
    shape = (n, 5) if head == "pixelwise" else (n, 5, s, s)
    enc.eval()
    with torch.no_grad():
        a, b = enc.forward_at(scene, table.cuda()), enc(stacked)
        on_cpu, unchecked, as_long = enc.forward_at(scene, table), enc.forward_at(scene, table, check=False), enc.forward_at(scene, table.long())
    assert a.shape == b.shape == shape and torch.equal(a, b) and bool(torch.isfinite(a).all())
    assert torch.equal(on_cpu, a) and torch.equal(unchecked, a) and torch.equal(as_long, a)
    enc.train()
    cot = torch.randn(shape, device="cuda")
    runs = []
    for fwd in (lambda: enc.forward_at(scene, table.cuda()), lambda: enc(stacked), lambda: enc.forward_at(scene, table, check=False)):
        enc.zero_grad(set_to_none=True)
        torch.manual_seed(11)   # pins the step's dropout seeds
        out = fwd()
        (out * cot).sum().backward()
        torch.cuda.synchronize()
        runs.append((out.detach().clone(), {k: q.grad.clone() for k, q in enc.named_parameters() if q.grad is not None}))
    (out_t, g_t), (out_s, g_s), (out_2, g_2) = runs
    assert torch.equal(out_t, out_s) and not torch.equal(out_t, a)   # the same dropout masks, and dropout was on
    want = [k for k, q in enc.named_parameters() if q.requires_grad]
    assert sorted(g_t) == sorted(g_s) == sorted(g_2) == sorted(want) and (not linear_eval or all("mlp_head" in k for k in want))
    bad = [k for k in want if not (torch.equal(g_t[k], g_s[k]) and bool(torch.isfinite(g_t[k]).all()))]
    assert not bad, bad
    assert torch.equal(out_2, out_t) and not [k for k in want if not torch.equal(g_2[k], g_t[k])]   # a second backward: the same bits
    assert any(float(g_t[k].abs().max()) > 0 for k in want)


def test_forward_at_keeps_the_refusals():
    """a bad row, a scene that wants a gradient, an encoder wrapped in SimMIM under grad, and gradient accumulation"""
    from maskedsst_amd import SimMIMSpatialSpectral
    seed_all(5)
    enc = _encoder("default").cuda()
    s, scene, table = _scene_and_table("default")
    scene = scene.cuda()
    bad = table.clone()
    bad[6, 2] = SCENE_HW[1] - s + 1
    with pytest.raises(ValueError, match=r"row 6\b"):
        enc.forward_at(scene, bad.cuda())
    with pytest.raises(NotImplementedError, match="(?i)overlap"):
        enc.forward_at(scene.clone().requires_grad_(True), table)
    enc.forward_at(scene, table).sum().backward()
    with pytest.raises(RuntimeError, match="accumulation"):
        enc.forward_at(scene, table).sum().backward()
    enc2 = _encoder("default")
    mim = SimMIMSpatialSpectral(encoder=enc2, masking_ratio=0.7, mask_patch_size=4, tube_masking=True,
                                to_pixels_per_spectral_block=True).cuda()   # kept alive: the encoder holds its wrapper weakly
    assert mim.encoder is enc2
    with pytest.raises(NotImplementedError):
        enc2.forward_at(scene, table)
    with torch.no_grad():
        assert enc2.forward_at(scene, table).shape == (13, 5, 8, 8)


def _oracle_logits(params, img, head, cfg):
    from oracle import classify_forward
    from oracle.model import encoder_embed, pos_table, transformer_forward
    ocfg = oracle_cfg_from(cfg)
    if head == "default":
        return classify_forward(params, img, ocfg)
    _, tok = encoder_embed(params, img, ocfg)
    y = transformer_forward(params, tok + pos_table(params, ocfg), ocfg)
    i = 2 if head == "pixelwise" else 1
    args = (y, params["encoder.mlp_head.0.weight"], params["encoder.mlp_head.0.bias"], params[f"encoder.mlp_head.{i}.weight"],
            params[f"encoder.mlp_head.{i}.bias"], ocfg.S)
    return pix_head_ref(*args, ocfg.Nsq ** 2) if head == "pixelwise" else spectral_head_ref(*args, ocfg.Nsq)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("head", list(HEADS))
def test_forward_at_vs_oracle(head, precision):
    """the oracle runs on the copied windows.  fp32: the classification path's bar of tests/test_gpu_shifting_window.py (logits 1e-4 of
    their maximum); bf16: that of tests/test_gpu_pixelwise.py (logits 1e-2 in relative L2: bf16 MFMA operands of the
    blocks).  The same kernels as forward, so no bar of its own."""
    seed_all(5)
    cfg = dict(bands=20, depth=1, heads=2, n_classes=5, image_size=7 if head == "pixelwise" else 8)
    enc = _encoder(head, precision)
    s, scene, table = _scene_and_table(head)
    params = {"encoder." + k: v.detach().clone() for k, v in enc.state_dict().items()}
    with torch.no_grad():
        ref = _oracle_logits(params, stack_at(scene, table, s), head, cfg)
        logits = enc.cuda().eval().forward_at(scene.cuda(), table)
    assert logits.shape == ref.shape
    errs = dict(max=relerr(logits, ref), l2=rel_l2(logits, ref))
    print(head, precision, errs)
    assert errs["max"] < 1e-4 if precision == "fp32" else errs["l2"] < 1e-2, errs


@pytest.mark.parametrize("head", list(HEADS))
def test_predict_at_chunks_and_classes(head):
    seed_all(5)
    enc = _encoder(head, dropout=0.1).cuda().train()   # predict_at runs the eval forward whatever the mode, and leaves the mode alone
    s, scene, table = _scene_and_table(head)
    scene = scene.cuda()
    one_cls, one = enc.predict_at(scene, table, return_logits=True)
    three_cls, three = enc.predict_at(scene, table.cuda(), return_logits=True, max_windows=3)
    assert enc.training
    assert one.shape == ((13, 5) if head == "pixelwise" else (13, 5, s, s)) and one_cls.dtype == torch.int64
    assert torch.equal(one, three) and torch.equal(one_cls, three_cls) and bool(torch.isfinite(one).all())
    assert torch.equal(one_cls, one.argmax(dim=1)) and torch.equal(enc.predict_at(scene, table), one_cls)
    enc.eval()
    with torch.no_grad():
        assert torch.equal(enc(stack_at(scene, table, s)), one)
    assert enc.predict_at(scene, table[:1], return_logits=True)[1].shape == ((1, 5) if head == "pixelwise" else (1, 5, s, s))   # never squeezed


def test_predict_at_is_predict_scene_at_the_listed_centres():
    """a pixelwise model: the dense map of predict_scene at stride 1 holds, at the centres of the listed windows, the logits of predict_at
    -- asserted bit for bit.

    The pixelwise head's logits kernel used to give a sample last bits that depended on whether its index in the launch was even or odd
    (a commuted first sum in one half of a packed multiply-add chain, msst_pixhead.hip: dot4): 10 of these 13 rows then differed from
    predict_scene's map by 1.6e-7 of the largest logit, since a window's number in predict_scene's chunk and its row in the table have the
    same parity for 2 rows only.  Also checked here: chunks of 1 and 3 windows, where every row's parity changes."""
    seed_all(5)
    enc = _encoder("pixelwise").cuda()
    s, scene, table = _scene_and_table("pixelwise")
    scene = scene.cuda()
    one_cls, one = enc.predict_at(scene, table, return_logits=True)
    classes, logits = enc.predict_scene(scene, stride=1, return_logits=True)
    sc, y, x = table.long().cuda().unbind(1)
    at_centres = logits[sc, :, y + s // 2, x + s // 2]
    nq = SCENE_HW[1] - s + 1
    number = sc * (SCENE_HW[0] - s + 1) * nq + y * nq + x   # the window's number in predict_scene's single chunk
    rows = (at_centres != one).any(dim=1)
    print("rows that differ", rows.int().tolist(), "slot parity differs", ((number - torch.arange(13, device="cuda")) % 2).tolist(),
          "largest difference relative to the largest logit", relerr(at_centres, one))
    assert torch.equal(classes[sc, y + s // 2, x + s // 2], one_cls)
    assert torch.equal(at_centres, one)
    for mw in (1, 3):
        assert torch.equal(enc.predict_at(scene, table, return_logits=True, max_windows=mw)[1], one), mw


# ------------------------------------------------------------------------------------------ train_step_at
def _finetune_script():
    spec = importlib.util.spec_from_file_location("finetune_script_at", os.path.join(ROOT, "finetune.py"))
    ft = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ft)
    return ft


# (head, loss): torch's CrossEntropyLoss over [n, nc, s, s] logits sums its forward with atomics on the device, so its loss value is not
# reproducible run to run; the patch head is therefore stepped with the HIP loss (finetune.py --loss fused), the pixelwise head with both
STEP_CASES = [("default", "fused"), ("pixelwise", "torch"), ("pixelwise", "fused")]


@pytest.mark.parametrize("optimizer", ["torch", "fused"])
@pytest.mark.parametrize("head,loss", STEP_CASES, ids=[f"{h}-loss_{l}" for h, l in STEP_CASES])
def test_train_step_at_is_the_step_on_the_stacked_copy(head, loss, optimizer):
    """one train_step_at step against train_step itself on the stacked copy of the same windows (windows of the model's size: train_step
    neither crops nor stacks), from the same initial state and dropout seeds, with both optimizers finetune.py offers: loss and every
    updated parameter, bit for bit"""
    from maskedsst_amd import centre_origins, window_labels
    from maskedsst_amd.config import Dotdict
    from maskedsst_amd.utils import train_step, train_step_at
    ft = _finetune_script()
    pix = head == "pixelwise"
    cfg = Dotdict(dict(image_size=8, patch_sub=1 if pix else 0, pixelwise=pix, ignored_label=-1, lr=1e-3, mlp_head_lr=3e-3,
                       weight_decay=1e-4, linear_eval=False))
    seed_all(5)
    s, scene, table = _scene_and_table(head)
    label_map = torch.randint(-1, 5, (2, *SCENE_HW))
    if pix:
        table, labels = centre_origins(label_map, s)
        pick = torch.randperm(table.shape[0])[:13]
        table, labels = table[pick], labels[pick]
    else:
        labels = window_labels(label_map, table, s)
    scene = scene.cuda()
    stacked = stack_at(scene, table, s)
    results = []
    for at in (True, False):
        seed_all(7)
        enc = _encoder(head, dropout=0.1).cuda().train()
        before = {k: q.detach().clone() for k, q in enc.named_parameters()}
        opt = ft.make_optimizer(enc, cfg, optimizer)
        criterion = ft.make_criterion(loss, -1)
        torch.manual_seed(3)
        if at:
            out = train_step_at(scene, labels, table, enc, cfg, criterion, opt)
        else:
            out = train_step(stacked, labels, enc, cfg, "cuda", criterion, opt)
        torch.cuda.synchronize()
        after = {k: q.detach().clone() for k, q in enc.named_parameters()}
        assert all(not torch.equal(after[k], before[k]) for k in after), [k for k in after if torch.equal(after[k], before[k])]
        results.append((out[0].detach().clone(), float(out[1]), after))
    (loss_at, acc_at, p_at), (loss_st, acc_st, p_st) = results
    print(head, loss, optimizer, "loss", loss_at.item(), loss_st.item(), "acc", acc_at, acc_st)
    bad = [k for k in p_at if not (torch.equal(p_at[k], p_st[k]) and bool(torch.isfinite(p_at[k]).all()))]
    assert not bad, bad
    assert bool(torch.isfinite(loss_at)) and torch.equal(loss_at, loss_st) and acc_at == acc_st
