"""GPU: scene gradients through overlapping windows.  msst_tokenize_at_bwd_input bit for bit against msst_tokenize_bwd_input on the
gathered windows; msst_scene_fold_at bit for bit against its sequential restatement on the CPU (tests/scene_grad_util.py) and within the
derived bound of a float64 sum; forward_at(..., scene_grad=True) against forward on the stacked windows; the oracle's autograd through the
gathered windows; and scene_saliency against manual autograd, for every max_windows."""
import ctypes

import pytest
import torch

from conftest import seed_all
from input_grad_util import build_model, fixture, oracle_logits
from scene_grad_util import BS, HS, WS, cover_of, fold_restatement, grid_table, overlap_table, stack_at
from util import record, relerr

pytestmark = pytest.mark.gpu

D = 96
UNSUPPORTED = -2


def _V(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib():
    from maskedsst_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------------------------------ 1. the per-window kernel
def _tok_weights(P, S, gen):
    r = lambda *shape: torch.randn(*shape, device="cuda", generator=gen)   # noqa: E731
    return [1 + 0.3 * r(P), 0.2 * r(P), 0.4 * r(S, D, P), 0.1 * r(S, D), 1 + 0.3 * r(D), 0.2 * r(D)]


def _bwd_input(lib, w, img, dx0, P, p, seed):
    B, C, N = img.shape[0], img.shape[1], img.shape[2] * img.shape[3]
    out = torch.full((B, C, N), float("nan"), device="cuda")
    rc = lib.msst_tokenize_bwd_input(_V(img), *[_V(t) for t in w], None, _V(dx0), None, _V(out), B, C // P, N, P, p, seed, _stream())
    assert rc == 0
    return out


def _at_bwd_input(lib, w, scene, table, window, dx0, P, p, seed, expect=0):
    Bs, C, Hs, Ws = scene.shape
    assert table.is_cuda and table.dtype == torch.int32 and table.is_contiguous()
    out = torch.full((table.shape[0], C, window * window), float("nan"), device="cuda")
    rc = lib.msst_tokenize_at_bwd_input(_V(scene), _V(table), *[_V(t) for t in w], _V(dx0), _V(out), Bs, Hs, Ws, window, table.shape[0],
                                        C // P, P, p, seed, _stream())
    assert rc == expect
    return out


@pytest.mark.parametrize("P", [1, 5, 10, 16])
def test_listed_input_gradient_is_the_stacked_one(P):
    lib = _lib()
    S = 3
    gen = torch.Generator(device="cuda").manual_seed(100 + P)
    w = _tok_weights(P, S, gen)
    scene = torch.randn(BS, S * P, HS, WS, device="cuda", generator=gen)
    for window in (1, 5, 8):
        table = overlap_table(window)
        stacked = stack_at(scene, table, window)
        dx0 = torch.randn(table.shape[0], S * window * window, D, device="cuda", generator=gen)
        for p, seed in ((0.0, 0), (0.1, 12345)):
            want = _bwd_input(lib, w, stacked, dx0, P, p, seed)
            got = _at_bwd_input(lib, w, scene, table.cuda(), window, dx0, P, p, seed)
            again = _at_bwd_input(lib, w, scene, table.cuda(), window, dx0, P, p, seed)
            torch.cuda.synchronize()
            # (P = 1: a LayerNorm over one pixel is constant, its input gradient is exactly zero)
            assert bool(torch.isfinite(got).all()) and (float(got.abs().max()) > 0 or P == 1), (window, p)
            assert torch.equal(got, want) and torch.equal(again, got), (window, p)
        assert P == 1 or not torch.equal(got, _bwd_input(lib, w, stacked, dx0, P, 0.0, 0))   # the dropout was on


def test_refused_listed_input_gradient_writes_nothing():
    lib = _lib()
    gen = torch.Generator(device="cuda").manual_seed(3)
    table = overlap_table(8).cuda()
    scene = torch.randn(BS, 3 * 17, HS, WS, device="cuda", generator=gen)
    w = _tok_weights(17, 3, gen)
    dx0 = torch.randn(table.shape[0], 3 * 64, D, device="cuda", generator=gen)
    out = _at_bwd_input(lib, w, scene, table, 8, dx0, 17, 0.0, 0, expect=UNSUPPORTED)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


# ------------------------------------------------------------------------------------------ 2. the fold
def _fold(lib, dwin, table, window, group, out=None, accumulate=0, fill=float("nan")):
    from maskedsst_amd.scene import origins_csr
    C = dwin.shape[1]
    cell_ptr, cell_win = origins_csr(table.cuda(), BS, HS, WS)
    if out is None:
        out = torch.full((BS, C, HS, WS), fill, device="cuda")
    rc = lib.msst_scene_fold_at(_V(dwin), _V(cell_ptr), _V(cell_win), _V(out), BS, C, HS, WS, window, table.shape[0], group, accumulate,
                                _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("C,group", [(30, 10), (50, 16)], ids=["30b_group10", "50b_group16_tail"])
@pytest.mark.parametrize("window", [8, 5, 1])
def test_fold_gives_the_bits_of_the_sequential_restatement(window, C, group):
    lib = _lib()
    table = overlap_table(window)
    gen = torch.Generator(device="cuda").manual_seed(10 * window + C)
    dwin = torch.randn(table.shape[0], C, window * window, device="cuda", generator=gen)
    got = _fold(lib, dwin, table, window, group)
    want, _ = fold_restatement(dwin, table, BS, HS, WS, window)
    cover = cover_of(table, BS, HS, WS, window)
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got.cpu(), want)
    uncovered = (cover == 0)[:, None].expand_as(want)
    assert bool(uncovered.any()) and float(got.cpu()[uncovered].abs().max()) == 0.0
    assert int(cover.max()) >= 3 or window == 1
    # a second call over memory full of NaN, accumulate = 0: defined whole again
    assert torch.equal(_fold(lib, dwin, table, window, group, out=torch.full_like(got, float("nan"))), got)
    # accumulate over this table: the running map's values are where the sums start, untouched pixels keep theirs
    start = torch.randn(BS, C, HS, WS, device="cuda", generator=gen)
    acc = _fold(lib, dwin, table, window, group, out=start.clone(), accumulate=1)
    want_acc, _ = fold_restatement(dwin, table, BS, HS, WS, window, start=start)
    assert torch.equal(acc.cpu(), want_acc) and torch.equal(acc.cpu()[uncovered], start.cpu()[uncovered])
    # against float64: |got - want| <= (m - 1) 2^-24 sum |addends|, m the pixel's cover count (m - 1 rounded additions, each within
    # half an ulp of a partial sum that the sum of |addends| bounds)
    want64, mag64 = fold_restatement(dwin, table, BS, HS, WS, window, dtype=torch.float64)
    bound = (cover[:, None].double() - 1).clamp(min=0) * 2.0 ** -24 * mag64
    err = (got.cpu().double() - want64).abs()
    print("fold vs float64: largest error / bound", float((err / bound.clamp(min=1e-300)).max()))
    assert bool((err <= bound).all())


@pytest.mark.parametrize("window,stride", [(8, 3), (5, 1), (8, 8)])
def test_fold_of_a_grid_split_into_calls_keeps_every_bit(window, stride):
    lib = _lib()
    table = grid_table(window, stride)
    n, C = table.shape[0], 30
    gen = torch.Generator(device="cuda").manual_seed(n)
    dwin = torch.randn(n, C, window * window, device="cuda", generator=gen)
    one = _fold(lib, dwin, table, window, 10)
    assert torch.equal(one.cpu(), fold_restatement(dwin, table, BS, HS, WS, window)[0])
    for cuts in ((n // 2,), (n // 3, n - 5), (1, 2)):
        out = torch.full_like(one, float("nan"))
        bounds = (0, *cuts, n)
        for k, (i0, i1) in enumerate(zip(bounds, bounds[1:])):
            _fold(lib, dwin[i0:i1].contiguous(), table[i0:i1], window, 10, out=out, accumulate=int(k > 0))
        assert torch.equal(out, one), cuts


# ------------------------------------------------------------------------------------------ 3. autograd
HEADS = ["default", "spectral", "pixelwise"]


def _encoder(head, precision="fp32", dropout=0.0, depth=1):
    """30 bands; patch heads: 8 x 8 windows; pixelwise: the fixture's model (5 x 5 windows, its seed-5 parameters) with the dropout set"""
    if head == "pixelwise":
        model, _, _ = build_model("pixwise_30b_L1_B3_img5_h2", precision)
        model.dropout_p = model.emb_dropout_p = dropout
        return model
    from maskedsst_amd import ViTSpatialSpectral
    return ViTSpatialSpectral(
        image_size=8, spatial_patch_size=1, spectral_patch_size=10, num_classes=5, dim=96, depth=depth, heads=2, mlp_dim=64,
        dropout=dropout, emb_dropout=dropout, channels=30, spectral_pos_embed=False, spectral_pos=torch.arange(3),
        blockwise_patch_embed=True, precision=precision, spectral_mlp_head=head == "spectral")


def _window(head):
    return 5 if head == "pixelwise" else 8


def _param_grads(model):
    return {k: q.grad.clone() for k, q in model.named_parameters() if q.grad is not None}


@pytest.mark.parametrize("regime", ["train_full", "train_linear_eval", "eval"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("head", HEADS)
def test_scene_grad_is_the_fold_of_the_stacked_input_gradient(head, precision, regime):
    seed_all(5)
    enc = _encoder(head, precision, dropout=0.1).cuda()
    assert enc.dropout_p == 0.1 and enc.emb_dropout_p == 0.1
    if regime == "train_linear_eval":
        for n, q in enc.named_parameters():
            q.requires_grad_("mlp_head" in n)
    enc.train(regime != "eval")
    w = _window(head)
    table = overlap_table(w)
    scene = torch.randn(BS, 30, HS, WS).cuda()
    n, nc = table.shape[0], enc.num_classes
    cot = torch.randn((n, nc) if head == "pixelwise" else (n, nc, w, w), device="cuda")

    def run(fwd, x):
        enc.zero_grad(set_to_none=True)
        torch.manual_seed(11)   # pins the step's dropout seeds
        out = fwd(x)
        (out * cot).sum().backward()
        torch.cuda.synchronize()
        return out.detach().clone(), x.grad, _param_grads(enc)

    xs = scene.clone().requires_grad_(True)
    out_s, g_s, p_s = run(lambda x: enc.forward_at(x, table, scene_grad=True), xs)
    xw = stack_at(scene, table, w).requires_grad_(True)
    out_w, g_w, p_w = run(enc, xw)
    out_d, g_d, p_d = run(lambda x: enc.forward_at(x, table), scene.clone())             # the scene detached
    out_2, g_2, _ = run(lambda x: enc.forward_at(x, table.cuda(), check=False, scene_grad=True), scene.clone().requires_grad_(True))
    assert torch.equal(out_s, out_w) and torch.equal(out_s, out_d) and g_d is None
    want, _ = fold_restatement(g_w.reshape(n, 30, w * w), table, BS, HS, WS, w)
    assert g_s is not None and g_s.shape == scene.shape and g_s.dtype == torch.float32
    assert bool(torch.isfinite(g_s).all()) and float(g_s.abs().max()) > 0
    assert torch.equal(g_s.cpu(), want)
    assert torch.equal(g_2, g_s) and torch.equal(out_2, out_s)   # a second run: the same bits
    uncovered = (cover_of(table, BS, HS, WS, w) == 0)[:, None].expand_as(want)
    assert float(g_s.cpu()[uncovered].abs().max()) == 0.0
    trainable = sorted(k for k, q in enc.named_parameters() if q.requires_grad)
    assert sorted(p_s) == sorted(p_d) == sorted(p_w) == trainable and trainable
    bad = [k for k in trainable if not (torch.equal(p_s[k], p_d[k]) and torch.equal(p_s[k], p_w[k]))]
    assert not bad, bad
    if regime != "eval":
        with torch.no_grad():
            assert not torch.equal(out_s, enc.eval().forward_at(scene, table))   # the dropout was on


@pytest.mark.parametrize("head", HEADS)
def test_frozen_eval_model_gives_scene_grad(head):
    seed_all(5)
    enc = _encoder(head, depth=2).cuda().eval()
    for q in enc.parameters():
        q.requires_grad_(False)
    table = overlap_table(_window(head))
    scene = torch.randn(BS, 30, HS, WS).cuda().requires_grad_(True)
    enc.forward_at(scene, table, scene_grad=True).square().mean().backward()
    assert scene.grad is not None and bool(torch.isfinite(scene.grad).all()) and float(scene.grad.abs().max()) > 0
    assert all(q.grad is None for q in enc.parameters())
    with pytest.raises(NotImplementedError, match="(?i)overlap"):
        enc.forward_at(scene, table)


# ------------------------------------------------------------------------------------------ 4. against the oracle
ORACLE_CASES = {"default": "cls_50b_L2_B2_specpos", "spectral": None, "pixelwise": "pixwise_30b_L1_B3_img5_h2"}


@pytest.mark.parametrize("head", HEADS)
def test_scene_grad_fp32_matches_the_oracle(head):
    """the oracle's autograd on the CPU through the gathered windows (indexing the scene: its autograd sums the overlaps); relerr <= 2e-4,
    the project's bar for fp32 input gradients (test_gpu_input_grad.py::test_img_grad_fp32_matches_oracle)"""
    name = ORACLE_CASES[head]
    if name is not None:
        model, params, _ = build_model(name)
        cfg = fixture(name)["cfg"]
    else:
        seed_all(5)
        model = _encoder("spectral", depth=2)
        params = {"encoder." + k: v.detach().clone() for k, v in model.state_dict().items()}
        cfg = dict(bands=30, depth=2, heads=2, n_classes=5, image_size=8, spectral_mlp_head=True, spectral_pos_embed=False)
    w, bands = cfg["image_size"], cfg["bands"]
    table = overlap_table(w)
    gen = torch.Generator().manual_seed(7)
    scene = torch.randn(BS, bands, HS, WS, generator=gen)
    xo = scene.clone().requires_grad_(True)
    ref = oracle_logits(params, stack_at(xo, table, w), cfg)
    cot = torch.randn(ref.shape, generator=gen)
    (ref * cot).sum().backward()
    xs = scene.cuda().requires_grad_(True)
    out = model.cuda().eval().forward_at(xs, table, scene_grad=True)
    (out.reshape(ref.shape) * cot.cuda()).sum().backward()
    torch.cuda.synchronize()
    err = relerr(xs.grad, xo.grad)
    print(f"scene_grad fp32 {head}: relerr {err:.4e}")
    record("scene_grad_fp32", head=head, err=err)
    assert relerr(out.reshape(ref.shape), ref) < 1e-4
    assert err <= 2e-4, err


# ------------------------------------------------------------------------------------------ 5. scene_saliency
SALIENCY_CASES = [("default", 8), ("default", 3), ("spectral", 3), ("pixelwise", 1), ("pixelwise", 2)]


def _manual_saliency(enc, scene, stride, tmap):
    """autograd over forward_at(scene_grad=True) on the whole grid: score = sum over pixels of weight x the logit at the target class"""
    from util import host_fold
    for q in enc.parameters():   # the frozen model scene_saliency runs
        q.requires_grad_(False)
        q.grad = None
    w, pix = enc.num_spatial_patches_sqrt, bool(getattr(enc, "pixelwise", False))
    table = grid_table(w, stride)
    n = table.shape[0]
    if pix:
        cover = torch.zeros(BS, HS, WS, dtype=torch.int32)
        for s, y, x in table.tolist():
            cover[s, y + w // 2, x + w // 2] += 1
    else:
        cover = host_fold(torch.zeros(n, 1, w * w), BS, HS, WS, w, stride)[2]
    weight = torch.where((cover > 0) & (tmap.cpu() >= 0), 1.0 / cover.clamp(min=1).float(), torch.zeros(()))
    tcl = tmap.cpu().clamp(min=0)
    x = scene.clone().requires_grad_(True)
    out = enc.forward_at(x, table, scene_grad=True)
    if pix:
        at = [(s, y + w // 2, x0 + w // 2) for s, y, x0 in table.tolist()]
        idx = torch.tensor([int(tcl[a]) for a in at]).view(n, 1)
        wgt = torch.stack([weight[a] for a in at]).view(n, 1)
        out = out.view(n, -1)
    else:
        idx = torch.stack([tcl[s, y:y + w, x0:x0 + w] for s, y, x0 in table.tolist()]).view(n, 1, w, w)
        wgt = torch.stack([weight[s, y:y + w, x0:x0 + w] for s, y, x0 in table.tolist()]).view(n, 1, w, w)
    (out.gather(1, idx.cuda()) * wgt.cuda()).sum().backward()
    return x.grad, cover


@pytest.mark.parametrize("head,stride", SALIENCY_CASES, ids=[f"{h}-stride{s}" for h, s in SALIENCY_CASES])
def test_scene_saliency_is_manual_autograd_for_every_chunking(head, stride):
    from maskedsst_amd import band_importance_scene, scene_saliency
    seed_all(5)
    enc = _encoder(head, dropout=0.1).cuda().train()   # scene_saliency runs the eval forward whatever the mode, and leaves the mode alone
    flags = []
    for i, q in enumerate(enc.parameters()):
        q.requires_grad_(i % 3 != 0)
        q.grad = torch.full_like(q, 2.0) if i % 2 else None
        flags.append((q.requires_grad, q.grad))
    scene = torch.randn(BS, 30, HS, WS).cuda()
    sal = scene_saliency(enc, scene, stride=stride)
    assert enc.training and not scene.requires_grad
    for q, (f, g) in zip(enc.parameters(), flags):
        assert q.requires_grad == f and q.grad is g and (g is None or float((g - 2.0).abs().max()) == 0.0)
    classes = enc.predict_scene(scene, stride=stride)
    assert sal.grad.shape == scene.shape and sal.grad.dtype == torch.float32 and sal.classes.dtype == torch.int64 and sal.cover.dtype == torch.int32
    assert torch.equal(sal.classes, classes) and torch.equal(sal.cover > 0, classes != -1)
    assert bool(torch.isfinite(sal.grad).all()) and float(sal.grad.abs().max()) > 0
    enc.eval()
    manual, cover = _manual_saliency(enc, scene, stride, classes)
    enc.train()
    assert torch.equal(sal.cover.cpu(), cover)
    assert torch.equal(sal.grad, manual)
    for mw in (1, 7):
        assert torch.equal(scene_saliency(enc, scene, stride=stride, max_windows=mw).grad, sal.grad), mw
    # pixels outside every window: zero gradient (a pixelwise model's windows reach beyond the pixels that count)
    w = _window(head)
    reach = cover_of(grid_table(w, stride), BS, HS, WS, w)
    outside = (reach == 0)[:, None].expand_as(sal.grad)
    assert not bool(outside.any()) or float(sal.grad.cpu()[outside].abs().max()) == 0.0
    # targets: an int is that class everywhere; a map with -1 skips pixels; band_importance_scene sums gradient x input
    enc.eval()
    three = scene_saliency(enc, scene, target=3, stride=stride)
    assert torch.equal(three.grad, _manual_saliency(enc, scene, stride, torch.full_like(classes, 3))[0])
    tmap = classes.clone()
    tmap[0] = -1
    part = scene_saliency(enc, scene, target=tmap, stride=stride, max_windows=7)
    assert torch.equal(part.grad, _manual_saliency(enc, scene, stride, tmap)[0])
    assert float(part.grad[0].abs().max()) == 0.0 and float(part.grad[1].abs().max()) > 0   # no pixel of scene 0 counts
    bands = band_importance_scene(enc, scene, stride=stride)
    assert bands.shape == (BS, 30) and torch.equal(bands, (sal.grad * scene).flatten(2).sum(dim=2))


def test_scene_saliency_windows_at_the_scene_border_stride_8():
    """stride 8 on 19 x 17: rows 16.. and column 16 are in no window -- zero gradient, class -1, cover 0"""
    from maskedsst_amd import scene_saliency
    seed_all(5)
    enc = _encoder("default").cuda().eval()
    sal = scene_saliency(enc, torch.randn(BS, 30, HS, WS).cuda())
    assert float(sal.grad[:, :, 16:].abs().max()) == 0.0 and float(sal.grad[:, :, :, 16:].abs().max()) == 0.0
    assert bool((sal.classes[:, 16:] == -1).all()) and bool((sal.cover[:, :16, :16] == 1).all()) and int(sal.cover[:, 16:].max()) == 0
    assert float(sal.grad[:, :, :16, :16].abs().min()) > 0.0
