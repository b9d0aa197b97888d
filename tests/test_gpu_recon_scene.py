"""GPU: whole-scene SimMIM reconstruction -- msst_tokenize_scene_fwd_masked bit for bit against the batch tokenizer on the copied
windows, SimMIMSpatialSpectral.reconstruct_scene bit for bit against reconstruct on the stacked windows where windows do not overlap,
within the rounding of k - 1 fp32 additions and one division of the float64 mean where they do, its tables against float64 sums over
the returned tensors, its independence of the split into chunks and of the module's mode, the C argument checks on device buffers,
pretrain.py --recon-tiles and tools/recon_time.py --scene.  The chain to the reference runs through reconstruct, which
test_gpu_recon.py pins to the oracle."""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT
from util import build_product, record

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # unit roundoff of fp32
BADARG, UNSUPPORTED = -3, -2

# the smallest shapes at which each piece can still go wrong (depth 1):
#   A  MFMA tokenizer (P = 10, 8 x 8); 399 pixels per plane: more than one pass of a 256-thread workgroup; uncovered trailing rows and
#      columns at stride 3 and 8; chunk boundaries in mid-row
#   B  generic tokenizer, N = 36 (idle lanes), a single window row, one window per launch
#   C  4-wave block kernel (2 heads), P at its limit, Ws = window
#   D  one window is the whole scene; planes below one wave
SHAPES = {
    "A": dict(cfg=dict(bands=20, depth=1, B=2, heads=8), scene=(2, 19, 21), strides=(8, 3, 1), max_windows=(3, None)),
    "B": dict(cfg=dict(bands=15, depth=1, B=1, heads=8, spectral_patch=5, image_size=6, mask_patch_size=2), scene=(1, 6, 13), strides=(6, 5), max_windows=(1, None)),
    "C": dict(cfg=dict(bands=64, depth=1, B=2, heads=2, spectral_patch=16, image_size=4, mask_patch_size=2), scene=(2, 9, 4), strides=(4, 2), max_windows=(None,)),
    "D": dict(cfg=dict(bands=20, depth=1, B=1, heads=8), scene=(1, 8, 8), strides=(8,), max_windows=(None,)),
}
MASKS = ("random", "all", "none", "column")
_models, _scenes = {}, {}


def model_of(shape, prec, per_block):
    key = (shape, prec, per_block)
    if key not in _models:
        cfg = dict(SHAPES[shape]["cfg"], to_pixels_per_spectral_block=bool(per_block))
        _models[key] = build_product(cfg, precision=prec, device="cuda")[0].eval()
    return _models[key]


def scene_of(shape):
    """(scene on the device, its CPU copy, {mask kind: bool [Bs, S, Hs, Ws]}): seeded, computed once per shape, read-only"""
    if shape not in _scenes:
        cfg, (Bs, Hs, Ws) = SHAPES[shape]["cfg"], SHAPES[shape]["scene"]
        S = cfg["bands"] // cfg.get("spectral_patch", 10)
        g = torch.Generator().manual_seed(7 + Hs * Ws)
        scene = torch.randn(Bs, cfg["bands"], Hs, Ws, generator=g)
        column = torch.zeros(Bs, S, Hs, Ws, dtype=torch.bool)
        column[:, :, :, Ws // 2] = True     # one dead detector column through every block
        masks = dict(random=torch.rand(Bs, S, Hs, Ws, generator=g) < 0.5, all=torch.ones(Bs, S, Hs, Ws, dtype=torch.bool),
                     none=torch.zeros(Bs, S, Hs, Ws, dtype=torch.bool), column=column)
        _scenes[shape] = (scene.cuda(), scene, masks)
    return _scenes[shape]


def window_of(model):
    return model.encoder.num_spatial_patches_sqrt


def stack(scene, w, stride):
    """the windows of scene [Bs, C, Hs, Ws] as a batch [Bs nr nq, C, w, w], in the kernels' window order (a copy)"""
    u = scene.unfold(2, w, stride).unfold(3, w, stride)     # [Bs, C, nr, nq, w, w]
    return u.permute(0, 2, 3, 1, 4, 5).reshape(-1, scene.shape[1], w, w).contiguous()


def reconstruct_batched(model, win, wm, blend, max_windows):
    """model.reconstruct on the stacked windows, in batches of max_windows windows (None: one batch) -> (cube [nwin, C, w, w],
    band_err [nwin, C], band_cnt [nwin, C]).  The batches are those of reconstruct_scene's chunks, because the encoder's last bits depend
    on them: the block kernels add a query's keys in the order of their rows in the 64-row tile, so where 64 // L sequences of
    length L do not fill tiles window by window (shape B: 36 spectral sequences of 3 tokens, 21 to a tile) a window's sums associate
    differently with its place in the batch -- predict_scene's chunk test records 2e-6 for it.  Shapes A, C and D fill whole tiles:
    any batching gives them the same bits (test_splits_mode_and_repetition_leave_every_bit)."""
    n = win.shape[0]
    step = n if max_windows is None else max_windows
    recs = [model.reconstruct(win[i:i + step].contiguous(), wm[i:i + step], blend=blend) for i in range(0, n, step)]
    return tuple(torch.cat([getattr(r, f) for r in recs]) for f in ("cube", "band_err", "band_cnt"))


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a) if a.dtype == torch.float32 else a, bits(b) if b.dtype == torch.float32 else b)


def check_tables(rec, noblend_cube, scene_cpu, tag):
    """band_cnt = the pixels of rec.mask per band; band_err within n 2^-53 relative of the float64 sum of |cube_noblend - scene| over
    them (the terms are exact in double, so only the order of the n additions differs), both from the returned tensors"""
    m = rec.mask.cpu()
    d = torch.where(m, (noblend_cube.cpu().double() - scene_cpu.double()).abs(), torch.zeros((), dtype=torch.float64))
    ref, n = d.sum(dim=(2, 3)), m.sum(dim=(2, 3))
    assert torch.equal(rec.band_cnt.cpu(), n.to(torch.int32)), tag
    err = rec.band_err.cpu()
    excess = (err - ref).abs() - n.double() * 2.0 ** -53 * ref
    print(f"{tag}: band_err worst |got - ref| / (n 2^-53 ref) = "
          f"{float(((err - ref).abs() / (n.double() * 2.0 ** -53 * ref).clamp(min=1e-300)).max()):.3e}")
    assert not (excess > 0).any(), (tag, float(excess.max()))
    assert (err[n == 0] == 0).all(), tag


# ------------------------------------------------------------------------------------------------------------------ 1. tokenizer
@pytest.mark.parametrize("shape", ["A", "B", "C"])
def test_masked_scene_tokenizer_gives_the_batch_tokenizers_bits(shape):
    model = model_of(shape, "fp32", 1)
    eng = model.engine()
    scene, _, masks = scene_of(shape)
    w = window_of(model)
    Bs, _, Hs, Ws = scene.shape
    S, N, P = eng.S, eng.N, eng.P
    for stride in SHAPES[shape]["strides"]:
        from maskedsst_amd import scene_mask_to_windows
        win = stack(scene, w, stride)
        nwin = win.shape[0]
        for kind in MASKS:
            m = masks[kind]
            want = eng.tokenize(win, scene_mask_to_windows(m, w, stride).to(device="cuda", dtype=torch.uint8).contiguous())
            out = torch.full((nwin, S * N, 96), float("nan"), device="cuda")
            eng.tokenize_scene_masked(scene, m.to(device="cuda", dtype=torch.uint8).contiguous(), stride, 0, nwin, out=out)
            assert same_bits(out, want), (shape, stride, kind)
            # a split in mid-row: the second half on its own
            half = nwin // 2
            out2 = torch.full((nwin - half, S * N, 96), float("nan"), device="cuda")
            eng.tokenize_scene_masked(scene, m.to(device="cuda", dtype=torch.uint8).contiguous(), stride, half, nwin - half, out=out2)
            assert same_bits(out2, want[half:]), (shape, stride, kind)
        # nothing masked: the bits of msst_tokenize_scene_fwd
        fp = eng.fp
        split, pos_a, pos_b = eng._pos_tables()
        V = ctypes.c_void_p
        plain = torch.full((nwin, S * N, 96), float("nan"), device="cuda")
        rc = eng.lib.msst_tokenize_scene_fwd(
            V(scene.data_ptr()), V(fp.ptr("pre_g")), V(fp.ptr("pre_b")), V(fp.ptr("embed.w.0")), V(fp.ptr("embed.b.0")),
            V(fp.ptr("post_g")), V(fp.ptr("post_b")), V(pos_a), V(pos_b), split, V(plain.data_ptr()), Bs, Hs, Ws, w, stride, 0, nwin, S, P,
            V(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        zero = eng.tokenize_scene_masked(scene, masks["none"].to(device="cuda", dtype=torch.uint8).contiguous(), stride, 0, nwin)
        assert same_bits(zero, plain), (shape, stride)
        assert not same_bits(out, plain)   # ... and the column mask does change tokens: the equality above is not vacuous


# ------------------------------------------------------------------------------------------------------- 2. stride == window
CASES = [(s, p, b) for s in SHAPES for p in ("fp32", "bf16") for b in (1, 0)]


@pytest.mark.parametrize("shape,prec,per_block", CASES)
def test_non_overlapping_windows_give_reconstructs_bits(shape, prec, per_block):
    """every covered pixel is covered once: the sum starts from nothing, one add, a division by 1 -- the bits of reconstruct on the
    stacked windows (reconstruct_batched: in the batches of the chunks), re-tiled"""
    from maskedsst_amd import scene_mask_to_windows
    model = model_of(shape, prec, per_block)
    scene, scene_cpu, masks = scene_of(shape)
    w = window_of(model)
    Bs, C, Hs, Ws = scene.shape
    nr, nq = Hs // w, Ws // w
    win = stack(scene, w, w)
    for kind in MASKS:
        m = masks[kind]
        wm = scene_mask_to_windows(m, w, w)
        recs = {}
        for blend in (True, False):
            for mw in SHAPES[shape]["max_windows"]:
                rec = model.reconstruct_scene(scene, m, stride=w, blend=blend, max_windows=mw)
                ref_cube, _, ref_cnt = reconstruct_batched(model, win, wm, blend, mw)
                tag = f"{shape} {prec} per_block={per_block} {kind} blend={blend} max_windows={mw}"
                assert rec.cube.shape == rec.mask.shape == (Bs, C, Hs, Ws) and rec.cube.dtype == torch.float32 and rec.mask.dtype == torch.bool
                assert rec.band_err.shape == rec.band_cnt.shape == (Bs, C) and rec.cover.shape == (Bs, Hs, Ws)
                assert (rec.band_err.dtype, rec.band_cnt.dtype, rec.cover.dtype) == (torch.float64, torch.int32, torch.int32)
                tiled = ref_cube.view(Bs, nr, nq, C, w, w).permute(0, 3, 1, 4, 2, 5).reshape(Bs, C, nr * w, nq * w)
                assert same_bits(rec.cube[:, :, :nr * w, :nq * w], tiled), tag
                assert torch.equal(rec.band_cnt, ref_cnt.view(Bs, nr * nq, C).sum(1, dtype=torch.int32)), tag
                cover = torch.zeros(Bs, Hs, Ws, dtype=torch.int32, device="cuda")
                cover[:, :nr * w, :nq * w] = 1
                assert torch.equal(rec.cover, cover), tag
                unc = (cover == 0)[:, None].expand(Bs, C, Hs, Ws)
                if blend:
                    assert torch.equal(bits(rec.cube)[unc], bits(scene)[unc]), tag     # uncovered: the input's bits
                else:
                    assert torch.isnan(rec.cube[unc]).all() and not torch.isnan(rec.cube[~unc]).any(), tag   # ... or absent
                P = C // m.shape[1]
                counted = (m.cuda() & (cover > 0)[:, None]).repeat_interleave(P, dim=1)
                assert torch.equal(rec.mask, counted), tag
                recs[blend] = rec
        assert torch.equal(recs[True].band_err, recs[False].band_err) and torch.equal(recs[True].band_cnt, recs[False].band_cnt)
        for blend in (True, False):
            check_tables(recs[blend], recs[False].cube, scene_cpu, f"{shape} {prec} per_block={per_block} {kind} blend={blend}")


# ------------------------------------------------------------------------------------------------------------------ 3. overlap
def fold(p, Bs, Hs, Ws, w, stride):
    """float64 per-pixel sum, sum of magnitudes and count of the per-window predictions p [nwin, C, w, w] (CPU)"""
    from maskedsst_amd.scene import scene_windows
    C = p.shape[1]
    s1 = torch.zeros(Bs, C, Hs, Ws, dtype=torch.float64)
    sa = torch.zeros(Bs, C, Hs, Ws, dtype=torch.float64)
    k = torch.zeros(Bs, Hs, Ws, dtype=torch.int32)
    org = scene_windows(Hs, Ws, w, stride)
    pd = p.double()
    for s in range(Bs):
        for i, (y0, x0) in enumerate(org):
            s1[s, :, y0:y0 + w, x0:x0 + w] += pd[s * len(org) + i]
            sa[s, :, y0:y0 + w, x0:x0 + w] += pd[s * len(org) + i].abs()
            k[s, y0:y0 + w, x0:x0 + w] += 1
    return s1, sa, k


@pytest.mark.parametrize("shape,prec,per_block", [c for c in CASES if c[0] != "D"])
def test_overlapping_windows_are_averaged(shape, prec, per_block):
    """against the float64 mean of the per-window reconstruct(blend=False) predictions p_1 .. p_k of each pixel:
    |cube - mean| <= (k + 1) 2^-24 (sum |p_i|) / k -- k - 1 fp32 additions and one division, to first order, with one unit of slack
    (the predictions taken in the batches of the chunks: reconstruct_batched)"""
    from maskedsst_amd import scene_mask_to_windows
    model = model_of(shape, prec, per_block)
    scene, scene_cpu, masks = scene_of(shape)
    w = window_of(model)
    Bs, C, Hs, Ws = scene.shape
    for stride in SHAPES[shape]["strides"]:
        if stride == w:
            continue
        win = stack(scene, w, stride)
        for kind in MASKS:
            m = masks[kind]
            mw = SHAPES[shape]["max_windows"][0]
            p = reconstruct_batched(model, win, scene_mask_to_windows(m, w, stride), False, mw)[0].cpu()
            s1, sa, k = fold(p, Bs, Hs, Ws, w, stride)
            kk = k[:, None].expand(Bs, C, Hs, Ws)
            cov = kk > 0
            recs = {}
            for blend in (True, False):
                rec = model.reconstruct_scene(scene, m, stride=stride, blend=blend, max_windows=mw)
                tag = f"{shape} {prec} per_block={per_block} stride={stride} {kind} blend={blend}"
                assert torch.equal(rec.cover.cpu(), k), tag
                P = C // m.shape[1]
                me = m.repeat_interleave(P, dim=1)
                assert torch.equal(rec.mask.cpu(), me & cov), tag
                recs[blend] = rec
            cube = recs[False].cube.cpu()
            assert torch.isnan(cube[~cov]).all() and not torch.isnan(cube[cov]).any()
            kd = kk.double().clamp(min=1)
            dev = (cube.double() - s1 / kd).abs()[cov]
            bound = ((kd + 1) * U * sa / kd)[cov]
            ratio = float((dev / bound.clamp(min=1e-300)).max())
            print(f"{shape} {prec} per_block={per_block} stride={stride} {kind}: worst |cube - mean| / bound = {ratio:.3e} (k up to {int(k.max())})")
            assert not (dev > bound).any(), (shape, prec, stride, kind, ratio)
            blended = recs[True].cube.cpu()
            keep = ~(me & cov)      # not masked, or uncovered: the input's bits
            assert torch.equal(bits(blended)[keep], bits(scene_cpu)[keep])
            assert torch.equal(bits(blended)[me & cov], bits(cube)[me & cov])
            assert torch.equal(recs[True].band_err, recs[False].band_err) and torch.equal(recs[True].band_cnt, recs[False].band_cnt)
            for blend in (True, False):
                check_tables(recs[blend], cube, scene_cpu, f"{shape} {prec} per_block={per_block} stride={stride} {kind} blend={blend}")
            record("recon_scene_overlap", shape=shape, prec=prec, per_block=per_block, stride=stride, mask=kind, ratio_to_bound=ratio)


# ------------------------------------------------------------------------------------------------- 4. splits and determinism
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_splits_mode_and_repetition_leave_every_bit(prec):
    cfg = dict(SHAPES["A"]["cfg"])
    model = build_product(cfg, precision=prec, device="cuda")[0]
    model.encoder.dropout_p = model.encoder.emb_dropout_p = 0.1   # build_product builds without dropout: switch both sites on
    scene, _, masks = scene_of("A")
    m = masks["random"]
    for stride in (3, 8):
        for blend in (True, False):
            model.train()
            first = model.reconstruct_scene(scene, m, stride=stride, blend=blend)
            assert model.training and model.encoder.training
            model.eval()
            others = [model.reconstruct_scene(scene, m, stride=stride, blend=blend, max_windows=mw) for mw in (1, 3, None, None)]
            assert not model.training and not model.encoder.training
            torch.cuda.synchronize()
            for other in others:
                for name, a, b in zip(first._fields, first, other):
                    assert same_bits(a, b), (prec, stride, blend, name)
            assert not any(t.requires_grad for t in first)
    assert all(p.grad is None for p in model.parameters())
    model.train()   # ... and training mode does apply dropout to forward itself, so the equality above is not vacuous
    win = stack(scene, 8, 8)
    fm = model.draw_masks(win.shape[0])
    with torch.no_grad():
        assert float(model(win, masks=fm)) != float(model(win, masks=fm))


# ------------------------------------------------------------------------------------------------------------- 5. mask=None
def test_drawn_masks_are_placed_in_scene_coordinates():
    from maskedsst_amd import window_masks_to_scene
    model = model_of("A", "fp32", 1)
    scene, _, _ = scene_of("A")
    Bs, C, Hs, Ws = scene.shape
    S = model.encoder.num_spectral_patches
    model.last_masks = None
    rec = model.reconstruct_scene(scene)
    assert model.last_masks is not None and model.last_masks[0].shape == (Bs * 2 * 2, model.encoder.num_patches)
    m = window_masks_to_scene(model.last_masks[0], Bs, S, Hs, Ws, 8)
    again = model.reconstruct_scene(scene, m, stride=8)
    for name, a, b in zip(rec._fields, rec, again):
        assert same_bits(a, b), name
    assert int(rec.band_cnt.sum()) == int(model.last_masks[0].sum()) * model.pixel_values_per_patch
    kept = model.last_masks
    for stride in (7, 3):
        with pytest.raises(ValueError, match="stride must be 8"):
            model.reconstruct_scene(scene, stride=stride)
    assert model.last_masks is kept


# ---------------------------------------------------------------------------------------------------------------- 6. report
def test_recon_report_of_a_scene_equals_that_of_the_stacked_windows():
    from maskedsst_amd import recon_report, scene_mask_to_windows
    model = model_of("A", "bf16", 1)
    scene, _, masks = scene_of("A")
    P = model.pixel_values_per_patch
    a = recon_report(model.reconstruct_scene(scene, masks["random"], stride=8), P)
    b = recon_report(model.reconstruct(stack(scene, 8, 8), scene_mask_to_windows(masks["random"], 8, 8)), P)
    assert a.masked == b.masked > 0
    assert abs(a.mae - b.mae) <= 1e-12 * abs(b.mae), (a.mae, b.mae)
    assert torch.equal(a.band_present, b.band_present) and a.block_mae.shape == b.block_mae.shape


# -------------------------------------------------------------------------------------------------------- 7. argument checks
def test_c_calls_refuse_bad_arguments_and_touch_nothing():
    model = model_of("A", "fp32", 1)
    eng = model.engine()
    eng.ensure()
    lib, fp = eng.lib, eng.fp
    scene, _, masks = scene_of("A")
    Bs, C, Hs, Ws = scene.shape
    S, N, P, w = eng.S, eng.N, eng.P, 8
    V = ctypes.c_void_p
    st = V(torch.cuda.current_stream().cuda_stream)
    mask_u8 = masks["random"].to(device="cuda", dtype=torch.uint8).contiguous()
    SENT = 12345.0
    out = torch.full((4, S * N, 96), SENT, device="cuda")
    split, pos_a, pos_b = eng._pos_tables()

    def tok(scene_p=scene.data_ptr(), mt=fp.ptr("mask_token"), mk=mask_u8.data_ptr(), out_p=out.data_ptr(), Hs_=Hs, window=w, stride=3,
            win0=0, nwin=4, S_=S, P_=P):
        return lib.msst_tokenize_scene_fwd_masked(
            V(scene_p), V(fp.ptr("pre_g")), V(fp.ptr("pre_b")), V(fp.ptr("embed.w.0")), V(fp.ptr("embed.b.0")), V(fp.ptr("post_g")),
            V(fp.ptr("post_b")), V(pos_a), V(pos_b), split, V(mt), V(mk), V(out_p), Bs, Hs_, Ws, window, stride, win0, nwin, S_, P_, st)

    per_scene = 4 * 5   # 19 x 21 at stride 3
    for kw in (dict(scene_p=0), dict(mt=0), dict(mk=0), dict(out_p=0), dict(S_=0), dict(P_=0), dict(nwin=-1), dict(win0=-1), dict(stride=0),
               dict(stride=9), dict(Hs_=7), dict(win0=Bs * per_scene - 3), dict(nwin=Bs * per_scene + 1)):
        assert tok(**kw) == BADARG, kw
    assert tok(window=9, stride=9) == UNSUPPORTED
    torch.cuda.synchronize()
    assert (out == SENT).all()
    assert tok() == 0 and tok(nwin=0) == 0
    torch.cuda.synchronize()
    assert not (out == SENT).any()

    win_recon = torch.zeros(4, C, N, device="cuda")
    cube = torch.full((Bs, C, Hs, Ws), SENT, device="cuda")
    err = torch.full((Bs, C), SENT, dtype=torch.float64, device="cuda")
    cnt = torch.full((Bs, C), 12345, dtype=torch.int32, device="cuda")
    cover = torch.full((Bs, Hs, Ws), 12345, dtype=torch.int32, device="cuda")
    ptr = dict(win_recon=win_recon, scene=scene, scene_mask=mask_u8, cube=cube, band_err=err, band_cnt=cnt, cover=cover)

    def asm(win0=0, nwin=4, Bs_=Bs, S_=S, P_=P, Hs_=Hs, Ws_=Ws, window=w, stride=3, finalize=1, blend=1, null=()):
        a = {k: V(0 if k in null else t.data_ptr()) for k, t in ptr.items()}
        return lib.msst_scene_recon_assemble(a["win_recon"], win0, nwin, a["scene"], a["scene_mask"], a["cube"], a["band_err"], a["band_cnt"],
                                             a["cover"], Bs_, S_, P_, Hs_, Ws_, window, stride, finalize, blend, st)

    for kw in (dict(Bs_=0), dict(S_=0), dict(P_=-1), dict(Hs_=0), dict(Ws_=0), dict(window=0), dict(stride=0), dict(nwin=-1), dict(win0=-1)):
        assert asm(**kw) == BADARG, kw
    for kw in (dict(stride=9), dict(window=9, stride=9), dict(Hs_=7), dict(Ws_=7), dict(S_=65), dict(P_=17)):
        assert asm(**kw) == UNSUPPORTED, kw
    for k in ("win_recon", "scene", "scene_mask", "cube", "cover", "band_err", "band_cnt"):
        assert asm(null=(k,)) == BADARG, k
    assert asm(win0=Bs * per_scene - 3) == BADARG and asm(nwin=Bs * per_scene + 1) == BADARG
    torch.cuda.synchronize()
    assert (cube == SENT).all() and (err == SENT).all() and (cnt == 12345).all() and (cover == 12345).all()
    # a call that is not the finalizing one writes sums only; statistics may be absent as a pair
    assert asm(finalize=0) == 0
    torch.cuda.synchronize()
    assert (err == SENT).all() and (cnt == 12345).all() and (cover == 12345).all() and not (cube == SENT).all()
    assert asm(win0=4, nwin=0, null=("win_recon", "band_err", "band_cnt")) == 0
    torch.cuda.synchronize()
    assert (err == SENT).all() and (cnt == 12345).all() and not (cover == 12345).any()


# ---------------------------------------------------------------------------------------------------------------- 8. scripts
def child(cmd, timeout):
    """a script in a fresh child process under its own time limit.  A child that timed out or died of a signal (a GPU fault, an abort)
    ends the session: nothing more is started on the device after it."""
    e = dict(os.environ)
    e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
    try:
        r = subprocess.run(cmd, cwd=ROOT, env=e, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as t:
        pytest.exit(f"{' '.join(cmd)} timed out after {timeout} s: no further GPU work\n{(t.stderr or '')[-2000:]}", returncode=1)
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        pytest.exit(f"{' '.join(cmd)} ended with {r.returncode}: no further GPU work\n{r.stderr[-3000:]}", returncode=1)
    assert r.returncode == 0, f"--- stdout\n{r.stdout[-3000:]}\n--- stderr\n{r.stderr[-3000:]}"
    return r.stdout


def test_recon_time_scene_script(tmp_path):
    """tools/recon_time.py --scene at a small shape: exit 0, ONE JSON line with both paths' times, the same line appended to --append"""
    log = str(tmp_path / "t.jsonl")
    out = child([sys.executable, os.path.join("tools", "recon_time.py"), "--scene", "--steps", "2", "--warmup", "1", "--reps", "2",
                 "--tiles", "2", "--tile-size", "20", "--bands", "50", "--depth", "1", "--append", log], 300)
    lines = [l for l in out.splitlines() if l.strip()]
    assert len(lines) == 1, out
    row = json.loads(lines[0])
    assert [json.loads(l) for l in open(log)] == [row]
    assert row["tool"] == "recon_scene_time" and row["tiles"] == 2 and row["tile_size"] == 20 and row["windows"] == 8 and row["bands"] == 50
    assert len(row["reconstruct_scene_ms"]) == len(row["stacked_ms"]) == 2
    for k in ("reconstruct_scene_ms", "stacked_ms"):
        assert all(v > 0 for v in row[k]), (k, row)
    assert row["assemble_kernels_ms"] > 0 and row["masked_tokenizer_ms"] > 0
    assert row["cube_equal"] and row["assembled_equal"] and row["band_cnt_equal"] and row["max_rel_band_err_diff"] < 1e-12


def test_pretrain_recon_tiles_script():
    """pretrain.py --synthetic --recon-tiles at a tiny size: one more line per validation pass, over every window of the tiles"""
    out = child([sys.executable, "pretrain.py", "--synthetic", "--batch-size", "8", "--tiles", "8", "--epochs", "1", "--pool-tiles", "8",
                 "--depth", "1", "--val-tiles", "1", "--recon-tiles"], 600)
    lines = [l for l in out.splitlines() if " recon tiles masked_mae " in l]
    assert len(lines) == 1, out
    f = lines[0].split()
    assert f[:2] == ["epoch", "0"] and float(f[5]) > 0
    # one 64 x 64 tile of 200 bands: 64 windows of 1280 tokens, the same number of masked tokens in each (tube masks), 10 bands per
    # token -- and more pixels than ONE window holds (12800): the line covers the whole tile
    n = int(f[7])
    assert n % (64 * 10) == 0 and 12800 < n < 64 * 1280 * 10, lines[0]
    assert "worst bands" in lines[0] and not any(" recon masked_mae " in l for l in out.splitlines())
