"""Whole-scene SimMIM reconstruction, host side (no GPU needed): the two mask helpers against a plain loop over scene_windows and
against the reference-made window order, the ValueErrors of reconstruct_scene that need no device, the C ABI of
msst_tokenize_scene_fwd_masked / msst_scene_recon_assemble (additive under MSST_VERSION 109) and their argument checks (they run before
any HIP call, so host buffers and no device are enough to see them), recon_report on a hand-built SceneReconstruction, and the flags
of pretrain.py."""
import ctypes
import math
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import ROOT, load_golden
from util import build_product

BADARG, UNSUPPORTED = -3, -2   # include/msst.h: MSST_ERR_BADARG, MSST_ERR_UNSUPPORTED
CALLS = ("msst_tokenize_scene_fwd_masked", "msst_scene_recon_assemble")


# ------------------------------------------------------------------------------------------------------------------ mask helpers
def loop_windows(mask, window, stride):
    """scene_mask_to_windows restated as the plain loop over scene_windows"""
    from maskedsst_amd.scene import scene_windows
    Bs, S, Hs, Ws = mask.shape
    rows = []
    for s in range(Bs):
        for y0, x0 in scene_windows(Hs, Ws, window, stride):
            rows.append(torch.stack([mask[s, c, y0 + n // window, x0 + n % window] for c in range(S) for n in range(window * window)]))
    return torch.stack(rows)


@pytest.mark.parametrize("Hs,Ws,w,stride", [(19, 21, 8, 8), (19, 21, 8, 3), (9, 10, 8, 1), (6, 13, 6, 5), (9, 4, 4, 2), (8, 8, 8, 8)])
def test_scene_mask_to_windows_against_the_loop(Hs, Ws, w, stride):
    from maskedsst_amd import scene_mask_to_windows
    from maskedsst_amd.scene import scene_windows
    g = torch.Generator().manual_seed(Hs * 100 + Ws + stride)
    mask = torch.rand(2, 3, Hs, Ws, generator=g) < 0.5
    got = scene_mask_to_windows(mask, w, stride)
    assert got.dtype == torch.bool and got.shape == (2 * len(scene_windows(Hs, Ws, w, stride)), 3 * w * w)
    assert torch.equal(got, loop_windows(mask, w, stride))


@pytest.mark.parametrize("Hs,Ws,w", [(19, 21, 8), (6, 13, 6), (9, 4, 4), (8, 8, 8), (16, 16, 8)])
def test_window_masks_round_trip(Hs, Ws, w):
    from maskedsst_amd import scene_mask_to_windows, window_masks_to_scene
    from maskedsst_amd.scene import scene_windows
    Bs, S = 2, 3
    org = scene_windows(Hs, Ws, w, w)
    g = torch.Generator().manual_seed(Hs + Ws)
    bm = torch.rand(Bs * len(org), S * w * w, generator=g) < 0.5
    scene = window_masks_to_scene(bm, Bs, S, Hs, Ws, w)
    assert scene.dtype == torch.bool and scene.shape == (Bs, S, Hs, Ws)
    # against the plain loop, and unmasked where no window covers the pixel
    want = torch.zeros(Bs, S, Hs, Ws, dtype=torch.bool)
    for s in range(Bs):
        for i, (y0, x0) in enumerate(org):
            want[s, :, y0:y0 + w, x0:x0 + w] = bm[s * len(org) + i].view(S, w, w)
    assert torch.equal(scene, want)
    nr, nq = Hs // w, Ws // w
    assert not scene[:, :, nr * w:].any() and not scene[:, :, :, nq * w:].any()
    assert torch.equal(window_masks_to_scene(bm, Bs, S, Hs, Ws, w, stride=w), scene)   # the default stride is the window
    # inverses on the covered area
    assert torch.equal(scene_mask_to_windows(scene, w, w), bm)
    full = torch.rand(Bs, S, Hs, Ws, generator=g) < 0.5
    back = window_masks_to_scene(scene_mask_to_windows(full, w, w), Bs, S, Hs, Ws, w)
    assert torch.equal(back[:, :, :nr * w, :nq * w], full[:, :, :nr * w, :nq * w])


def test_mask_helpers_refuse():
    from maskedsst_amd import scene_mask_to_windows, window_masks_to_scene
    bm = torch.zeros(2 * 4, 3 * 64, dtype=torch.bool)
    for stride in (7, 1):
        with pytest.raises(ValueError, match="stride == window"):
            window_masks_to_scene(bm, 2, 3, 16, 16, 8, stride=stride)
    for bad in (bm[:-1], bm[:, :-1], bm.float()):
        with pytest.raises(ValueError):
            window_masks_to_scene(bad, 2, 3, 16, 16, 8)
    with pytest.raises(ValueError):
        window_masks_to_scene(bm, 2, 3, 7, 16, 8)          # the scene is smaller than a window
    m = torch.zeros(2, 3, 16, 16, dtype=torch.bool)
    for bad in (m[0], m.float()):
        with pytest.raises(ValueError):
            scene_mask_to_windows(bad, 8, 8)
    for stride in (0, 9, 2.5, True):
        with pytest.raises(ValueError):
            scene_mask_to_windows(m, 8, stride)
    with pytest.raises(ValueError):
        scene_mask_to_windows(m, 17, 1)


@pytest.mark.parametrize("case", ["s8", "s7"])
def test_window_order_is_the_reference_stack_order(case):
    """the reference-made fixture of stack_image_batch: window i of scene_mask_to_windows holds the pixels of stacked sample i"""
    from maskedsst_amd import scene_mask_to_windows
    g = load_golden("stack_image_batch.npz")
    image_size, patch_sub = (int(v) for v in g[case + "_cfg"])
    w = image_size - patch_sub
    img, stacked = g[case + "_img"], g[case + "_stacked_img"]     # [B, C, H, W] -> [B nr nq, C, w, w], distinct integers
    for bit in range(3):   # three bit planes of the pixel values, as bool masks with the bands as the block axis
        m = torch.from_numpy(((img >> bit) & 1).astype(bool))
        want = torch.from_numpy(((stacked >> bit) & 1).astype(bool)).reshape(stacked.shape[0], -1)
        assert torch.equal(scene_mask_to_windows(m, w, w), want)


# ----------------------------------------------------------------------------------------------------------- reconstruct_scene
CFG = dict(bands=20, depth=1, B=2, heads=2)


def test_reconstruct_scene_checks_then_refuses_the_cpu():
    model, _, _ = build_product(CFG)
    S = model.encoder.num_spectral_patches
    scene = torch.randn(2, 20, 19, 21)
    mask = torch.zeros(2, S, 19, 21, dtype=torch.bool)
    for bad in (scene[0], scene[:, :10], scene[:, :, :7], scene[:, :, :, :7], scene[:0], "scene"):
        with pytest.raises(ValueError):
            model.reconstruct_scene(bad)
    for bad in (mask[:1], mask[:, :1], mask[:, :, :8], mask.float(), mask.to(torch.uint8), mask.view(2, S, 21, 19), [mask]):
        with pytest.raises(ValueError, match="mask must be a bool"):
            model.reconstruct_scene(scene, bad)
    for stride in (0, 9, 2.5, True, -1):
        with pytest.raises(ValueError, match="stride"):
            model.reconstruct_scene(scene, mask, stride=stride)
    for mw in (0, -3, 1.5, True):
        with pytest.raises(ValueError, match="max_windows"):
            model.reconstruct_scene(scene, mask, max_windows=mw)
    # random window masks need non-overlapping windows
    model.last_masks = None
    for stride in (1, 3, 7):
        with pytest.raises(ValueError, match="stride must be 8"):
            model.reconstruct_scene(scene, stride=stride)
    assert model.last_masks is None
    model.train()
    for kw in (dict(mask=mask), dict(mask=mask, stride=3, blend=False, max_windows=3), dict(), dict(stride=8)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            model.reconstruct_scene(scene, **kw)
    assert model.training
    nwin = 2 * 2 * 2   # 19 x 21 holds 2 x 2 windows of 8 x 8
    assert model.last_masks is not None and model.last_masks[0].shape == (nwin, model.encoder.num_patches)
    # a bare encoder has neither a mask token nor to_pixels
    assert not hasattr(model.encoder, "reconstruct_scene")


def test_recon_report_on_a_scene_reconstruction():
    from maskedsst_amd import recon_report, SceneReconstruction
    assert SceneReconstruction._fields == ("cube", "mask", "band_err", "band_cnt", "cover")
    # 2 scenes x 4 bands (two spectral blocks of 2 bands); band 2 has no masked pixel in either scene
    rec = SceneReconstruction(torch.zeros(2, 4, 3, 3), torch.zeros(2, 4, 3, 3, dtype=torch.bool),
                              torch.tensor([[1.0, 2.0, 0.0, 4.0], [3.0, 0.0, 0.0, 4.0]], dtype=torch.float64),
                              torch.tensor([[2, 4, 0, 1], [2, 0, 0, 3]], dtype=torch.int32), torch.ones(2, 3, 3, dtype=torch.int32))
    r = recon_report(rec, 2)
    assert r.masked == 12 and r.mae == 14.0 / 12.0
    assert r.band_mae[[0, 1, 3]].tolist() == [1.0, 0.5, 2.0] and math.isnan(float(r.band_mae[2]))
    assert r.worst_bands == [3, 0, 1] and r.block_mae.tolist() == [6.0 / 8.0, 8.0 / 4.0]


# --------------------------------------------------------------------------------------------------------------------- C ABI
def test_c_abi_declares_and_exports_the_entry_points():
    from maskedsst_amd import _lib
    header = open(_lib.HEADER_PATH).read()
    assert _lib.header_version() == 109   # additive: the revision does not move
    lib = _lib.load()
    assert lib.msst_version() == 109
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in CALLS:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in _lib.declared_symbols()
        assert re.search(r" T %s$" % name, out, re.M), name
    import maskedsst_amd
    for name in ("SceneReconstruction", "window_masks_to_scene", "scene_mask_to_windows"):
        assert name in maskedsst_amd.__all__ and hasattr(maskedsst_amd, name)


def _ptr():
    buf = (ctypes.c_char * 64)()
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)


def test_tokenize_scene_fwd_masked_refuses_bad_arguments_before_launch():
    """the checks of msst_tokenize_scene_fwd, plus a null mask_token or scene_mask; host memory stands in for the device buffers: a
    refused call dereferences nothing and launches nothing"""
    from maskedsst_amd import _lib
    lib = _lib.load()
    buf, p = _ptr()

    def call(fn="msst_tokenize_scene_fwd_masked", scene=p, out=p, mask_token=p, scene_mask=p, Bs=2, Hs=19, Ws=21, window=8, stride=3,
             win0=0, nwin=4, S=2, P=10):
        if fn == "msst_tokenize_scene_fwd":
            return lib.msst_tokenize_scene_fwd(scene, p, p, p, p, p, p, p, None, 0, out, Bs, Hs, Ws, window, stride, win0, nwin, S, P, None)
        return lib.msst_tokenize_scene_fwd_masked(scene, p, p, p, p, p, p, p, None, 0, mask_token, scene_mask, out, Bs, Hs, Ws, window,
                                                  stride, win0, nwin, S, P, None)

    bad = [dict(scene=None), dict(out=None), dict(S=0), dict(P=0), dict(nwin=-1), dict(win0=-1), dict(Bs=0), dict(window=0),
           dict(stride=0), dict(stride=9), dict(Hs=7), dict(Ws=7), dict(win0=2 * 4 * 5 - 3), dict(nwin=2 * 4 * 5 + 1)]
    for kw in bad:   # 19 x 21 at stride 3: 4 x 5 windows per scene
        assert call(**kw) == BADARG == call("msst_tokenize_scene_fwd", **kw), kw
    assert b"msst_tokenize_scene_fwd_masked" in (call(S=0), lib.msst_last_error())[1]
    assert call(window=9, stride=9, Hs=20) == UNSUPPORTED == call("msst_tokenize_scene_fwd", window=9, stride=9, Hs=20)
    assert call(mask_token=None) == BADARG and call(scene_mask=None) == BADARG
    assert call(mask_token=None, window=9, stride=9, Hs=20) == BADARG


def test_scene_recon_assemble_refuses_bad_arguments_before_launch():
    from maskedsst_amd import _lib
    lib = _lib.load()
    buf, p = _ptr()
    names = ["win_recon", "scene", "scene_mask", "cube", "band_err", "band_cnt", "cover"]

    def call(win0=0, nwin=4, Bs=2, S=2, P=10, Hs=19, Ws=21, window=8, stride=3, finalize=1, blend=1, **null):
        a = {k: (None if null.get(k) else p) for k in names}
        return lib.msst_scene_recon_assemble(a["win_recon"], win0, nwin, a["scene"], a["scene_mask"], a["cube"], a["band_err"],
                                             a["band_cnt"], a["cover"], Bs, S, P, Hs, Ws, window, stride, finalize, blend, None)

    for dim in ("Bs", "S", "P", "Hs", "Ws", "window", "stride"):
        for v in (0, -1):
            assert call(**{dim: v}) == BADARG, (dim, v)
    assert call(nwin=-1) == BADARG and call(win0=-1) == BADARG
    assert b"msst_scene_recon_assemble" in lib.msst_last_error()
    all_null = {k: True for k in names}
    for over in (dict(stride=9), dict(window=9, stride=9, Hs=20), dict(Hs=7), dict(Ws=7), dict(S=65), dict(P=17), dict(window=20, Hs=20, Ws=20)):
        assert call(**over) == UNSUPPORTED and call(**over, **all_null) == UNSUPPORTED, over   # decided by the sizes alone
    assert call(S=64, P=16, **all_null) == BADARG              # the limits themselves are inside
    assert call(S=65, P=0) == BADARG                           # a size below 1 wins over a size beyond the kernel
    for k in ("win_recon", "scene", "scene_mask", "cube", "cover"):
        assert call(**{k: True}) == BADARG, k
    assert call(band_err=True) == BADARG and call(band_cnt=True) == BADARG   # statistics: both or neither
    assert call(win0=2 * 4 * 5 - 3) == BADARG and call(nwin=2 * 4 * 5 + 1) == BADARG   # windows beyond Bs nr nq (4 x 5 per scene)
    assert b"out of range" in lib.msst_last_error()


# ------------------------------------------------------------------------------------------------------------------- scripts
def test_pretrain_parser_takes_recon_tiles():
    import pretrain
    ap = pretrain.build_parser()
    a = ap.parse_args([])
    assert a.recon_tiles is False and a.recon_report is False
    a = ap.parse_args(["--recon-tiles"])
    assert a.recon_tiles is True and a.recon_report is False


def test_product_still_does_not_import_oracle():
    code = ("import sys; sys.path.insert(0, %r); import maskedsst_amd, maskedsst_amd.engine, maskedsst_amd.recon, maskedsst_amd.scene; "
            "assert not any(m == 'oracle' or m.startswith('oracle.') for m in sys.modules), 'oracle imported'" % ROOT)
    subprocess.run([sys.executable, "-c", code], check=True)
    for f in ("recon.py", "vit_simmim_original.py", "engine.py"):
        src = open(os.path.join(ROOT, "maskedsst_amd", f)).read()
        assert "import oracle" not in src and "from oracle" not in src, f
