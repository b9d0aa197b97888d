"""Scene inference, host side: window enumeration, validation metrics, the C ABI of the two scene entry points and the
argument checks of predict_scene (no GPU needed)."""
import ctypes
import math
import os
import re

import pytest
import torch

from conftest import ROOT


def notebook_windows(Hs, Ws, window, stride):
    """The window loop of the reference's inference_example.ipynb, restated for any scene size and step: x over rows
    (outer), y over columns (inner), windows that do not fit skipped."""
    out = []
    for x in range(0, Hs, stride):
        for y in range(0, Ws, stride):
            if x + window > Hs or y + window > Ws:
                continue
            out.append((x, y))
    return out


@pytest.mark.parametrize("Hs,Ws,window,stride", [
    (64, 64, 8, 8),     # the notebook's tiling
    (40, 44, 8, 8),     # non-square, last columns uncovered
    (21, 30, 8, 8),     # sizes not a multiple of the window
    (64, 64, 8, 3),     # overlapping windows
    (19, 17, 8, 5),
    (12, 9, 6, 1),      # stride 1
    (8, 8, 8, 8),       # one window
    (7, 20, 8, 8),      # no window fits
])
def test_scene_windows_match_notebook_loop(Hs, Ws, window, stride):
    from maskedsst_amd.scene import scene_windows
    assert scene_windows(Hs, Ws, window, stride) == notebook_windows(Hs, Ws, window, stride)


def test_scene_windows_grid_shape():
    from maskedsst_amd.scene import scene_windows
    for Hs, Ws, w, s in [(64, 64, 8, 8), (40, 44, 8, 3), (9, 30, 6, 1)]:
        ws = scene_windows(Hs, Ws, w, s)
        nr, nq = (Hs - w) // s + 1, (Ws - w) // s + 1
        assert len(ws) == nr * nq
        if nr > 1:
            assert ws[nq] == (s, 0)   # row-major: window nq starts the second window row


def _maps():
    # 1 scene, 3 classes, 2 x 3 pixels; pixel (1, 2) uncovered (class -1), pixel (0, 1) labelled ignore
    logits = torch.tensor([[[[2.0, 0.0, 1.0], [0.0, 0.0, 0.0]],
                            [[1.0, 3.0, 0.0], [2.0, 0.0, 0.0]],
                            [[0.0, 1.0, 5.0], [1.0, 4.0, 0.0]]]])
    classes = torch.tensor([[[0, 1, 2], [1, 2, -1]]])
    labels = torch.tensor([[[0, -1, 1], [1, 2, 0]]])
    return logits, classes, labels


def test_scene_metrics_hand_built():
    import torch.nn.functional as F
    from maskedsst_amd.scene import scene_metrics
    logits, classes, labels = _maps()
    m = scene_metrics(logits, classes, labels)
    # counted pixels: (0,0) label 0 pred 0, (0,2) label 1 pred 2, (1,0) label 1 pred 1, (1,1) label 2 pred 2
    rows = torch.tensor([[2.0, 1.0, 0.0], [1.0, 0.0, 5.0], [0.0, 2.0, 1.0], [0.0, 0.0, 4.0]])
    want_loss = float(F.cross_entropy(rows, torch.tensor([0, 1, 1, 2])))
    assert m.loss == pytest.approx(want_loss, rel=1e-6)
    assert m.acc == pytest.approx(3 / 4)
    # recall: class 0 1/1, class 1 1/2, class 2 1/1
    assert m.macro_acc == pytest.approx((1 + 0.5 + 1) / 3)
    loss, acc, macro = m   # a plain tuple too
    assert (loss, acc, macro) == (m.loss, m.acc, m.macro_acc)


def test_scene_metrics_other_ignore_index_and_empty():
    from maskedsst_amd.scene import scene_metrics
    logits, classes, labels = _maps()
    labels = labels.clone()
    labels[labels == -1] = 7
    m = scene_metrics(logits, classes, labels, ignore_index=7)
    assert m.acc == pytest.approx(3 / 4)
    # nothing counts: every pixel uncovered or ignored
    m = scene_metrics(logits, torch.full_like(classes, -1), labels)
    assert all(math.isnan(v) for v in m)


def test_header_declares_scene_entry_points():
    from maskedsst_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "msst.h")).read()
    for name in ("msst_tokenize_scene_fwd", "msst_scene_assemble"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.declared_symbols()
    assert _lib.header_version() >= 105


def test_library_exports_scene_entry_points():
    from maskedsst_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "msst_tokenize_scene_fwd") and hasattr(lib, "msst_scene_assemble")
    loaded = _lib.load()
    assert loaded.msst_version() == _lib.header_version()


def test_scene_entry_points_refuse_bad_arguments():
    """Argument checks happen on the host before anything is enqueued (no device needed): MSST_ERR_BADARG (-3) for an
    inconsistent (scene, window, stride) triple or a window range outside the grid, MSST_ERR_UNSUPPORTED (-2) for a window of
    more than 64 pixels."""
    from maskedsst_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)   # never dereferenced: every call below is refused before a launch
    P = [fake] * 9

    def tok(Bs, Hs, Ws, w, s, win0, nwin, scene=fake, out=fake):
        return lib.msst_tokenize_scene_fwd(scene, *P[1:], 0, out, Bs, Hs, Ws, w, s, win0, nwin, 5, 10, None)

    assert tok(1, 16, 16, 8, 0, 0, 1) == -3         # stride 0
    assert tok(1, 16, 16, 8, 9, 0, 1) == -3         # stride > window
    assert tok(1, 7, 16, 8, 8, 0, 1) == -3          # scene smaller than a window
    assert tok(1, 16, 16, 8, 8, 0, 5) == -3         # 4 windows in the grid
    assert tok(1, 16, 16, 8, 8, -1, 1) == -3
    assert tok(1, 16, 16, 8, 8, 0, 1, scene=None) == -3
    assert tok(1, 20, 20, 9, 9, 0, 1) == -2         # 81 pixels per window

    def asm(Bs, Hs, Ws, w, s, win0, nwin, fin=1, classes=fake, wl=fake):
        return lib.msst_scene_assemble(wl, win0, nwin, fake, classes, Bs, 8, Hs, Ws, w, s, fin, None)

    assert asm(2, 16, 16, 8, 0, 0, 1) == -3
    assert asm(2, 16, 16, 8, 8, 0, 9) == -3         # 8 windows in the grid
    assert asm(2, 16, 16, 8, 8, 0, 1, classes=None) == -3
    assert asm(2, 16, 16, 8, 8, 0, 1, wl=None) == -3
    assert asm(2, 4, 16, 8, 8, 0, 1) == -3
    assert "msst_scene_assemble" in lib.msst_last_error().decode()


def _cpu_encoder():
    from maskedsst_amd import ViTSpatialSpectral
    return ViTSpatialSpectral(image_size=8, spatial_patch_size=1, spectral_patch_size=10, num_classes=4, dim=96, depth=1,
                              heads=8, mlp_dim=64, channels=20, spectral_pos_embed=False, spectral_pos=torch.arange(2))


@pytest.mark.parametrize("shape,kw", [
    ((1, 30, 16, 16), {}),                    # wrong band count
    ((1, 20, 7, 16), {}),                     # smaller than a window
    ((1, 20, 16, 5), {}),
    ((20, 16, 16), {}),                       # not 4-D
    ((1, 20, 16, 16), {"stride": 0}),
    ((1, 20, 16, 16), {"stride": 9}),
    ((1, 20, 16, 16), {"stride": 2.5}),
    ((1, 20, 16, 16), {"max_windows": 0}),
])
def test_predict_scene_rejects_bad_input(shape, kw):
    enc = _cpu_encoder()
    with pytest.raises(ValueError):
        enc.predict_scene(torch.zeros(shape), **kw)
