"""Scene gradients through overlapping windows, host side (no GPU needed): ``maskedsst_amd.scene.origins_csr`` against a brute-force
dictionary, the C ABI of msst_tokenize_at_bwd_input / msst_scene_fold_at and their argument checks (they run before any HIP call, so
fake buffers and no device are enough to see them), ``scene_saliency``'s refusals on CPU tensors, and ``forward_at``'s refusal without the
opt-in."""
import os
import re
import subprocess

import pytest
import torch

from scene_grad_util import BS, HS, WS, overlap_table

BADARG, UNSUPPORTED = -3, -2   # include/msst.h: MSST_ERR_BADARG, MSST_ERR_UNSUPPORTED
CALLS = {"msst_tokenize_at_bwd_input": 20, "msst_scene_fold_at": 13}   # declared argument counts


def _csr_brute(rows, Bs, Hs, Ws):
    cells = {}
    for i, (s, y, x) in enumerate(rows):
        cells.setdefault((s * Hs + y) * Ws + x, []).append(i)
    ptr, win = [0], []
    for c in range(Bs * Hs * Ws):
        win += cells.get(c, [])   # ascending window number within a cell: the order they were appended in
        ptr.append(len(win))
    return ptr, win


@pytest.mark.parametrize("window", [8, 5, 1])
def test_origins_csr_is_the_brute_force_index(window):
    from maskedsst_amd.scene import origins_csr
    table = overlap_table(window)
    assert 13 <= table.shape[0] <= 40
    ptr, win = _csr_brute(table.tolist(), BS, HS, WS)
    for t in (table, table.long()):
        cell_ptr, cell_win = origins_csr(t, BS, HS, WS)
        assert cell_ptr.dtype == cell_win.dtype == torch.int32 and cell_ptr.shape == (BS * HS * WS + 1,) and cell_win.shape == (table.shape[0],)
        assert cell_ptr.tolist() == ptr and cell_win.tolist() == win
    assert max(b - a for a, b in zip(ptr, ptr[1:])) >= 2   # the repeated window: a cell that holds two
    assert sorted(win) == list(range(table.shape[0]))


def test_origins_csr_of_an_empty_table():
    from maskedsst_amd.scene import origins_csr
    cell_ptr, cell_win = origins_csr(torch.zeros(0, 3, dtype=torch.int32), 2, 5, 4)
    assert cell_ptr.dtype == cell_win.dtype == torch.int32
    assert cell_ptr.tolist() == [0] * 41 and cell_win.shape == (0,)


def test_c_abi_declares_and_exports_the_scene_gradient_calls():
    from maskedsst_amd import _lib
    header = open(_lib.HEADER_PATH).read()
    lib = _lib.load()
    assert lib.msst_version() == _lib.header_version() == 109   # additive: the revision stays
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name, nargs in CALLS.items():
        m = re.search(r"^int %s\(([^;]*)\);" % name, header, re.M)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(getattr(lib, name).argtypes), name
        assert name in _lib.declared_symbols() and re.search(r" T %s$" % name, out, re.M), name
    assert "Also under 109, on the same terms" in open(os.path.join(os.path.dirname(os.path.dirname(_lib.HEADER_PATH)), "INTEGRATION.md")).read()


def _at(lib, ptr=4096, origins=4096, **k):
    a = {**dict(Bs=2, Hs=19, Ws=17, window=8, nwin=13, S=3, P=10), **k}
    return lib.msst_tokenize_at_bwd_input(ptr, origins, *([ptr] * 8), a["Bs"], a["Hs"], a["Ws"], a["window"], a["nwin"], a["S"], a["P"],
                                          0.1, 7, None)


def _fold(lib, dwin=4096, cell_ptr=4096, cell_win=4096, dscene=4096, **k):
    a = {**dict(Bs=2, C=30, Hs=19, Ws=17, window=8, nwin=13, group=10, accumulate=0), **k}
    return lib.msst_scene_fold_at(dwin, cell_ptr, cell_win, dscene, a["Bs"], a["C"], a["Hs"], a["Ws"], a["window"], a["nwin"], a["group"],
                                  a["accumulate"], None)


def test_scene_gradient_calls_refuse_bad_arguments_before_launch():
    """fake, never dereferenced pointers (or none) and no device: no call can have reached a launch"""
    from maskedsst_amd import _lib
    lib = _lib.load()
    for bad in (dict(window=9, Hs=32, Ws=32), dict(P=17), dict(window=8, Hs=7), dict(window=8, Ws=7)):
        assert _at(lib, **bad) == UNSUPPORTED, bad
    for bad in (dict(Bs=0), dict(Hs=0), dict(Ws=0), dict(window=0), dict(S=0), dict(P=0), dict(nwin=-1)):
        assert _at(lib, **bad) == BADARG, bad
    assert _at(lib, ptr=None) == BADARG and _at(lib, origins=None) == BADARG
    assert b"msst_tokenize_at_bwd_input" in lib.msst_last_error()
    assert _at(lib, nwin=0) == 0   # an empty call enqueues nothing
    for bad in (dict(group=17), dict(window=9, Hs=32, Ws=32), dict(window=8, Hs=7), dict(window=8, Ws=7), dict(C=65536 * 16 + 1, group=16)):
        assert _fold(lib, **bad) == UNSUPPORTED, bad
    for bad in (dict(Bs=0), dict(C=0), dict(Hs=0), dict(Ws=0), dict(window=0), dict(group=0), dict(nwin=-1)):
        assert _fold(lib, **bad) == BADARG, bad
    for null in ("dwin", "cell_ptr", "cell_win", "dscene"):
        assert _fold(lib, **{null: None}) == BADARG, null
    assert b"msst_scene_fold_at" in lib.msst_last_error()
    assert _fold(lib, nwin=0, accumulate=1, dwin=None, cell_win=None) == 0   # nothing to add: no launch


def _model(**kw):
    from maskedsst_amd import ViTSpatialSpectral
    return ViTSpatialSpectral(
        **{**dict(image_size=8, spatial_patch_size=1, spectral_patch_size=10, num_classes=4, dim=96, depth=1, heads=2, mlp_dim=64, dropout=0.0,
                  emb_dropout=0.0, channels=30, spectral_pos_embed=False, spectral_pos=torch.arange(3), blockwise_patch_embed=True), **kw})


def test_forward_at_without_the_opt_in_still_refuses():
    scene = torch.zeros(BS, 30, HS, WS)
    table = overlap_table(8)
    for kw in (dict(), dict(scene_grad=False)):
        with pytest.raises(NotImplementedError, match="(?i)overlap"):
            _model().forward_at(scene.clone().requires_grad_(True), table, **kw)


def test_scene_saliency_refuses_bad_arguments_before_a_device_is_asked_for():
    from maskedsst_amd import scene_saliency, band_importance_scene
    m = _model()
    scene = torch.zeros(BS, 30, HS, WS)
    for stride in (0, 9, 2.5, True):
        with pytest.raises(ValueError, match="stride"):
            scene_saliency(m, scene, stride=stride)
    for target in (torch.zeros(BS, HS, dtype=torch.int64), torch.zeros(BS, WS, HS, dtype=torch.int64), torch.zeros(BS + 1, HS, WS, dtype=torch.int64),
                   torch.zeros(BS, HS, WS), [0, 1]):
        with pytest.raises(ValueError, match="target"):
            scene_saliency(m, scene, target=target)
    out_of_range = torch.zeros(BS, HS, WS, dtype=torch.int64)
    out_of_range[1, 3, 2] = 4
    for target in (4, -1, out_of_range):
        with pytest.raises(ValueError, match="class"):
            scene_saliency(m, scene, target=target)
    with pytest.raises(ValueError):
        scene_saliency(m, torch.zeros(BS, 20, HS, WS))
    with pytest.raises(ValueError, match="max_windows"):
        scene_saliency(m, scene, max_windows=0)
    with pytest.raises(ValueError, match="mode"):
        band_importance_scene(m, scene, mode="nope")
