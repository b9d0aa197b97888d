"""D4 augmentation of listed windows, host side (no GPU needed): orient_windows against the normative torch expression, window_labels
and random_orients, the refusals of forward_at / predict_at / SimMIM forward_at on CPU tensors (they come before a device is asked
for), ResidentTileLoader(augment="d4"), train_step_at on a stub model, the scripts' flag checks, and the C ABI of the five _orient
entry points with their argument checks (they run before any HIP call: fake buffers and no device are enough to see them)."""
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

BADARG, UNSUPPORTED = -3, -2   # include/msst.h: MSST_ERR_BADARG, MSST_ERR_UNSUPPORTED
# declared argument counts: the namesake's plus the orientation table
CALLS = {"msst_tokenize_at_fwd_orient": 23, "msst_tokenize_at_bwd_orient": 31, "msst_tokenize_at_fwd_masked_orient": 23,
         "msst_tokenize_at_bwd_masked_orient": 31, "msst_head_at_fwd_orient": 21}


def _normative(w, o):
    k, f = o & 3, o >> 2
    return torch.rot90(torch.flip(w, (-1,)) if f else w, k, (-2, -1))


# ------------------------------------------------------------------------------------------ the helpers
@pytest.mark.parametrize("s", [1, 2, 7, 8])
def test_orient_windows_is_the_torch_expression_and_inverse_undoes_it(s):
    from maskedsst_amd import orient_windows
    g = torch.Generator().manual_seed(s)
    orient = torch.cat([torch.arange(8), torch.tensor([5, 5, 0, 3])])
    for x in (torch.randn(12, 3, s, s, generator=g), torch.randint(-1, 9, (12, s, s), generator=g), torch.randn(12, 2, 3, s, s, generator=g)):
        got = orient_windows(x, orient)
        assert got.shape == x.shape and got.dtype == x.dtype
        for i, o in enumerate(orient.tolist()):
            assert torch.equal(got[i], _normative(x[i], o)), (s, i, o)
        assert torch.equal(orient_windows(got, orient, inverse=True), x)
        assert torch.equal(orient_windows(orient_windows(x, orient, inverse=True), orient), x)
        assert torch.equal(orient_windows(x, torch.zeros(12, dtype=torch.uint8)), x)   # code 0 is the identity
        assert torch.equal(orient_windows(x, orient.to(torch.uint8)), got) and torch.equal(orient_windows(x, orient.int()), got)
    if s > 1:   # the eight orientations of a generic window are eight different windows
        w = torch.randn(1, s, s, generator=g).expand(8, s, s).contiguous()
        assert len({orient_windows(w, torch.arange(8))[o].numpy().tobytes() for o in range(8)}) == 8


def test_orient_windows_refuses_bad_arguments():
    from maskedsst_amd import orient_windows
    x = torch.zeros(4, 3, 8, 8)
    for bad in (torch.zeros(4, 1, dtype=torch.int64), torch.zeros(3, dtype=torch.int64), torch.zeros(5, dtype=torch.int64),
                torch.zeros(4), [0, 0, 0, 0]):
        with pytest.raises(ValueError, match="orient"):
            orient_windows(x, bad)
    for bad_x in (torch.zeros(4, 8), torch.zeros(4, 7, 8)):
        with pytest.raises(ValueError):
            orient_windows(bad_x, torch.zeros(4, dtype=torch.int64))


@pytest.mark.parametrize("window", [8, 7])
def test_window_labels_orient_is_orient_windows_of_window_labels(window):
    from maskedsst_amd import orient_windows, random_origins, random_orients, window_labels
    g = torch.Generator().manual_seed(2)
    labels = torch.randint(-1, 6, (2, 17, 12), generator=g)   # not square
    origins = random_origins(2, 17, 12, window, 40, generator=g)
    orient = random_orients(40, generator=g)
    got = window_labels(labels, origins, window, orient)
    plain = window_labels(labels, origins, window)
    assert got.dtype == torch.int64 and got.shape == (40, window, window)
    assert torch.equal(got, orient_windows(plain, orient))
    for i, ((b, y, x), o) in enumerate(zip(origins.tolist(), orient.tolist())):
        assert torch.equal(got[i], _normative(labels[b, y:y + window, x:x + window], o)), i
    assert torch.equal(window_labels(labels, origins, window, orient=None), plain)
    if window % 2:   # the centre of an odd window is a fixed point of every orientation
        assert torch.equal(got[:, window // 2, window // 2], plain[:, window // 2, window // 2])


def test_random_orients():
    from maskedsst_amd import random_orients
    a = random_orients(4000, generator=torch.Generator().manual_seed(7))
    b = random_orients(4000, generator=torch.Generator().manual_seed(7))
    c = random_orients(4000, generator=torch.Generator().manual_seed(8))
    assert a.dtype == torch.uint8 and a.shape == (4000,) and a.device.type == "cpu"
    assert torch.equal(a, b) and not torch.equal(a, c)
    counts = torch.bincount(a.long(), minlength=8)
    assert counts.numel() == 8 and int(counts.min()) > 400   # 0 .. 7, every code about 500 times
    assert random_orients(0).shape == (0,) and random_orients(3, device="cpu").dtype == torch.uint8
    with pytest.raises(ValueError):
        random_orients(-1)


# ------------------------------------------------------------------------------------------ refusals of the model methods
def _model(**kw):
    from maskedsst_amd import ViTSpatialSpectral
    return ViTSpatialSpectral(
        **{**dict(image_size=8, spatial_patch_size=1, spectral_patch_size=10, num_classes=4, dim=96, depth=1, heads=2, mlp_dim=64, dropout=0.0,
                  emb_dropout=0.0, channels=20, spectral_pos_embed=False, spectral_pos=torch.arange(2), blockwise_patch_embed=True), **kw})


def _mim():
    from maskedsst_amd import SimMIMSpatialSpectral
    return SimMIMSpatialSpectral(encoder=_model(), masking_ratio=0.7, mask_patch_size=4, tube_masking=True)


GOOD = torch.tensor([[0, 0, 0], [1, 8, 4], [1, 3, 2]], dtype=torch.int32)   # scenes [2, 20, 16, 12]: y0 <= 8, x0 <= 4
CODES = torch.tensor([0, 7, 3], dtype=torch.uint8)


def _scene():
    return torch.zeros(2, 20, 16, 12)


def _bad_tables():
    return (CODES.view(3, 1), CODES[:2], torch.cat([CODES, CODES[:1]]), CODES.float(), CODES.tolist())


def test_forward_at_refuses_bad_orientation_tables():
    m, mim = _model(), _mim()
    for bad in _bad_tables():
        for check in (True, False):   # shape and dtype are checked without reading the table
            with pytest.raises(ValueError, match="orient"):
                m.forward_at(_scene(), GOOD, check=check, orient=bad)
            with pytest.raises(ValueError, match="orient"):
                mim.forward_at(_scene(), GOOD, check=check, orient=bad)
        with pytest.raises(ValueError, match="orient"):
            m.predict_at(_scene(), GOOD, orient=bad)


@pytest.mark.parametrize("value", [8, -1])
def test_forward_at_names_the_first_code_out_of_range(value):
    o = torch.tensor([0, 7, 3], dtype=torch.int64)
    o[1] = value
    for call in (lambda: _model().forward_at(_scene(), GOOD, orient=o), lambda: _model().predict_at(_scene(), GOOD, orient=o),
                 lambda: _mim().forward_at(_scene(), GOOD, orient=o), lambda: _model().forward_at(_scene(), GOOD, orient=o.int())):
        with pytest.raises(ValueError, match=r"orient\[1\] = %d\b" % value):
            call()
    bad_row = GOOD.clone()
    bad_row[2, 1] = 9
    with pytest.raises(ValueError, match=r"row 2\b"):   # the origins' own check still speaks
        _model().forward_at(_scene(), bad_row, orient=CODES)


def test_orient_with_a_scene_gradient_is_refused():
    for kw in (dict(scene_grad=True), dict()):
        with pytest.raises(NotImplementedError, match="orient"):
            _model().forward_at(_scene().requires_grad_(True), GOOD, orient=CODES, **kw)
    with pytest.raises(NotImplementedError, match="orient"):
        _model().forward_at(_scene(), GOOD, scene_grad=True, orient=CODES)
    with pytest.raises(NotImplementedError, match="(?i)overlap"):   # without orient: the message it always had
        _model().forward_at(_scene().requires_grad_(True), GOOD)


def test_predict_at_refuses_tta_with_orient_and_unknown_tta():
    m = _model()
    with pytest.raises(ValueError, match="tta"):
        m.predict_at(_scene(), GOOD, orient=CODES, tta="d4")
    for bad in ("d8", "flip", True, 4):
        with pytest.raises(ValueError, match="tta"):
            m.predict_at(_scene(), GOOD, tta=bad)


def test_good_tables_reach_the_device_check():
    """in range, on a CPU scene: the existing 'no CPU fallback' error -- from every route, check=False included"""
    from maskedsst_amd._lib import MsstError
    m, mim = _model(), _mim()
    calls = [lambda: m.forward_at(_scene(), GOOD, orient=CODES), lambda: m.forward_at(_scene(), GOOD, check=False, orient=CODES.long()),
             lambda: m.predict_at(_scene(), GOOD, orient=CODES), lambda: m.predict_at(_scene(), GOOD, tta="d4"),
             lambda: mim.forward_at(_scene(), GOOD, orient=CODES), lambda: mim.forward_at(_scene(), GOOD, check=False, orient=CODES)]
    for call in calls:
        with pytest.raises((MsstError, RuntimeError), match="(?i)cuda|cpu|fallback|device"):
            call()


def test_the_engine_refuses_orient_outside_plain_listed_windows():
    from maskedsst_amd.engine import Windows, _TOK_FWD, _TOK_BWD, _TOK_INPUT_BWD, _tok_entry
    img, table = torch.zeros(2, 20, 16, 12), GOOD
    with pytest.raises(NotImplementedError, match="orient"):
        Windows("batch", torch.zeros(3, 20, 8, 8), orient=CODES)
    with pytest.raises(NotImplementedError, match="orient"):
        Windows("listed", img, table, csr=(None, None), orient=CODES)
    src, plain = Windows("listed", img, table, orient=CODES), Windows("listed", img, table)
    assert _tok_entry(_TOK_FWD, "tokenize", src, False, (0.1, 7)) == ("msst_tokenize_at_fwd_orient", (0.1, 7))
    assert _tok_entry(_TOK_FWD, "tokenize", src, True) == ("msst_tokenize_at_fwd_masked_orient", ())
    assert _tok_entry(_TOK_BWD, "tokenize_bwd", src, False)[0] == "msst_tokenize_at_bwd_orient"
    assert _tok_entry(_TOK_BWD, "tokenize_bwd", src, True)[0] == "msst_tokenize_at_bwd_masked_orient"
    assert _tok_entry(_TOK_FWD, "tokenize", plain, False)[0] == "msst_tokenize_at_fwd"   # without orient: the entry point it always was
    with pytest.raises(NotImplementedError):   # masked, listed and embedding dropout: still refused
        _tok_entry(_TOK_FWD, "tokenize", src, True, (0.1, 7))
    with pytest.raises(NotImplementedError, match="oriented"):
        _tok_entry(_TOK_INPUT_BWD, "tokenize_input_bwd", src, False)


# ------------------------------------------------------------------------------------------ the loader
@pytest.mark.parametrize("crop", ["batch", "sample"])
def test_resident_tile_loader_d4_keeps_the_origins_of_its_seed(crop):
    from maskedsst_amd.data import ResidentTileLoader
    kw = dict(image_size=8, tile_size=16, pool_tiles=5, steps=4, seed=11, device="cpu", crop=crop)
    plain = list(ResidentTileLoader(6, 20, **kw))
    aug = list(ResidentTileLoader(6, 20, augment="d4", **kw))
    again = list(ResidentTileLoader(6, 20, augment="d4", **kw))
    assert len(plain) == len(aug) == 4
    seen = []
    for p, a, b in zip(plain, aug, again):
        assert len(p) == 2 and len(a) == 3
        tiles, origins, orient = a
        assert torch.equal(tiles, p[0]) and torch.equal(origins, p[1])
        assert orient.dtype == torch.uint8 and orient.shape == (6,) and int(orient.max()) <= 7 and torch.equal(orient, b[2])
        seen += orient.tolist()
    assert len(set(seen)) > 3   # drawn, not constant
    with pytest.raises(ValueError, match="augment"):
        ResidentTileLoader(6, 20, augment="flip", **kw)


# ------------------------------------------------------------------------------------------ train_step_at
class _StubAt:
    """a model that only records what train_step_at hands it"""

    def __init__(self, nc, pixelwise, s):
        self.nc, self.pixelwise, self.s, self.seen = nc, pixelwise, s, None

    def forward_at(self, scene, origins, orient=None):
        self.seen = (scene, origins, orient)
        n = origins.shape[0]
        shape = (n, self.nc) if self.pixelwise else (n, self.nc, self.s, self.s)
        return torch.zeros(*shape, requires_grad=True) + torch.arange(self.nc, dtype=torch.float32).view(1, -1, *([1] * (len(shape) - 2)))

    def __call__(self, img):
        raise AssertionError("train_step_at must not call forward on a stacked copy")


class _StubOpt:
    def __init__(self):
        self.calls = []

    def zero_grad(self):
        self.calls.append("zero_grad")

    def step(self):
        self.calls.append("step")


@pytest.mark.parametrize("pixelwise,s", [(False, 8), (True, 7), (True, 8)])
@pytest.mark.parametrize("as_maps", [False, True])
def test_train_step_at_hands_orient_to_forward_at_and_to_the_labels(pixelwise, s, as_maps):
    from maskedsst_amd import random_orients, random_origins, window_labels
    from maskedsst_amd.config import Dotdict
    from maskedsst_amd.utils import train_step_at
    cfg = Dotdict(dict(image_size=8, patch_sub=8 - s, pixelwise=pixelwise, ignored_label=-1))
    g = torch.Generator().manual_seed(0)
    scene, label_map = torch.randn(2, 20, 21, 18, generator=g), torch.randint(-1, 6, (2, 21, 18), generator=g)
    origins = random_origins(2, 21, 18, s, 24, generator=g)
    orient = random_orients(24, generator=g)
    patches = torch.stack([_normative(label_map[b, y:y + s, x:x + s], o) for (b, y, x), o in zip(origins.tolist(), orient.tolist())])
    want = patches[:, s // 2, s // 2] if pixelwise else patches   # the labels of the ORIENTED windows (pixelwise: under their centre)
    labels = label_map if as_maps else (want if pixelwise else window_labels(label_map, origins, s, orient))
    seen = []

    def criterion(out, label):
        seen.append(label.clone())
        return torch.nn.functional.cross_entropy(out, label, ignore_index=-1)

    m, opt = _StubAt(6, pixelwise, s), _StubOpt()
    loss, acc, _ = train_step_at(scene, labels, origins, m, cfg, criterion, opt, orient=orient)
    assert m.seen[0] is scene and torch.equal(m.seen[1], origins) and m.seen[2] is orient
    assert len(seen) == 1 and seen[0].dtype == torch.int64 and torch.equal(seen[0], want)
    assert opt.calls == ["zero_grad", "step"] and bool(torch.isfinite(loss))
    if as_maps and not pixelwise:   # and without the keyword: the un-oriented labels, forward_at called as it always was
        train_step_at(scene, labels, origins, m, cfg, criterion, opt)
        assert m.seen[2] is None and torch.equal(seen[1], window_labels(label_map, origins, s))
        assert not torch.equal(seen[1], seen[0])


# ------------------------------------------------------------------------------------------ the scripts
@pytest.mark.parametrize("script,flags,needs", [("finetune.py", ["--augment", "d4"], "--train-at"), ("finetune.py", ["--val-tta"], "--val-at"),
                                                ("pretrain.py", ["--augment", "d4"], "--resident-tiles")])
def test_scripts_reject_the_flags_without_the_listed_windows_route(script, flags, needs):
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + flags, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode != 0 and needs in r.stderr and flags[0] in r.stderr, r.stderr[-400:]


# ------------------------------------------------------------------------------------------ the C ABI
def test_c_abi_declares_and_exports_the_orient_calls():
    from maskedsst_amd import _lib
    header = open(_lib.HEADER_PATH).read()
    lib = _lib.load()
    assert lib.msst_version() == _lib.header_version() == 109   # additive: the revision stays
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name, nargs in CALLS.items():
        m = re.search(r"^int %s\(([^;]*)\);" % name, header, re.M)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(getattr(lib, name).argtypes), name
        assert "const int32_t* origins, const uint8_t* orient" in m.group(1)
        assert name in _lib.declared_symbols() and re.search(r" T %s$" % name, out, re.M), name
        base = re.search(r"^int %s\(([^;]*)\);" % name.replace("_orient", ""), header, re.M)   # the namesake: one argument fewer, unchanged
        assert base and len(base.group(1).split(",")) == nargs - 1


_SHAPE = dict(Bs=2, Hs=16, Ws=16, window=8, nwin=8, S=2, P=10, split=0)


def _fwd(lib, ptr=4096, origins=4096, orient=4096, **k):
    a = {**_SHAPE, **k}
    return lib.msst_tokenize_at_fwd_orient(ptr, origins, orient, *([ptr] * 8), a["split"], ptr, a["Bs"], a["Hs"], a["Ws"], a["window"], a["nwin"],
                                           a["S"], a["P"], 0.1, 7, None)


def _bwd(lib, ptr=4096, origins=4096, orient=4096, nchunk=2, **k):
    a = {**_SHAPE, **k}
    return lib.msst_tokenize_at_bwd_orient(ptr, origins, orient, *([ptr] * 8), nchunk, *([ptr] * 8), a["split"], a["Bs"], a["Hs"], a["Ws"],
                                           a["window"], a["nwin"], a["S"], a["P"], 0.1, 7, None)


def _fwd_masked(lib, ptr=4096, origins=4096, orient=4096, **k):
    a = {**_SHAPE, **k}
    return lib.msst_tokenize_at_fwd_masked_orient(ptr, origins, orient, *([ptr] * 8), a["split"], ptr, ptr, ptr, a["Bs"], a["Hs"], a["Ws"],
                                                  a["window"], a["nwin"], a["S"], a["P"], None)


def _bwd_masked(lib, ptr=4096, origins=4096, orient=4096, nchunk=2, **k):
    a = {**_SHAPE, **k}
    return lib.msst_tokenize_at_bwd_masked_orient(ptr, origins, orient, *([ptr] * 9), nchunk, *([ptr] * 8), a["split"], ptr, a["Bs"], a["Hs"],
                                                  a["Ws"], a["window"], a["nwin"], a["S"], a["P"], None)


def _head(lib, ptr=4096, origins=4096, orient=4096, K=89, **k):
    a = {**_SHAPE, **k}
    return lib.msst_head_at_fwd_orient(ptr, ptr, origins, orient, ptr, ptr, ptr, 1, ptr, ptr, ptr, ptr, a["Bs"], a["Hs"], a["Ws"], a["window"],
                                       a["nwin"], a["S"], a["P"], K, None)


def test_the_orient_calls_refuse_bad_arguments_before_launch():
    """fake, never dereferenced pointers (or none) and no device: no call can have reached a launch"""
    from maskedsst_amd import _lib
    lib = _lib.load()
    for call in (_fwd, _bwd, _fwd_masked, _bwd_masked, _head):
        assert call(lib, orient=None) == BADARG, call.__name__                       # a null orientation table
        assert call(lib, nwin=-1) == BADARG, call.__name__
        assert call(lib, window=9, Hs=32, Ws=32) == UNSUPPORTED, call.__name__      # window * window > 64
        for bad in (dict(P=17), dict(window=8, Hs=7), dict(window=8, Ws=7)):
            assert call(lib, **bad) == UNSUPPORTED, (call.__name__, bad)
        for bad in (dict(Bs=0), dict(Hs=0), dict(Ws=0), dict(window=0), dict(S=0), dict(P=0)):
            assert call(lib, **bad) == BADARG, (call.__name__, bad)
        assert call(lib, ptr=None) == BADARG and call(lib, origins=None) == BADARG   # null buffers, null table
        assert b"_orient" in lib.msst_last_error()
    for call in (_fwd, _bwd, _fwd_masked, _bwd_masked):
        assert call(lib, split=96) == BADARG and call(lib, split=-1) == BADARG
    for call in (_bwd, _bwd_masked):
        assert call(lib, nwin=0) == BADARG and call(lib, nchunk=0) == BADARG
    assert _head(lib, nwin=0) == BADARG and _head(lib, K=0) == BADARG and _head(lib, K=129) == BADARG
    assert _head(lib, nwin=65536) == UNSUPPORTED and _fwd(lib, window=7, nwin=65536) == UNSUPPORTED   # one grid row per window
    assert _fwd(lib, nwin=0) == 0 and _fwd_masked(lib, nwin=0) == 0   # an empty forward call enqueues nothing
