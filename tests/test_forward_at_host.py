"""Windows at listed scene positions, host side (no GPU needed): the origin helpers of maskedsst_amd.scene against brute-force loops that
restate the reference's Houston2018Dataset (src/data_houston2018.py:248-255, :303-317, :319-329), the C ABI of msst_tokenize_at_fwd /
msst_tokenize_at_bwd and their argument checks (they run before any HIP call, so fake buffers and no device are enough to see them),
``forward_at``'s refusals on CPU tensors, and ``train_step_at`` on a stub model."""
import re
import subprocess

import pytest
import torch

BADARG, UNSUPPORTED = -3, -2   # include/msst.h: MSST_ERR_BADARG, MSST_ERR_UNSUPPORTED
CALLS = {"msst_tokenize_at_fwd": 22, "msst_tokenize_at_bwd": 30}   # declared argument counts


def _label_maps(Bs, Hs, Ws, window, seed):
    """sparse label maps with labelled pixels on the border, exactly window // 2 away from it on each side, and one step inside that"""
    g = torch.Generator().manual_seed(seed)
    lab = torch.where(torch.rand(Bs, Hs, Ws, generator=g) < 0.15, torch.randint(0, 6, (Bs, Hs, Ws), generator=g), torch.tensor(-1))
    h = window // 2
    for b in range(Bs):
        for y, x in ((0, 0), (Hs - 1, Ws - 1), (0, Ws // 2), (Hs // 2, 0),                       # on the border: no window fits
                     (h, h), (Hs - 1 - h, Ws - 1 - h), (h, Ws - 1 - h), (Hs - 1 - h, h),         # the outermost centres that fit
                     (h - 1, h), (h, h - 1), (Hs - h, h), (h, Ws - h)):                           # one pixel too far out
            lab[b, y, x] = (y + x + b) % 6
    return lab


def _centre_brute(labels, window, ignore_index=-1):
    """data_houston2018.py:248-255 (labeled_idx) and :303-317 (the slice), scene by scene"""
    rows, labs = [], []
    h = window // 2
    add = 0 if window % 2 == 0 else 1
    for b in range(labels.shape[0]):
        lab = labels[b]
        for y in range(lab.shape[0]):
            for x in range(lab.shape[1]):
                if lab[y, x] == ignore_index:
                    continue
                if not (y >= h and y + h < lab.shape[0] and x >= h and x + h < lab.shape[1]):
                    continue
                ys, xs = slice(y - h, y + h + add), slice(x - h, x + h + add)
                assert ys.stop - ys.start == window and ys.stop <= lab.shape[0] and xs.stop <= lab.shape[1]
                assert y - ys.start == h and x - xs.start == h   # the centre sits at index window // 2 of the slice
                rows.append((b, ys.start, xs.start))
                labs.append(int(lab[y, x]))
    return rows, labs


@pytest.mark.parametrize("window", [8, 7])
@pytest.mark.parametrize("Bs,Hs,Ws", [(1, 19, 23), (2, 17, 12)])
def test_centre_origins_restates_the_reference_loop(window, Bs, Hs, Ws):
    from maskedsst_amd import centre_origins
    labels = _label_maps(Bs, Hs, Ws, window, 3)
    origins, centre = centre_origins(labels, window)
    rows, labs = _centre_brute(labels, window)
    assert origins.dtype == torch.int32 and centre.dtype == torch.int64 and origins.shape == (len(rows), 3) and len(rows) > 8
    assert origins.tolist() == [list(r) for r in rows] and centre.tolist() == labs   # nonzero()'s order: scene, row, column
    h = window // 2
    assert origins[:, 1].min() == 0 and origins[:, 1].max() == Hs - 1 - 2 * h   # the outermost centres are in, and nothing beyond
    assert origins[:, 2].min() == 0 and origins[:, 2].max() == Ws - 1 - 2 * h
    assert int(origins[:, 1].max()) + window <= Hs and int(origins[:, 2].max()) + window <= Ws
    # another ignore_index
    o2, c2 = centre_origins(torch.where(labels == -1, torch.tensor(255), labels), window, ignore_index=255)
    assert torch.equal(o2, origins) and torch.equal(c2, centre)


def test_centre_origins_of_an_all_ignored_map_is_empty():
    from maskedsst_amd import centre_origins, window_labels
    labels = torch.full((2, 9, 11), -1)
    origins, centre = centre_origins(labels, 7)
    assert origins.shape == (0, 3) and origins.dtype == torch.int32 and centre.shape == (0,) and centre.dtype == torch.int64
    assert window_labels(labels, origins, 7).shape == (0, 7, 7)
    with pytest.raises(ValueError):
        centre_origins(labels[0], 7)


@pytest.mark.parametrize("window", [8, 7])
def test_window_labels_is_the_reference_slice(window):
    from maskedsst_amd import centre_origins, window_labels
    labels = _label_maps(2, 17, 21, window, 5)
    origins, centre = centre_origins(labels, window)
    origins = torch.cat([origins.flip(0), torch.tensor([[1, 17 - window, 21 - window], [0, 0, 0]], dtype=torch.int32)])
    got = window_labels(labels, origins, window)
    assert got.shape == (origins.shape[0], window, window) and got.dtype == torch.int64
    for i, (b, y, x) in enumerate(origins.tolist()):
        assert torch.equal(got[i], labels[b, y:y + window, x:x + window]), i   # :324
    assert torch.equal(got[:centre.numel(), window // 2, window // 2], centre.flip(0))


@pytest.mark.parametrize("window", [8, 7])
def test_random_origins_range_reproducibility_and_redraw(window):
    from maskedsst_amd import random_origins, window_labels
    Bs, Hs, Ws, n = 2, 20, 13, 400
    a = random_origins(Bs, Hs, Ws, window, n, generator=torch.Generator().manual_seed(9))
    b = random_origins(Bs, Hs, Ws, window, n, generator=torch.Generator().manual_seed(9))
    c = random_origins(Bs, Hs, Ws, window, n, generator=torch.Generator().manual_seed(10))
    assert a.shape == (n, 3) and a.dtype == torch.int32 and torch.equal(a, b) and not torch.equal(a, c)
    for col, hi in enumerate((Bs - 1, Hs - window, Ws - window)):
        assert int(a[:, col].min()) == 0 and int(a[:, col].max()) == hi, (col, hi)   # the closed range, both ends reached in 400 draws
    assert random_origins(Bs, Hs, Ws, window, 0).shape == (0, 3)
    # drop_unlabeled (:326-327): one labelled pixel in scene 1 -- every window must hold it; brute force over the returned rows
    labels = torch.full((Bs, Hs, Ws), -1)
    labels[1, 11, 6] = 3
    d = random_origins(Bs, Hs, Ws, window, 50, generator=torch.Generator().manual_seed(9), labels=labels)
    e = random_origins(Bs, Hs, Ws, window, 50, generator=torch.Generator().manual_seed(9), labels=labels)
    assert d.shape == (50, 3) and torch.equal(d, e)
    for s, y, x in d.tolist():
        assert s == 1 and 0 <= y <= Hs - window and 0 <= x <= Ws - window
        assert bool((labels[s, y:y + window, x:x + window] != -1).any())
    assert len({tuple(r) for r in d.tolist()}) > 1   # redrawn, not one window repeated
    assert bool((window_labels(labels, d, window) == 3).flatten(1).any(1).all())
    with pytest.raises(ValueError):
        random_origins(Bs, Hs, Ws, window, 5, labels=torch.full((Bs, Hs, Ws), -1))   # nothing labelled: the redraw would not end
    with pytest.raises(ValueError):
        random_origins(Bs, 6, Ws, window, 5)   # no window fits


def test_c_abi_declares_and_exports_the_listed_origin_calls():
    from maskedsst_amd import _lib
    header = open(_lib.HEADER_PATH).read()
    lib = _lib.load()
    assert lib.msst_version() == _lib.header_version() == 109   # additive: the revision stays
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name, nargs in CALLS.items():
        m = re.search(r"^int %s\(([^;]*)\);" % name, header, re.M)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(getattr(lib, name).argtypes), name
        assert "const int32_t* origins" in m.group(1)
        assert name in _lib.declared_symbols() and re.search(r" T %s$" % name, out, re.M), name


def _fwd(lib, ptr=4096, origins=4096, **k):
    a = {**dict(Bs=2, Hs=16, Ws=16, window=8, nwin=8, S=2, P=10, split=0), **k}
    return lib.msst_tokenize_at_fwd(ptr, origins, *([ptr] * 8), a["split"], ptr, a["Bs"], a["Hs"], a["Ws"], a["window"], a["nwin"], a["S"],
                                    a["P"], 0.1, 7, None)


def _bwd(lib, ptr=4096, origins=4096, nchunk=2, **k):
    a = {**dict(Bs=2, Hs=16, Ws=16, window=8, nwin=8, S=2, P=10, split=0), **k}
    return lib.msst_tokenize_at_bwd(ptr, origins, *([ptr] * 8), nchunk, *([ptr] * 8), a["split"], a["Bs"], a["Hs"], a["Ws"], a["window"],
                                    a["nwin"], a["S"], a["P"], 0.1, 7, None)


def test_listed_origin_calls_refuse_bad_arguments_before_launch():
    """fake, never dereferenced pointers (or none) and no device: no call can have reached a launch"""
    from maskedsst_amd import _lib
    lib = _lib.load()
    for call in (_fwd, _bwd):
        for bad in (dict(window=9, Hs=32, Ws=32), dict(P=17), dict(window=8, Hs=7), dict(window=8, Ws=7)):
            assert call(lib, **bad) == UNSUPPORTED, (call.__name__, bad)
        for bad in (dict(Bs=0), dict(Hs=0), dict(Ws=0), dict(window=0), dict(S=0), dict(P=0), dict(nwin=-1), dict(split=96), dict(split=-1)):
            assert call(lib, **bad) == BADARG, (call.__name__, bad)
        assert call(lib, ptr=None) == BADARG and call(lib, origins=None) == BADARG   # null buffers, null table
        assert b"msst_tokenize_at" in lib.msst_last_error()
    assert _bwd(lib, nwin=0) == BADARG and _bwd(lib, nchunk=0) == BADARG
    assert _fwd(lib, window=7, nwin=65536) == UNSUPPORTED   # the generic kernels: one grid row per window
    assert _fwd(lib, nwin=0) == 0   # an empty forward call enqueues nothing


def _model(**kw):
    from maskedsst_amd import ViTSpatialSpectral
    return ViTSpatialSpectral(
        **{**dict(image_size=8, spatial_patch_size=1, spectral_patch_size=10, num_classes=4, dim=96, depth=1, heads=2, mlp_dim=64, dropout=0.0,
                  emb_dropout=0.0, channels=20, spectral_pos_embed=False, spectral_pos=torch.arange(2), blockwise_patch_embed=True), **kw})


GOOD = torch.tensor([[0, 0, 0], [1, 8, 4], [1, 3, 2]], dtype=torch.int32)   # scenes [2, 20, 16, 12]: y0 <= 8, x0 <= 4


def _scene():
    return torch.zeros(2, 20, 16, 12)


@pytest.mark.parametrize("shape", [(20, 16, 16), (1, 20, 16, 16, 1), (1, 30, 16, 16), (1, 20, 7, 16), (1, 20, 16, 7)])
def test_forward_at_refuses_bad_scenes(shape):
    o = torch.zeros(1, 3, dtype=torch.int32)
    with pytest.raises(ValueError):
        _model().forward_at(torch.zeros(*shape), o)
    with pytest.raises(ValueError):
        _model().predict_at(torch.zeros(*shape), o)


def test_forward_at_refuses_bad_tables():
    m = _model()
    for bad in (torch.zeros(3, 2, dtype=torch.int32), torch.zeros(3, dtype=torch.int32), torch.zeros(1, 3, 3, dtype=torch.int64),
                GOOD.float(), GOOD.double(), GOOD.tolist()):
        with pytest.raises(ValueError, match="origins"):
            m.forward_at(_scene(), bad)
        with pytest.raises(ValueError, match="origins"):
            m.forward_at(_scene(), bad, check=False)   # shape and dtype are checked without reading the table


@pytest.mark.parametrize("col,value", [(0, 2), (0, -1), (1, 9), (1, -1), (2, 5), (2, -1)])
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_forward_at_names_the_first_row_out_of_range(col, value, dtype):
    o = torch.cat([GOOD, GOOD, GOOD]).to(dtype)
    o[4, col] = value
    o[7, col] = value   # a later bad row: the first one is named
    with pytest.raises(ValueError, match=r"row 4\b"):
        _model().forward_at(_scene(), o)
    with pytest.raises(ValueError, match=r"row 4\b"):
        _model().predict_at(_scene(), o)


def test_forward_at_good_table_and_check_false_reach_the_device_check():
    """a table in range passes the checks and meets the CPU refusal; check=False does not read the table: a bad row gets as far"""
    from maskedsst_amd._lib import MsstError
    m = _model()
    bad = GOOD.clone()
    bad[1, 1] = 99
    for o, check in ((GOOD, True), (GOOD.long(), True), (bad, False)):
        with pytest.raises((MsstError, RuntimeError), match="(?i)cuda|cpu|fallback|device"):
            m.forward_at(_scene(), o, check=check)

    class Unreadable(torch.Tensor):
        """an origins table whose values cannot be looked at"""
        @classmethod
        def __torch_function__(cls, func, types, args=(), kwargs=None):
            name = getattr(func, "__name__", "")
            if name not in ("__get__", "dim"):   # shape, dtype and rank are all that check=False may ask for
                raise AssertionError("check=False read the table: " + name)
            return super().__torch_function__(func, types, args, kwargs or {})

    u = bad.as_subclass(Unreadable)
    with pytest.raises(AssertionError, match="read the table"):
        m.forward_at(_scene(), u)
    with pytest.raises((MsstError, RuntimeError), match="(?i)cuda|cpu|fallback|device"):
        m.forward_at(_scene(), u, check=False)


def test_forward_at_refuses_a_scene_that_wants_a_gradient():
    with pytest.raises(NotImplementedError, match="(?i)overlap"):
        _model().forward_at(_scene().requires_grad_(True), GOOD)


class _StubAt:
    """a model that only records what train_step_at hands it"""

    def __init__(self, nc, pixelwise, s):
        self.nc, self.pixelwise, self.s, self.seen = nc, pixelwise, s, None

    def forward_at(self, scene, origins):
        self.seen = (scene, origins)
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


@pytest.mark.parametrize("pixelwise", [False, True])
@pytest.mark.parametrize("as_maps", [False, True])
def test_train_step_at_feeds_the_labels_of_the_listed_windows(pixelwise, as_maps):
    from maskedsst_amd import centre_origins, window_labels
    from maskedsst_amd.config import Dotdict
    from maskedsst_amd.utils import train_step_at
    s = 7 if pixelwise else 8
    cfg = Dotdict(dict(image_size=8, patch_sub=1 if pixelwise else 0, pixelwise=pixelwise, ignored_label=-1))
    torch.manual_seed(0)
    scene, label_map = torch.randn(2, 20, 21, 18), _label_maps(2, 21, 18, s, 1)
    origins, centre = centre_origins(label_map, s)
    pick = torch.randperm(origins.shape[0])[:24]
    origins, centre = origins[pick], centre[pick]
    want = centre if pixelwise else torch.stack([label_map[b, y:y + s, x:x + s] for b, y, x in origins.tolist()])
    labels = label_map if as_maps else (centre if pixelwise else window_labels(label_map, origins, s))
    seen = []

    def criterion(out, label):
        seen.append(label.clone())
        return torch.nn.functional.cross_entropy(out, label, ignore_index=-1)

    m, opt = _StubAt(6, pixelwise, s), _StubOpt()
    state = torch.get_rng_state()
    loss, acc, _ = train_step_at(scene, labels, origins, m, cfg, criterion, opt)
    assert torch.equal(torch.get_rng_state(), state)   # nothing drawn: no crop
    assert m.seen[0] is scene and torch.equal(m.seen[1], origins)   # the scene as it is, not a copy of its windows
    assert len(seen) == 1 and seen[0].dtype == torch.int64 and torch.equal(seen[0], want)
    assert opt.calls == ["zero_grad", "step"] and bool(torch.isfinite(loss)) and 0.0 <= float(acc) <= 1.0
    with pytest.raises(ValueError):
        train_step_at(scene, want[:-1], origins, m, cfg, criterion, opt)
