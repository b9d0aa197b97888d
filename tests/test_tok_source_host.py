"""Host: the tokenizer's window source (``engine.Windows``) from the Engine methods down to the C calls.  An Engine whose ``lib`` is a
recording stand-in is driven on CPU tensors (as tests/test_dp_gloo.py does); every cell of the (method, source, mask) table must reach
its entry point with the integer arguments written out below by hand -- shapes, window grid, nchunk, pos_split, dropout seed -- and
with the source's own pointers in front."""
import ctypes

import pytest
import torch

import maskedsst_amd.engine as engine_mod
from maskedsst_amd import SimMIMSpatialSpectral, ViTSpatialSpectral
from maskedsst_amd.engine import Windows

T, K = 128, 5            # tokens of a window (S N), masked tokens in the head call
DROP = (0.25, 77)        # embedding dropout (p, seed): both must reach the call


class RecordingLib:
    """every msst_* entry point: records (name, arguments), reports success"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("msst_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


def _engine(monkeypatch, image_size=8, simmim=True, spectral_pos_embed=False):
    torch.manual_seed(3)
    enc = ViTSpatialSpectral(image_size=image_size, spatial_patch_size=1, spectral_patch_size=10, num_classes=4, dim=96, depth=1, heads=2,
                             mlp_dim=64, channels=20, spectral_pos_embed=spectral_pos_embed, spectral_pos=torch.arange(2), precision="fp32")
    model = SimMIMSpatialSpectral(encoder=enc, masking_ratio=0.7, mask_patch_size=4, tube_masking=True,
                                  to_pixels_per_spectral_block=True) if simmim else enc
    eng = model.engine()
    monkeypatch.setattr(engine_mod, "_stream", lambda: ctypes.c_void_p(0))
    eng._require_cuda = lambda t: None   # CPU tensors stand in for device memory in this test only
    eng.lib = RecordingLib()
    return eng


def _sources(s=8):
    """the three sources of the issue: 3 windows each way but the tiles' 2 x 2 x 2 = 8 (19 = 2 s + 3 rows, 17 = 2 s + 1 columns: dropped)"""
    g = torch.Generator().manual_seed(1)
    origins = torch.tensor([[0, 0, 0], [1, 8, 4], [0, 3, 1]], dtype=torch.int32)
    return {"batch": Windows("batch", torch.randn(3, 20, s, s, generator=g)),
            "tiles": Windows("tiles", torch.randn(2, 20, 19, 17, generator=g), s=s),
            "listed": Windows("listed", torch.randn(2, 20, 16, 12, generator=g), origins)}


def _ints(args):
    return [a for a in args if type(a) is int]


def _floats(args):
    return [a for a in args if type(a) is float]


def _lead(src):
    return [src.img.data_ptr()] + ([src.origins.data_ptr()] if src.kind == "listed" else [])


def _one_call(eng):
    (name, args), = eng.lib.calls
    eng.lib.calls.clear()
    return name, args


# the shape integers of each source as its entry points take them: B S N P / Bs Hs Ws window stride win0 nwin S P / Bs Hs Ws window nwin S P
SHAPE = {"batch": [3, 2, 64, 10], "tiles": [2, 19, 17, 8, 8, 0, 8, 2, 10], "listed": [2, 16, 12, 8, 3, 2, 10]}
N_WIN = {"batch": 3, "tiles": 8, "listed": 3}

FWD = [("batch", False, "msst_tokenize_fwd"), ("batch", True, "msst_tokenize_fwd"), ("tiles", False, "msst_tokenize_scene_fwd_train"),
       ("listed", False, "msst_tokenize_at_fwd"), ("listed", True, "msst_tokenize_at_fwd_masked")]
BWD = [("batch", False, "msst_tokenize_bwd"), ("batch", True, "msst_tokenize_bwd"), ("tiles", False, "msst_tokenize_scene_bwd"),
       ("listed", False, "msst_tokenize_at_bwd"), ("listed", True, "msst_tokenize_at_bwd_masked")]
INPUT_BWD = [("batch", False, "msst_tokenize_bwd_input"), ("batch", True, "msst_tokenize_bwd_input"),
             ("tiles", False, "msst_tokenize_scene_bwd_input"), ("listed", False, "msst_tokenize_at_bwd_input")]


def _drop(kind, masked):
    """the masked listed entry points take no dropout arguments; a mask and dropout together have no listed entry point at all"""
    return (0.0, 0) if (kind == "listed" and masked) else DROP


def _drop_ints(kind, masked):
    return [] if (kind == "listed" and masked) else [77]


@pytest.mark.parametrize("kind,masked,entry", FWD)
def test_tokenize_reaches_its_entry_point(monkeypatch, kind, masked, entry):
    eng = _engine(monkeypatch)
    src = _sources()[kind]
    n = N_WIN[kind]
    mask = torch.zeros(n, T, dtype=torch.uint8) if masked else None
    out = eng.tokenize(src, mask, emb_drop=_drop(kind, masked))
    name, args = _one_call(eng)
    assert name == entry and tuple(out.shape) == (n, T, 96)
    assert _ints(args) == [0] + SHAPE[kind] + _drop_ints(kind, masked)            # pos_split, the shape, the seed
    assert _floats(args) == ([] if (kind == "listed" and masked) else [0.25])
    ptrs = [a.value or 0 for a in args if isinstance(a, ctypes.c_void_p)]
    assert ptrs[:len(_lead(src))] == _lead(src)
    assert out.data_ptr() in ptrs
    if masked:
        assert mask.data_ptr() in ptrs and eng.fp.ptr("mask_token") in ptrs
    elif kind == "batch":                                                         # nothing masked: the zero mask
        assert eng._zero_mask_for(n * T, "cpu").data_ptr() in ptrs
    if kind == "batch":                                                           # a bare tensor means a batch: the same call
        eng.tokenize(src.img, mask, emb_drop=DROP)
        assert [type(a) for a in _one_call(eng)[1]] == [type(a) for a in args]


def test_tokenize_without_positions_passes_the_zero_table(monkeypatch):
    eng = _engine(monkeypatch, spectral_pos_embed=True)
    src = _sources()["batch"]
    eng.tokenize(src)
    split = eng.enc.pos_embed.shape[-1]
    assert split > 0 and _ints(_one_call(eng)[1]) == [split] + SHAPE["batch"] + [0]
    eng.tokenize(src, with_pos=False)
    _, args = _one_call(eng)
    assert _ints(args) == [0] + SHAPE["batch"] + [0]
    assert args[7].value == eng._zero_pos.data_ptr() and not args[8].value


@pytest.mark.parametrize("kind,masked,entry", BWD)
def test_tokenize_bwd_reaches_its_entry_point(monkeypatch, kind, masked, entry):
    eng = _engine(monkeypatch)
    src = _sources()[kind]
    n = N_WIN[kind]
    fired = []
    eng.bucket_hook = lambda name, start, end: fired.append(name)
    mask = torch.zeros(n, T, dtype=torch.uint8) if masked else None
    dx0 = torch.zeros(n, T, 96)
    eng.ensure()
    eng.tokenize_bwd(src, mask, dx0, emb_drop=_drop(kind, masked))
    name, args = _one_call(eng)
    assert name == entry
    assert _ints(args) == [n, 0] + SHAPE[kind] + _drop_ints(kind, masked)         # nchunk = min(windows, 64), pos_split, the shape, the seed
    ptrs = [a.value or 0 for a in args if isinstance(a, ctypes.c_void_p)]
    assert ptrs[:len(_lead(src))] == _lead(src) and dx0.data_ptr() in ptrs
    assert (eng.fp.ptr("mask_token", eng.fp.grad) in ptrs) == (kind == "batch" or masked)
    if masked:
        assert mask.data_ptr() in ptrs
    elif kind == "batch":
        assert eng._zero_mask_for(n * T, "cpu").data_ptr() in ptrs
    assert "tokenizer" in fired


@pytest.mark.parametrize("kind,masked,entry", INPUT_BWD)
def test_tokenize_input_bwd_reaches_its_entry_point(monkeypatch, kind, masked, entry):
    eng = _engine(monkeypatch)
    src = _sources()[kind]
    n = N_WIN[kind]
    if kind == "listed":
        from maskedsst_amd.scene import origins_csr
        src = Windows("listed", src.img, src.origins, origins_csr(src.origins, 2, 16, 12))
    mask = torch.zeros(n, T, dtype=torch.uint8) if masked else None
    dx0 = torch.zeros(n, T, 96)
    eng.ensure()
    dimg = eng.tokenize_input_bwd(src, mask, dx0, emb_drop=DROP)
    assert tuple(dimg.shape) == tuple(src.img.shape)
    calls = list(eng.lib.calls)
    assert calls[0][0] == entry and _ints(calls[0][1]) == SHAPE[kind] + [77]
    ptrs = [a.value or 0 for a in calls[0][1] if isinstance(a, ctypes.c_void_p)]
    assert ptrs[:len(_lead(src))] == _lead(src) and dx0.data_ptr() in ptrs
    if kind != "listed":
        assert len(calls) == 1 and dimg.data_ptr() in ptrs
        return
    (name, args), = calls[1:]                                                     # the per-window gradients, then the fold into the scenes
    assert name == "msst_scene_fold_at" and _ints(args) == [2, 20, 16, 12, 8, 3, 10, 0]   # Bs C Hs Ws window nwin P accumulate
    assert args[3].value == dimg.data_ptr() and args[0].value in ptrs


def test_listed_input_bwd_folds_into_a_sink_and_refuses_without_the_index(monkeypatch):
    from maskedsst_amd.scene import origins_csr
    eng = _engine(monkeypatch)
    base = _sources()["listed"]
    dx0 = torch.zeros(3, T, 96)
    eng.ensure()
    with pytest.raises(NotImplementedError, match="scene_grad=True"):
        eng.tokenize_input_bwd(base, None, dx0)
    assert not eng.lib.calls
    sink = engine_mod.SceneGradSink(torch.zeros(2, 20, 16, 12))
    src = Windows("listed", base.img, base.origins, origins_csr(base.origins, 2, 16, 12), sink)
    for accumulate in (0, 1):                                                     # the first fold writes the map whole, the later ones add
        assert eng.tokenize_input_bwd(src, None, dx0) is sink.out
        fold = eng.lib.calls[-1][1]
        assert eng.lib.calls[-1][0] == "msst_scene_fold_at" and _ints(fold)[-1] == accumulate and fold[3].value == sink.out.data_ptr()


@pytest.mark.parametrize("kind,entry,ints", [("batch", "msst_head_fwd", [1, 3, 2, 64, 10, K]),
                                             ("listed", "msst_head_at_fwd", [1, 2, 16, 12, 8, 3, 2, 10, K])])
def test_head_fwd_reads_its_targets_from_the_source(monkeypatch, kind, entry, ints):
    eng = _engine(monkeypatch)
    src = _sources()[kind]
    eng.ensure()
    eng.head_fwd(torch.zeros(3, T, 96), src, torch.zeros(3, K, dtype=torch.int32))
    name, args = _one_call(eng)
    assert name == entry and _ints(args) == ints                                  # per_block, the shape, K
    assert [a.value for a in args[1:1 + len(_lead(src))]] == _lead(src)
    with pytest.raises(NotImplementedError, match="tiles"):
        eng.head_fwd(torch.zeros(8, T, 96), _sources()["tiles"], torch.zeros(8, K, dtype=torch.int32))


def _listed6(s):
    g = torch.Generator().manual_seed(2)
    origins = torch.tensor([[0, 0, 0], [1, 2, 3], [0, 1, 1], [1, 0, 0], [0, 4, 2], [1, 3, 3]], dtype=torch.int32)
    return Windows("listed", torch.randn(2, 20, 16, 12, generator=g), origins)


def test_generic_tokenizer_launches_in_chunks_and_refuses_dropout_then(monkeypatch):
    eng = _engine(monkeypatch, image_size=7, simmim=False)        # 7 x 7 windows: the generic kernels, one grid row per window
    monkeypatch.setattr(eng, "TILE_WINDOWS_PER_LAUNCH", 4)
    tiles = _sources(7)["tiles"]                                  # 19 // 7 = 2, 17 // 7 = 2: 8 windows again
    assert (tiles.grid, tiles.n) == ((2, 2), 8)
    out = eng.tokenize(tiles)
    calls = list(eng.lib.calls)
    eng.lib.calls.clear()
    assert [c[0] for c in calls] == ["msst_tokenize_scene_fwd_train"] * 2
    assert [_ints(c[1]) for c in calls] == [[0, 2, 19, 17, 7, 7, win0, 4, 2, 10, 0] for win0 in (0, 4)]
    assert [c[1][10].value for c in calls] == [out.data_ptr(), out[4:].data_ptr()]
    listed = _listed6(7)
    out = eng.tokenize(listed)
    calls = list(eng.lib.calls)
    eng.lib.calls.clear()
    assert [c[0] for c in calls] == ["msst_tokenize_at_fwd"] * 2
    assert [_ints(c[1]) for c in calls] == [[0, 2, 16, 12, 7, nwin, 2, 10, 0] for nwin in (4, 2)]
    assert [c[1][1].value for c in calls] == [listed.origins.data_ptr(), listed.origins[4:].data_ptr()]
    assert [c[1][11].value for c in calls] == [out.data_ptr(), out[4:].data_ptr()]
    for src in (tiles, listed):
        with pytest.raises(NotImplementedError, match="embedding dropout over"):
            eng.tokenize(src, emb_drop=DROP)
    assert not eng.lib.calls


def test_mfma_tokenizer_takes_any_number_of_windows_in_one_launch(monkeypatch):
    eng = _engine(monkeypatch, simmim=False)                      # 8 x 8 windows of 10-band patches
    monkeypatch.setattr(eng, "TILE_WINDOWS_PER_LAUNCH", 4)
    eng.tokenize(_sources()["tiles"], emb_drop=DROP)
    assert _ints(_one_call(eng)[1]) == [0] + SHAPE["tiles"] + [77]
    eng.tokenize(_listed6(8), emb_drop=DROP)
    assert _ints(_one_call(eng)[1]) == [0, 2, 16, 12, 8, 6, 2, 10, 77]


def test_combinations_without_an_entry_point_are_refused(monkeypatch):
    eng = _engine(monkeypatch)
    src = _sources()
    eng.ensure()
    dx8, dx3 = torch.zeros(8, T, 96), torch.zeros(3, T, 96)
    m8, m3 = torch.zeros(8, T, dtype=torch.uint8), torch.zeros(3, T, dtype=torch.uint8)
    refused = [lambda: eng.tokenize(src["tiles"], m8),                                      # tiles with a token mask
               lambda: eng.tokenize_bwd(src["tiles"], m8, dx8),
               lambda: eng.tokenize_input_bwd(src["tiles"], m8, dx8),
               lambda: eng.tokenize(src["listed"], m3, emb_drop=DROP),                       # a mask with embedding dropout on listed windows
               lambda: eng.tokenize_bwd(src["listed"], m3, dx3, emb_drop=DROP),
               lambda: eng.tokenize_input_bwd(src["listed"], m3, dx3),
               lambda: eng.tokenize_input_bwd(src["tiles"], None, dx8, dtarget=torch.zeros(8, 20, 64)),   # dtarget on anything but a batch
               lambda: eng.tokenize_input_bwd(src["listed"], None, dx3, dtarget=torch.zeros(3, 20, 64))]
    for call in refused:
        with pytest.raises(NotImplementedError, match="no entry point"):
            call()
    assert not eng.lib.calls


def test_classify_at_refuses_a_source_without_rows(monkeypatch):
    eng = _engine(monkeypatch, simmim=False)
    base = _sources()["listed"]
    with pytest.raises(ValueError, match="origins lists no window"):
        eng.classify_at(Windows("listed", base.img, base.origins[:0]))
    assert not eng.lib.calls


def test_the_old_spellings_are_gone():
    for name in ("_SimMIMLossAtFn", "ListedWindows", "_window_kw"):
        assert not hasattr(engine_mod, name), name
    for name in ("tokenize_windows", "_tokenize_at", "tokenize_at_masked", "tokenize_at_masked_bwd", "tokenize_windows_bwd",
                 "tokenize_windows_input_bwd", "simmim_loss_at", "tile_grid"):
        assert not hasattr(engine_mod.Engine, name), name
