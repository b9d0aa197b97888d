"""SimMIM pre-training on windows read from resident tiles, host side (no GPU needed): ``ResidentTileLoader`` against
``SyntheticCubeLoader`` at the same seed, the C ABI of msst_tokenize_at_fwd_masked / msst_tokenize_at_bwd_masked / msst_head_at_fwd and
their argument checks (they run before any HIP call, so fake buffers and no device are enough to see them), and the refusals of
``SimMIMSpatialSpectral.forward_at`` / ``forward_windows`` on CPU tensors."""
import re
import subprocess

import numpy as np
import pytest
import torch

BADARG, UNSUPPORTED = -3, -2   # include/msst.h: MSST_ERR_BADARG, MSST_ERR_UNSUPPORTED
CALLS = {"msst_tokenize_at_fwd_masked": 22, "msst_tokenize_at_bwd_masked": 30, "msst_head_at_fwd": 20}   # declared argument counts


def stack_at(pool, origins, window):
    return torch.stack([pool[s, :, y:y + window, x:x + window] for s, y, x in origins.tolist()]).contiguous()


# ------------------------------------------------------------------------------------------ loader
@pytest.mark.parametrize("image_size,zero_pad", [(8, 0), (6, 2)])
def test_resident_loader_lists_the_windows_the_host_loader_cuts(image_size, zero_pad):
    from maskedsst_amd.data import ResidentTileLoader, SyntheticCubeLoader
    kw = dict(image_size=image_size, tile_size=16, pool_tiles=5, steps=3, seed=11, device="cpu", zero_pad_bands=zero_pad)
    host = SyntheticCubeLoader(7, 20, **kw)
    res = ResidentTileLoader(7, 20, **kw)
    steps = 0
    for img, (tiles, origins) in zip(host, res):
        assert tiles is res.pool and tuple(tiles.shape) == (5, 20, 16, 16) and tiles.dtype == torch.float32
        assert origins.dtype == torch.int32 and tuple(origins.shape) == (7, 3)
        assert len({tuple(r[1:]) for r in origins.tolist()}) == 1   # crop="batch": one position per batch
        assert torch.equal(stack_at(tiles, origins, image_size), img), steps
        steps += 1
    assert steps == 3
    with pytest.raises(StopIteration):
        next(res)
    host.close()
    res.close()
    assert np.array_equal(res.pool.numpy(), host.pool)
    if zero_pad:
        assert float(res.pool[:, -zero_pad:].abs().max()) == 0.0


def test_resident_loader_full_tile_windows_and_bad_crop():
    from maskedsst_amd.data import ResidentTileLoader
    ld = ResidentTileLoader(3, 10, image_size=8, tile_size=8, pool_tiles=4, steps=1, seed=2, device="cpu")
    _, origins = next(ld)
    assert origins[:, 1:].abs().max() == 0   # the window is the tile: nothing to draw
    with pytest.raises(ValueError, match="crop"):
        ResidentTileLoader(3, 10, device="cpu", crop="tile")


def test_resident_loader_crop_sample_draws_a_position_per_window():
    from maskedsst_amd.data import ResidentTileLoader
    ld = ResidentTileLoader(32, 10, image_size=8, tile_size=16, pool_tiles=6, steps=4, seed=3, device="cpu", crop="sample")
    again = ResidentTileLoader(32, 10, image_size=8, tile_size=16, pool_tiles=6, steps=4, seed=3, device="cpu", crop="sample")
    seen = []
    for (tiles, origins), (_, o2) in zip(ld, again):
        assert torch.equal(origins, o2)   # reproducible under the seed
        assert origins.dtype == torch.int32 and tuple(origins.shape) == (32, 3)
        assert 0 <= int(origins[:, 0].min()) and int(origins[:, 0].max()) < 6
        assert 0 <= int(origins[:, 1:].min()) and int(origins[:, 1:].max()) + 8 <= 16   # inside the tiles
        assert len({tuple(r[1:]) for r in origins.tolist()}) > 8   # the positions differ per row
        assert stack_at(tiles, origins, 8).shape == (32, 10, 8, 8)
        seen.append(origins)
    assert len(seen) == 4 and not torch.equal(seen[0], seen[1])


# ------------------------------------------------------------------------------------------ C ABI
def test_c_abi_declares_and_exports_the_three_calls():
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
    # the declared ctypes of each argument against the header's C types
    ctype = {"int": "c_int", "float": "c_float", "uint32_t": "c_uint", "long": "c_long"}
    for name in CALLS:
        args = [a.strip() for a in re.search(r"^int %s\(([^;]*)\);" % name, header, re.M).group(1).split(",")]
        for a, t in zip(args, getattr(lib, name).argtypes):
            want = "c_void_p" if "*" in a else ctype[re.sub(r"/\*.*?\*/", "", a).split()[-2]]
            assert t.__name__ == want, (name, a, t)


_SHAPE = dict(Bs=2, Hs=16, Ws=16, window=8, nwin=8, S=2, P=10, split=0)


def _fwd(lib, ptr=4096, origins=4096, **k):
    a = {**_SHAPE, **k}
    return lib.msst_tokenize_at_fwd_masked(ptr, origins, *([ptr] * 8), a["split"], ptr, ptr, ptr, a["Bs"], a["Hs"], a["Ws"], a["window"],
                                           a["nwin"], a["S"], a["P"], None)


def _bwd(lib, ptr=4096, origins=4096, nchunk=2, **k):
    a = {**_SHAPE, **k}
    return lib.msst_tokenize_at_bwd_masked(ptr, origins, *([ptr] * 9), nchunk, *([ptr] * 8), a["split"], ptr, a["Bs"], a["Hs"], a["Ws"],
                                           a["window"], a["nwin"], a["S"], a["P"], None)


def _head(lib, ptr=4096, origins=4096, K=89, **k):
    a = {**_SHAPE, **k}
    return lib.msst_head_at_fwd(ptr, ptr, origins, ptr, ptr, ptr, 1, ptr, ptr, ptr, ptr, a["Bs"], a["Hs"], a["Ws"], a["window"], a["nwin"],
                                a["S"], a["P"], K, None)


def test_the_three_calls_refuse_bad_arguments_before_launch():
    """fake, never dereferenced pointers (or none) and no device: no call can have reached a launch"""
    from maskedsst_amd import _lib
    lib = _lib.load()
    for call in (_fwd, _bwd, _head):
        for bad in (dict(window=9, Hs=32, Ws=32), dict(P=17), dict(window=8, Hs=7), dict(window=8, Ws=7)):
            assert call(lib, **bad) == UNSUPPORTED, (call.__name__, bad)
        for bad in (dict(Bs=0), dict(Hs=0), dict(Ws=0), dict(window=0), dict(S=0), dict(P=0), dict(nwin=-1)):
            assert call(lib, **bad) == BADARG, (call.__name__, bad)
        assert call(lib, ptr=None) == BADARG and call(lib, origins=None) == BADARG   # null buffers, null table
        assert b"_at_" in lib.msst_last_error()
    for call in (_fwd, _bwd):
        assert call(lib, split=96) == BADARG and call(lib, split=-1) == BADARG
    assert _bwd(lib, nwin=0) == BADARG and _bwd(lib, nchunk=0) == BADARG
    assert _head(lib, nwin=0) == BADARG and _head(lib, K=0) == BADARG and _head(lib, K=129) == BADARG   # K beyond the window's tokens
    assert _head(lib, nwin=65536) == UNSUPPORTED                      # one grid row per window
    assert _fwd(lib, window=7, nwin=65536) == UNSUPPORTED             # the generic kernels: likewise
    assert _fwd(lib, nwin=0) == 0   # an empty forward call enqueues nothing


# ------------------------------------------------------------------------------------------ module refusals
def _mim(image_size=8, **kw):
    from maskedsst_amd import ViTSpatialSpectral, SimMIMSpatialSpectral
    enc = ViTSpatialSpectral(
        image_size=image_size, spatial_patch_size=1, spectral_patch_size=10, num_classes=4, dim=96, depth=1, heads=2, mlp_dim=64,
        dropout=0.0, emb_dropout=0.0, channels=20, spectral_pos_embed=False, spectral_pos=torch.arange(2), blockwise_patch_embed=True)
    return SimMIMSpatialSpectral(encoder=enc, **{**dict(masking_ratio=0.7, mask_patch_size=4, tube_masking=True), **kw})


GOOD = torch.tensor([[0, 0, 0], [1, 8, 4], [1, 3, 2]], dtype=torch.int32)   # tiles [2, 20, 16, 12]: y0 <= 8, x0 <= 4


def _tiles():
    return torch.zeros(2, 20, 16, 12)


@pytest.mark.parametrize("shape", [(20, 16, 16), (1, 20, 16, 16, 1), (1, 30, 16, 16), (1, 20, 7, 16), (1, 20, 16, 7), (0, 20, 16, 16)])
def test_forward_at_and_forward_windows_refuse_bad_tiles(shape):
    m = _mim()
    with pytest.raises(ValueError):
        m.forward_at(torch.zeros(*shape), torch.zeros(1, 3, dtype=torch.int32))
    with pytest.raises(ValueError):
        m.forward_windows(torch.zeros(*shape))


def test_forward_at_refuses_tiles_of_another_dtype_and_non_tensors():
    m = _mim()
    for bad in (_tiles().double(), _tiles().half(), _tiles().long()):
        with pytest.raises(ValueError, match="float32"):
            m.forward_at(bad, GOOD)
        with pytest.raises(ValueError, match="float32"):
            m.forward_windows(bad)
    with pytest.raises(ValueError):
        m.forward_at(_tiles().numpy(), GOOD)
    with pytest.raises(ValueError):
        m.forward_windows(_tiles().numpy())


def test_forward_at_refuses_bad_tables():
    m = _mim()
    for bad in (torch.zeros(3, 2, dtype=torch.int32), torch.zeros(3, dtype=torch.int32), torch.zeros(1, 3, 3, dtype=torch.int64),
                GOOD.float(), GOOD.double(), GOOD.tolist()):
        for check in (True, False):   # shape and dtype are checked without reading the table
            with pytest.raises(ValueError, match="origins"):
                m.forward_at(_tiles(), bad, check=check)
    with pytest.raises(ValueError, match="origins"):
        m.forward_at(_tiles(), GOOD[:0])   # no row
    with pytest.raises(ValueError, match="65535"):
        m.forward_at(_tiles(), torch.zeros(65536, 3, dtype=torch.int32))   # more windows than the head's grid holds
    with pytest.raises(ValueError, match="65535"):
        m.forward_windows(torch.zeros(1, 20, 1, 1).expand(16, 20, 8 * 64, 8 * 65))   # 16 * 64 * 65 = 66560 windows (a view: no memory)


@pytest.mark.parametrize("col,value", [(0, 2), (0, -1), (1, 9), (1, -1), (2, 5), (2, -1)])
def test_forward_at_names_the_first_row_out_of_range(col, value):
    o = torch.cat([GOOD, GOOD, GOOD])
    o[4, col] = value
    o[7, col] = value
    with pytest.raises(ValueError, match=r"row 4\b"):
        _mim().forward_at(_tiles(), o)


def test_forward_at_refuses_bad_masks():
    m = _mim()
    T, K = 128, int(0.7 * 128)
    bm, idx = m.draw_masks(3)
    assert tuple(bm.shape) == (3, T) and tuple(idx.shape) == (3, K)
    bad = [(bm[:2], idx[:2]), (bm, idx[:, :-1]), (bm[:, :-1], idx), (bm.to(torch.uint8), idx), (bm, idx.float()), bm, (bm,), (bm, idx, idx),
           (bm.view(3, 2, 64), idx)]
    for masks in bad:
        with pytest.raises(ValueError, match="masks"):
            m.forward_at(_tiles(), GOOD, masks)
    with pytest.raises(ValueError, match="masks"):
        m.forward_windows(_tiles(), (bm, idx))   # 2 tiles x 2 x 1 windows = 4 rows wanted
    assert m.last_masks is None   # a refused call leaves the model as it was


def test_forward_at_refuses_tiles_that_want_a_gradient():
    m = _mim()
    with pytest.raises(NotImplementedError, match="(?i)gradient"):
        m.forward_at(_tiles().requires_grad_(True), GOOD)
    with pytest.raises(NotImplementedError, match="(?i)gradient"):
        m.forward_windows(_tiles().requires_grad_(True))


def test_good_arguments_reach_the_device_check_and_draw_nothing_before_it():
    """a table in range passes the checks and meets the CPU refusal -- before any mask is drawn (the generators stay where they were);
    check=False does not look at the values: a bad row gets as far"""
    from maskedsst_amd._lib import MsstError
    m = _mim()
    bad = GOOD.clone()
    bad[1, 1] = 99
    state, np_state = torch.get_rng_state(), np.random.get_state()[1].copy()
    for o, check in ((GOOD, True), (GOOD.long(), True), (bad, False)):
        with pytest.raises((MsstError, RuntimeError), match="(?i)cuda|cpu|fallback|device"):
            m.forward_at(_tiles(), o, check=check)
    with pytest.raises((MsstError, RuntimeError), match="(?i)cuda|cpu|fallback|device"):
        m.forward_windows(_tiles())
    assert torch.equal(torch.get_rng_state(), state) and np.array_equal(np.random.get_state()[1], np_state)
    assert m.last_masks is None
