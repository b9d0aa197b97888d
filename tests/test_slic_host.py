"""SLIC superpixels and object-based class maps, host side (no GPU needed): the C ABI of the msst_slic_* entry points (additive under
MSST_VERSION 109) and their argument checks (they run before any HIP call, so null pointers and host buffers are enough to see them),
the ValueError / RuntimeError surface of maskedsst_amd/superpixel.py, the flags of finetune.py, and the float64 restatement of
tests/slic_util.py: it agrees with a plain loop over pixels and candidates, it tells itself apart from its mutations at the committed
bars, and its real-valued cases leave at most 1 % of their live pixels under the margin."""
import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch

import slic_util as su

BADARG, UNSUPPORTED = -3, -2   # include/msst.h: MSST_ERR_BADARG, MSST_ERR_UNSUPPORTED


# --------------------------------------------------------------------------------------------------------------------- C ABI
def test_c_abi_declares_and_exports_the_entry_points():
    from ctypes import c_float, c_int, c_long, c_void_p
    from maskedsst_amd import _lib
    header = open(_lib.HEADER_PATH).read()
    assert _lib.header_version() == 109   # additive: the revision does not move
    lib = _lib.load()
    assert lib.msst_version() == 109
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    P = c_void_p
    sigs = {
        # int Bs, int Hs, int Ws, int step, int C
        "msst_slic_scratch_floats": (c_long, [c_int, c_int, c_int, c_int, c_int]),
        # feat, cover, int Bs, int dim, int Hs, int Ws, int step, float hl, centroids, offsets, bias, counts, labels, prev_labels, moved,
        # best, slab, long slab_floats, stream
        "msst_slic_assign": (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, c_float, P, P, P, P, P, P, P, P, P, c_long, P]),
        # slab, long slab_floats, int Bs, int dim, int Hs, int Ws, int step, centroids, offsets, bias, counts, empty, stream
        "msst_slic_update": (c_int, [P, c_long, c_int, c_int, c_int, c_int, c_int, P, P, P, P, P, P]),
        # map, labels, int Bs, int C, int Hs, int Ws, int step, slab, long slab_floats, stream
        "msst_slic_pool": (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, P, c_long, P]),
        # slab, long slab_floats, int Bs, int C, int Hs, int Ws, int step, table, region_classes, stream
        "msst_slic_pool_finish": (c_int, [P, c_long, c_int, c_int, c_int, c_int, c_int, P, P, P]),
        # labels, region_classes, int Bs, int Hs, int Ws, int step, classes, stream
        "msst_slic_broadcast": (c_int, [P, P, c_int, c_int, c_int, c_int, P, P]),
    }
    for name, sig in sigs.items():
        m = re.search(r"^(?:int|long) %s\(([^;]*)\);" % name, header, re.M)
        assert m and len(m.group(1).split(",")) == len(sig[1]), name
        assert name in _lib.declared_symbols() and _lib._SIGS[name] == sig
        assert re.search(r" T %s$" % name, out, re.M)
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == sig
    assert re.search(r"^#define MSST_SLIC_FIT_CHANNELS 98\b", header, re.M)
    import maskedsst_amd
    from maskedsst_amd import superpixel
    assert superpixel.FIT_CHANNELS == 98 and superpixel.STEPS == (4, 8, 16)
    for n in ("Superpixels", "ObjectResult", "SuperpixelScene", "SlicCentres", "fit_superpixels", "superpixel_pool", "superpixel_classify",
              "superpixel_assign", "superpixel_update", "superpixel_scene"):
        assert n in maskedsst_amd.__all__ and hasattr(maskedsst_amd, n), n
    assert maskedsst_amd.Superpixels._fields == ("labels", "centroids", "positions", "counts", "history", "step", "grid")
    assert maskedsst_amd.ObjectResult._fields == ("classes", "region_scores", "region_classes")
    assert maskedsst_amd.SuperpixelScene._fields == ("superpixels", "classes", "region_scores", "cover")
    assert hasattr(maskedsst_amd.ViTSpatialSpectral, "superpixel_scene")
    assert "msst_slic.hip" in __import__("maskedsst_amd.build", fromlist=["SOURCES"]).SOURCES


def _ptr():
    buf = (ctypes.c_char * 1024)()
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)


SIZES_BAD = (dict(Bs=0), dict(Bs=-1), dict(Hs=0), dict(Ws=0), dict(Ws=-3), dict(step=0), dict(step=-8))
SIZES_OVER = (dict(step=1), dict(step=5), dict(step=32), dict(Hs=32769), dict(Ws=40000), dict(Bs=1 << 30, Hs=64, Ws=64))
BIG = 1 << 40


def test_scratch_floats():
    from maskedsst_amd import _lib
    f = _lib.load().msst_slic_scratch_floats
    assert f(2, 17, 33, 8, 98) == 2 * 3 * 5 * 16 * 99 and f(1, 1, 1, 4, 1) == 32 and f(3, 8, 8, 16, 128) == 3 * 16 * 129
    for bad in ((0, 8, 8, 8, 4), (1, 0, 8, 8, 4), (1, 8, -1, 8, 4), (1, 8, 8, 7, 4), (1, 8, 8, 8, 0), (1, 8, 8, 8, 129), (1, 32769, 8, 8, 4),
                (1 << 30, 64, 64, 8, 4)):
        assert f(*bad) == 0, bad


def test_assign_refuses_bad_arguments_before_launch():
    from maskedsst_amd import _lib
    lib = _lib.load()
    buf, p = _ptr()
    names = ("feat", "cover", "centroids", "offsets", "bias", "counts", "labels", "prev_labels", "moved", "best", "slab")

    def call(Bs=2, dim=96, Hs=5, Ws=7, step=8, hl=0.1, slab_floats=BIG, **ptr):
        a = {n: ptr.get(n, p) for n in names}
        return lib.msst_slic_assign(a["feat"], a["cover"], Bs, dim, Hs, Ws, step, hl, a["centroids"], a["offsets"], a["bias"], a["counts"],
                                    a["labels"], a["prev_labels"], a["moved"], a["best"], a["slab"], slab_floats, None)

    null = {n: None for n in names}
    for bad in SIZES_BAD + (dict(dim=0),):
        assert call(**bad) == BADARG and call(**bad, **null) == BADARG, bad
        assert b"msst_slic_assign" in lib.msst_last_error() and b"below 1" in lib.msst_last_error(), bad
    for over in SIZES_OVER + (dict(dim=95), dict(dim=128)):
        assert call(**over) == UNSUPPORTED and call(**over, **null) == UNSUPPORTED, over
        assert b"msst_slic_assign" in lib.msst_last_error(), over
    for hl in (-1.0, float("nan"), float("inf")):
        assert call(hl=hl) == BADARG and b"hl negative" in lib.msst_last_error(), hl
    for S in (4, 8, 16):                                             # the limits themselves are inside
        assert call(step=S, Hs=32768, Ws=3, **null) == BADARG and b"null" in lib.msst_last_error()
    for n in ("feat", "labels"):
        assert call(**{n: None}) == BADARG and b"null" in lib.msst_last_error(), n
    for n in names:
        assert call(**{n: ctypes.c_void_p(p.value + 2)}) == BADARG and b"misaligned" in lib.msst_last_error(), n
    for n in ("labels", "prev_labels"):                              # int64: 8 bytes
        assert call(**{n: ctypes.c_void_p(p.value + 4)}) == BADARG and b"misaligned" in lib.msst_last_error(), n
    for n in ("offsets", "bias", "counts"):
        assert call(**{n: None}) == BADARG and b"centroids without" in lib.msst_last_error(), n
    assert call(prev_labels=None) == BADARG and b"moved without" in lib.msst_last_error()
    need = lib.msst_slic_scratch_floats(2, 5, 7, 8, 98)
    assert call(slab_floats=need - 1) == BADARG and b"slab smaller" in lib.msst_last_error()


def test_update_refuses_bad_arguments_before_launch():
    from maskedsst_amd import _lib
    lib = _lib.load()
    buf, p = _ptr()
    names = ("slab", "centroids", "offsets", "bias", "counts", "empty")

    def call(Bs=2, dim=96, Hs=5, Ws=7, step=8, slab_floats=BIG, **ptr):
        a = {n: ptr.get(n, p) for n in names}
        return lib.msst_slic_update(a["slab"], slab_floats, Bs, dim, Hs, Ws, step, a["centroids"], a["offsets"], a["bias"], a["counts"],
                                    a["empty"], None)

    null = {n: None for n in names}
    for bad in SIZES_BAD + (dict(dim=-1),):
        assert call(**bad) == BADARG and call(**bad, **null) == BADARG and b"msst_slic_update" in lib.msst_last_error(), bad
    for over in SIZES_OVER + (dict(dim=97),):
        assert call(**over) == UNSUPPORTED and call(**over, **null) == UNSUPPORTED and b"msst_slic_update" in lib.msst_last_error(), over
    for n in names:
        if n != "empty":
            assert call(**{n: None}) == BADARG and b"null" in lib.msst_last_error(), n
        assert call(**{n: ctypes.c_void_p(p.value + 2)}) == BADARG and b"misaligned" in lib.msst_last_error(), n
    assert call(slab_floats=lib.msst_slic_scratch_floats(2, 5, 7, 8, 98) - 1) == BADARG and b"slab smaller" in lib.msst_last_error()


def test_pool_calls_refuse_bad_arguments_before_launch():
    from maskedsst_amd import _lib
    lib = _lib.load()
    buf, p = _ptr()

    def pool(Bs=2, C=5, Hs=5, Ws=7, step=4, slab_floats=BIG, **ptr):
        a = {n: ptr.get(n, p) for n in ("map", "labels", "slab")}
        return lib.msst_slic_pool(a["map"], a["labels"], Bs, C, Hs, Ws, step, a["slab"], slab_floats, None)

    def finish(Bs=2, C=5, Hs=5, Ws=7, step=4, slab_floats=BIG, **ptr):
        a = {n: ptr.get(n, p) for n in ("slab", "table", "region_classes")}
        return lib.msst_slic_pool_finish(a["slab"], slab_floats, Bs, C, Hs, Ws, step, a["table"], a["region_classes"], None)

    def broadcast(Bs=2, Hs=5, Ws=7, step=4, **ptr):
        a = {n: ptr.get(n, p) for n in ("labels", "region_classes", "classes")}
        return lib.msst_slic_broadcast(a["labels"], a["region_classes"], Bs, Hs, Ws, step, a["classes"], None)

    for fn, name, ptrs, optional in ((pool, b"msst_slic_pool", ("map", "labels", "slab"), ()),
                                     (finish, b"msst_slic_pool_finish", ("slab", "table", "region_classes"), ("region_classes",)),
                                     (broadcast, b"msst_slic_broadcast", ("labels", "region_classes", "classes"), ())):
        null = {n: None for n in ptrs}
        has_c = fn is not broadcast
        for bad in SIZES_BAD + ((dict(C=0), dict(C=-2)) if has_c else ()):
            assert fn(**bad) == BADARG and fn(**bad, **null) == BADARG and name in lib.msst_last_error(), (name, bad)
        for over in SIZES_OVER + ((dict(C=129),) if has_c else ()):
            assert fn(**over) == UNSUPPORTED and fn(**over, **null) == UNSUPPORTED and name in lib.msst_last_error(), (name, over)
        if has_c:
            assert fn(C=128, **null) == BADARG and b"null" in lib.msst_last_error()
            assert fn(slab_floats=lib.msst_slic_scratch_floats(2, 5, 7, 4, 5) - 1) == BADARG and b"slab smaller" in lib.msst_last_error()
        for n in ptrs:
            if n not in optional:
                assert fn(**{n: None}) == BADARG and b"null" in lib.msst_last_error(), (name, n)
            assert fn(**{n: ctypes.c_void_p(p.value + 2)}) == BADARG and b"misaligned" in lib.msst_last_error(), (name, n)


# --------------------------------------------------------------------------------------------------------- the Python surface
def cpu_superpixels(Bs=2, Hs=6, Ws=5, S=4):
    from maskedsst_amd import Superpixels
    gy, gx = su.grid(Hs, Ws, S)
    return Superpixels(torch.zeros(Bs, Hs, Ws, dtype=torch.int64), torch.zeros(Bs, gy * gx, 96), torch.zeros(Bs, gy * gx, 2),
                       torch.ones(Bs, gy * gx, dtype=torch.int32), torch.zeros(0, 2, dtype=torch.int64), S, (gy, gx))


def test_fit_superpixels_refuses_bad_arguments_before_device_work():
    from maskedsst_amd import SceneEmbedding, fit_superpixels
    good = torch.zeros(2, 96, 6, 5)
    for f in (torch.zeros(2, 95, 6, 5), torch.zeros(96, 6, 5), torch.zeros(2, 96, 0, 5), good.double(), good.permute(0, 1, 3, 2), None, [[0.0]]):
        with pytest.raises(ValueError):
            fit_superpixels(f)
    for cover in (torch.ones(2, 6, 5), torch.ones(2, 6, 4, dtype=torch.int32), torch.ones(1, 6, 5, dtype=torch.int32), "x"):
        with pytest.raises(ValueError):
            fit_superpixels(good, cover=cover)
    for kw in (dict(step=0), dict(step=5), dict(step=32), dict(step=8.0), dict(step=True), dict(step="8"), dict(compactness=-1.0),
               dict(compactness=float("nan")), dict(compactness=float("inf")), dict(compactness="1"), dict(compactness=1e30), dict(iters=-1),
               dict(iters=1.5), dict(iters=True)):
        with pytest.raises(ValueError):
            fit_superpixels(good, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fit_superpixels(good)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fit_superpixels(SceneEmbedding(good, torch.ones(2, 6, 5, dtype=torch.int32)), iters=0)


def test_pool_and_classify_refuse_bad_arguments_before_device_work():
    from maskedsst_amd import ViTSpatialSpectral, superpixel_classify, superpixel_pool, superpixel_scene
    sp = cpu_superpixels()
    good = torch.zeros(2, 4, 6, 5)
    for fn in (superpixel_pool, superpixel_classify):
        for m in (torch.zeros(2, 4, 6, 4), torch.zeros(2, 4, 5, 5), torch.zeros(1, 4, 6, 5), torch.zeros(2, 129, 6, 5), torch.zeros(2, 0, 6, 5),
                  torch.zeros(4, 6, 5), good.double(), good.permute(0, 1, 3, 2), None):
            with pytest.raises(ValueError):
                fn(sp, m)
        for bad in (None, tuple(sp), sp._replace(step=5), sp._replace(step=8), sp._replace(grid=(1, 1)), sp._replace(labels=sp.labels.int()),
                    sp._replace(labels=sp.labels[:, :, :4])):
            with pytest.raises(ValueError):
                fn(bad, good)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(sp, good)
    model = ViTSpatialSpectral(image_size=8, spatial_patch_size=1, spectral_patch_size=10, num_classes=4, dim=96, depth=1, heads=8, mlp_dim=64,
                               channels=50, spectral_pos=torch.arange(5), blockwise_patch_embed=True, precision="fp32")
    scene = torch.zeros(2, 50, 16, 16)
    for kw in (dict(embedding="x"), dict(step=3), dict(compactness=-1), dict(iters=-1), dict(scores=torch.zeros(2, 4, 16)),
               dict(scores=torch.zeros(2, 4, 16, 15)), dict(scores=torch.zeros(1, 4, 16, 16)), dict(scores=torch.zeros(2, 4, 16, 16).double())):
        with pytest.raises(ValueError):
            superpixel_scene(model, scene, **kw)
    with pytest.raises(ValueError):
        model.superpixel_scene(scene, step=12)


def test_low_level_calls_refuse_bad_arguments_before_device_work():
    from maskedsst_amd import SlicCentres, superpixel_assign, superpixel_update
    good = torch.zeros(2, 96, 6, 5)
    n_sp = 2 * 2
    cen = SlicCentres(torch.zeros(2, n_sp, 96), torch.zeros(2, n_sp, 2), torch.zeros(2, n_sp), torch.ones(2, n_sp, dtype=torch.int32))
    with pytest.raises(ValueError):
        superpixel_assign(good, None, 5)
    with pytest.raises(ValueError):
        superpixel_assign(torch.zeros(2, 95, 6, 5), None, 4)
    for bad in (tuple(cen), cen._replace(centroids=torch.zeros(2, n_sp + 1, 96)), cen._replace(offsets=torch.zeros(2, n_sp, 3)),
                cen._replace(bias=torch.zeros(2, n_sp).double()), cen._replace(counts=torch.ones(2, n_sp, dtype=torch.int64))):
        with pytest.raises(ValueError):
            superpixel_assign(good, None, 4, bad, 0.1)
        with pytest.raises(ValueError):
            superpixel_update(torch.zeros(10), (2, 6, 5), 4, bad)
    for hl in (-1.0, float("nan"), "x"):
        with pytest.raises(ValueError):
            superpixel_assign(good, None, 4, cen, hl)
    for prev in (torch.zeros(2, 6, 5), torch.zeros(2, 6, 4, dtype=torch.int64)):
        with pytest.raises(ValueError):
            superpixel_assign(good, None, 4, cen, 0.1, prev_labels=prev)
    for shape in ((2, 6), (2, 0, 5), (2.0, 6, 5)):
        with pytest.raises(ValueError):
            superpixel_update(torch.zeros(10), shape, 4, cen)
    with pytest.raises(ValueError):
        superpixel_update(torch.zeros(10).double(), (2, 6, 5), 4, cen)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        superpixel_assign(good, None, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        superpixel_update(torch.zeros(10), (2, 6, 5), 4, cen)


def test_hl_is_rounded_once_from_float64():
    from maskedsst_amd.superpixel import slic_hl, superpixel_grid
    for S in (4, 8, 16):
        assert slic_hl(S / 2.0, S) == 0.125 and slic_hl(0.0, S) == 0.0
        for c in (0.2, 1.0, 3.7):
            assert slic_hl(c, S) == su.hl_of(c, S) == float(np.float32(0.5 * (c / S) ** 2))
        for Hs, Ws in ((1, 1), (7, 9), (17, 33), (512, 512)):
            assert superpixel_grid(Hs, Ws, S) == su.grid(Hs, Ws, S) == (-(-Hs // S), -(-Ws // S))


def test_finetune_parser_takes_val_superpixel():
    import finetune
    ap = finetune.build_parser()
    assert ap.parse_args(["enmap"]).val_superpixel == 0 and ap.parse_args(["enmap"]).val_superpixel_compactness == 0.2
    a = ap.parse_args(["enmap", "--val-scenes", "4", "--val-every", "1", "--val-superpixel", "8", "--val-superpixel-compactness", "0.5"])
    assert a.val_superpixel == 8 and a.val_superpixel_compactness == 0.5
    with pytest.raises(SystemExit):
        finetune.check_val_superpixel(ap.parse_args(["enmap", "--val-superpixel", "8"]))           # needs --val-scenes and --val-every
    with pytest.raises(SystemExit):
        finetune.check_val_superpixel(ap.parse_args(["enmap", "--val-scenes", "4", "--val-every", "1", "--val-superpixel", "5"]))
    with pytest.raises(SystemExit):
        finetune.check_val_superpixel(ap.parse_args(["enmap", "--val-scenes", "4", "--val-every", "1", "--val-superpixel", "8",
                                                     "--val-superpixel-compactness", "-1"]))
    finetune.check_val_superpixel(a)
    finetune.check_val_superpixel(ap.parse_args(["enmap"]))


# ------------------------------------------------------------------------------------------------ the float64 restatement itself
@pytest.mark.parametrize("S", [4, 8, 16])
def test_restatement_against_a_plain_loop(S):
    rng = np.random.default_rng(S)
    Hs, Ws = (9, 11) if S == 4 else (13, 19) if S == 8 else (20, 35)
    feat = rng.normal(size=(2, 96, Hs, Ws)).astype(np.float32)
    cover = np.ones((2, Hs, Ws), dtype=np.int32)
    feat[0, 5, 1, 2] = np.nan
    feat[1, 7, Hs - 1, Ws - 1] = np.inf
    cover[1, 0, 0] = 0
    labels, cen, hist, trace = su.fit(feat, cover, S, 3.0, 2)
    assert int((labels == -1).sum()) == 3 and hist.shape == (2, 2) and hist[0, 0] > 0
    home = su.home_labels(su.live_map(feat, cover), S)
    assert np.array_equal(trace[0][0], home)
    gy, gx = su.grid(Hs, Ws, S)
    c0 = su.update_loops(feat, cover, home, S, su.new_centres(2, gy * gx))
    for k in ("cent", "off", "bias"):
        assert np.abs(trace[0][1][k] - c0[k]).max() < 1e-12, k
    assert np.array_equal(trace[0][1]["counts"], c0["counts"])
    hl = su.hl_of(3.0, S)
    lab1, best1, _ = su.assign(feat, cover, trace[0][1], S, hl)
    lab2, best2 = su.assign_loops(feat, cover, trace[0][1], S, hl)
    assert np.array_equal(lab1, lab2) and np.array_equal(lab1, trace[1][0]) and su.abs_err(best1, best2) < 1e-12
    c1 = su.update_loops(feat, cover, lab1, S, c0)
    for k in ("cent", "off", "bias"):
        assert np.abs(trace[1][1][k] - c1[k]).max() < 1e-12, k
    # a centre's pixels lie in its own 3 x 3 cells; positions are absolute
    pi, pj = su.cells(Hs, Ws, S)
    m = labels >= 0
    assert (np.abs(labels // gx - pi)[m] <= 1).all() and (np.abs(labels % gx - pj)[m] <= 1).all()
    pos = su.positions(cen, Hs, Ws, S)
    ys = np.broadcast_to(np.arange(Hs)[:, None], (Hs, Ws))
    k = labels[0][m[0]][0]
    assert abs(pos[0, k, 0] - ys[labels[0] == k].mean()) < 1e-12
    # pooling against a loop
    maps = rng.normal(size=(2, 3, Hs, Ws)).astype(np.float32)
    maps[:, 2, :, Ws // 2:] = -np.inf
    table, region, classes = su.pool(maps, labels, gy * gx)
    for b in range(2):
        for k in range(gy * gx):
            px = [(y, x) for y in range(Hs) for x in range(Ws) if labels[b, y, x] == k]
            if not px:
                assert np.isnan(table[b, k]).all() and region[b, k] == -1
                continue
            want = np.array([sum(float(maps[b, c, y, x]) for y, x in px) / len(px) for c in range(3)])
            fin = np.isfinite(want)
            assert np.array_equal(fin, np.isfinite(table[b, k])) and np.abs(want[fin] - table[b, k][fin]).max() < 1e-12
            assert region[b, k] == int(np.argmax(want))
    assert np.array_equal(classes == -1, labels == -1)


def test_restatement_rules():
    # ties go to the lowest id; a centre with count 0 is no candidate; a dead pixel is -1
    feat = np.zeros((1, 96, 4, 12), dtype=np.float32)
    cen = su.new_centres(1, 3)
    cen["off"][:] = 1.5
    cen["counts"][:] = 1
    lab, best, gap = su.assign(feat, None, cen, 4, 0.125)
    assert lab[0, 0].tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2] and gap[0, 0, 5] > 0
    cen["off"][0, :, 1] = [3.5, 1.5, -0.5]                            # centres 0 and 2 mirror each other about the middle cell
    lab, _, gap = su.assign(feat, None, cen, 4, 0.125)
    assert lab[0, 1, 5] == 1 and gap[0, 1, 5] > 0
    cen["counts"][0, 1] = 0                                           # the middle centre has no rows: its cell splits between 0 and 2
    lab, _, gap = su.assign(feat, None, cen, 4, 0.125)
    dead, _, _ = su.assign(feat, None, cen, 4, 0.125, mutate="dead_centre_candidate")
    assert lab[0, :, 4:8].tolist() == [[0, 0, 2, 2]] * 4 and not (gap[0, :, 4:8] == 0).any()
    cen["off"][0, :, 1] = [4.0, 1.5, -1.0]                            # centres at x = 4 and x = 7: x = 5.5 would tie, no pixel does
    cen["off"][0, 2, 1] = -2.0                                        # ... at x = 4 and x = 6: the pixels of column 5 tie
    lab, _, gap = su.assign(feat, None, cen, 4, 0.125)
    high, _, _ = su.assign(feat, None, cen, 4, 0.125, mutate="ties_highest")
    assert bool((gap[0, :, 5] == 0).all()) and lab[0, :, 5].tolist() == [0] * 4 and high[0, :, 5].tolist() == [2] * 4
    feat[0, 3, 2, 2] = np.nan
    lab, best, _ = su.assign(feat, None, cen, 4, 0.125)
    assert lab[0, 2, 2] == -1 and np.isnan(best[0, 2, 2]) and dead[0, 0, 5] == 1
    # an empty centre keeps what it had; count 0
    labels = su.home_labels(su.live_map(feat), 4)
    labels[labels == 1] = 0
    prev = su.new_centres(1, 3)
    prev["cent"][0, 1] = 7.0
    prev["off"][0, 1] = 2.5
    prev["bias"][0, 1] = -3.0
    out = su.update(feat, None, labels, 4, prev)
    assert out["counts"][0].tolist() == [31, 0, 16] and bool((out["cent"][0, 1] == 7.0).all()) and out["bias"][0, 1] == -3.0
    assert out["off"][0, 1].tolist() == [2.5, 2.5] and out["off"][0, 2].tolist() == [1.5, 1.5]
    zero = su.update(feat, None, labels, 4, prev, mutate="empty_zeroed")
    assert bool((zero["cent"][0, 1] == 0).all())


def committed(case):
    bar = su.bars(case)
    assert bar is not None, "profiles/slic_parity_measured.jsonl is not committed: nothing to hold the mutants against"
    return bar


def test_committed_bars_tell_the_mutants_apart():
    """every bar is 4 x a committed measurement, and every mutated restatement lies beyond the bar of a case that is there to catch it
    (or, where the GPU comparison is exact, differs)"""
    seen = set()
    # ---- the exact assignment: no bar, any difference shows
    differs = {m: False for m in ("plus_candidates", "dead_centre_candidate", "ties_highest", "no_bias")}
    for S, shape in ((4, (9, 17)), (8, (17, 33)), (4, (17, 33))):
        feat, cover, dead, cen, hl, prev = su.int_case(shape, S, "corner")
        ref, _, gap = su.assign(feat, cover, cen, S, hl)
        assert (gap == 0).any(), "the exact cases hold ties"
        for m in differs:
            differs[m] |= not np.array_equal(su.assign(feat, cover, cen, S, hl, mutate=m)[0], ref)
    assert all(differs.values()), differs
    seen |= set(differs)
    # ---- the exact update and the exact pooling
    feat, cover, dead, cen, hl, prev = su.int_case((17, 33), 8, "cell")
    labels, _, _ = su.assign(feat, cover, cen, 8, hl)
    ref = su.update(feat, cover, labels, 8, cen)
    assert (ref["counts"] == 0).any() and (labels == -1).any()
    for m in ("empty_zeroed", "sum_not_divided", "dead_pixel_counted"):
        got = su.update(feat, cover, labels, 8, cen, mutate=m)
        assert any(not np.array_equal(got[k], ref[k]) for k in ref), m
        seen.add(m)
    maps = su.int_maps((17, 33), 17)
    n_sp = int(np.prod(su.grid(17, 33, 8)))
    t0, r0, c0 = su.pool(maps, labels, n_sp)
    t1, r1, c1 = su.pool(maps, labels, n_sp, mutate="pool_across_scenes")
    assert not np.array_equal(np.nan_to_num(t0, neginf=-9e9), np.nan_to_num(t1, neginf=-9e9)) and not np.array_equal(c0, c1)
    seen.add("pool_across_scenes")
    # ---- the real-valued cases: the scores of a mutant lie beyond the bar
    for case in su.REAL_CASES:
        bar = committed(su.case_name(case))
        assert set(bar) == {"score", "centroid", "offset", "bias"} and all(0 < v < 1e-4 for v in bar.values()), bar
        ref = su.teacher_forced(case, iters=2)
        live = ref[1][0] >= 0
        for m in ("no_bias", "compactness_not_squared", "absolute_position"):
            got = su.teacher_forced(case, iters=2, assign_mutate=m) if m == "absolute_position" else su.teacher_forced(case, iters=2, mutate=m)
            assert np.abs(got[1][1] - ref[1][1])[live].max() > bar["score"], (case, m)
            seen.add(m)
        feat, cover = su.real_case(case)
        want = su.update(feat, cover, ref[1][0], case[2], ref[0][3])
        got = su.update(feat, cover, ref[1][0], case[2], ref[0][3], mutate="sum_not_divided")
        assert np.abs(got["cent"] - want["cent"]).max() > bar["centroid"] and np.abs(got["bias"] - want["bias"]).max() > bar["bias"], case
    assert seen == set(su.MUTANTS), sorted(set(su.MUTANTS) - seen)


def test_real_cases_leave_few_pixels_under_the_margin():
    """the labels of a real-valued case are compared on every live pixel whose float64 top-two margin reaches 4 x the measured score
    error: computed from the float64 restatement alone (its centres rounded to fp32 after every update, as a teacher-forced run hands
    them over), at most 1 % of a case's live pixels lie under it, at every iteration"""
    for case in su.REAL_CASES:
        gap = committed(su.case_name(case))["score"]
        trace = su.teacher_forced(case)
        moved = 0
        for (labels, best, margin, cen), (before, _, _, _) in zip(trace[1:], trace[:-1]):
            live = labels >= 0
            assert live.sum() > 900 and (~live).sum() == su.REAL_BS * 15
            under = (margin < gap) & live
            assert under.sum() <= su.MARGIN_SHARE * live.sum(), (case, int(under.sum()), int(live.sum()))
            moved += int((labels != before).sum())
        assert moved > 0, case                                        # the iteration does move pixels
