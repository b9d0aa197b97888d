"""Connected regions of class maps, host side (no GPU needed): the C ABI of msst_regions_label, msst_regions_merge and
msst_regions_scratch_bytes (additive under MSST_VERSION 109) and their argument checks (they run before any HIP call, so null pointers
and host buffers are enough to see them), the ValueError / RuntimeError surface of maskedsst_amd/regions.py, the new flags of
finetune.py, and the numpy restatement of tests/region_util.py itself: against scipy.ndimage.label run per value, against a second,
naive pairwise-union loop, on hand-built maps whose answer is written down here, and against its mutants -- each of which must differ
from it on at least one committed case."""
import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch

import region_util as ru

BADARG, UNSUPPORTED = -3, -2   # include/msst.h: MSST_ERR_BADARG, MSST_ERR_UNSUPPORTED
BIG = 1 << 50


# --------------------------------------------------------------------------------------------------------------------- C ABI
def test_c_abi_declares_and_exports_the_entry_points():
    from ctypes import c_int, c_long, c_void_p
    from maskedsst_amd import _lib
    header = open(_lib.HEADER_PATH).read()
    assert _lib.header_version() == 109   # additive: the revision does not move
    lib = _lib.load()
    assert lib.msst_version() == 109
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    P = c_void_p
    sigs = {
        # int Bs, int Hs, int Ws
        "msst_regions_scratch_bytes": (c_long, [c_int, c_int, c_int]),
        # values, int Bs, int Hs, int Ws, int connectivity, labels, sizes, count, scratch, long scratch_bytes, stream
        "msst_regions_label": (c_int, [P, c_int, c_int, c_int, c_int, P, P, P, P, c_long, P]),
        # values, labels, sizes, int Bs, int Hs, int Ws, int connectivity, int mode, int min_size, int step, values_out, history, scratch,
        # long scratch_bytes, stream
        "msst_regions_merge": (c_int, [P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, P, P, c_long, P]),
    }
    for name, sig in sigs.items():
        m = re.search(r"^(?:int|long) %s\(([^;]*)\);" % name, header, re.M)
        assert m and len(m.group(1).split(",")) == len(sig[1]), name
        assert name in _lib.declared_symbols() and _lib._SIGS[name] == sig
        assert re.search(r" T %s$" % name, out, re.M)
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == sig
    import maskedsst_amd
    from maskedsst_amd import regions
    for n in ("Regions", "SieveResult", "ConnectedSuperpixels", "label_regions", "region_ids", "check_regions", "sieve_classes",
              "enforce_connectivity"):
        assert n in maskedsst_amd.__all__ and hasattr(maskedsst_amd, n), n
    assert maskedsst_amd.Regions._fields == ("labels", "sizes", "count", "connectivity", "error")
    assert maskedsst_amd.SieveResult._fields == ("classes", "regions", "history")
    assert maskedsst_amd.ConnectedSuperpixels._fields == ("superpixels", "regions", "history")
    assert (regions.MODE_SIEVE, regions.MODE_FRAGMENTS) == (0, 1)
    assert "msst_regions.hip" in __import__("maskedsst_amd.build", fromlist=["SOURCES"]).SOURCES


def _ptr():
    buf = (ctypes.c_char * 1024)()
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)


SIZES_BAD = (dict(Bs=0), dict(Bs=-1), dict(Hs=0), dict(Ws=0), dict(Ws=-3))
SIZES_OVER = (dict(Hs=32769), dict(Ws=40000), dict(Hs=32768, Ws=32768 * 2), dict(Bs=1 << 30, Hs=64, Ws=64))


def test_scratch_bytes():
    from maskedsst_amd import _lib
    f = _lib.load().msst_regions_scratch_bytes
    assert f(1, 1, 1) == 16 + 32 and f(3, 17, 33) == 16 + 32 * 3 * 17 * 33 and f(1, 32768, 32768) == 16 + 32 * 32768 * 32768   # Hs Ws < 2^31 follows from the sides
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, -1), (1, 32769, 8), (1, 8, 32769), (1 << 27, 64, 64), (1 << 30, 64, 64)):
        assert f(*bad) == 0, bad


def test_label_refuses_bad_arguments_before_launch():
    from maskedsst_amd import _lib
    lib = _lib.load()
    buf, p = _ptr()
    names = ("values", "labels", "sizes", "count", "scratch")

    def call(Bs=2, Hs=5, Ws=7, connectivity=4, scratch_bytes=BIG, **ptr):
        a = {n: ptr.get(n, p) for n in names}
        return lib.msst_regions_label(a["values"], Bs, Hs, Ws, connectivity, a["labels"], a["sizes"], a["count"], a["scratch"], scratch_bytes,
                                      None)

    null = {n: None for n in names}
    for bad in SIZES_BAD:
        assert call(**bad) == BADARG and call(**bad, **null) == BADARG, bad
        assert b"msst_regions_label" in lib.msst_last_error() and b"below 1" in lib.msst_last_error(), bad
    for over in SIZES_OVER:
        assert call(**over) == UNSUPPORTED and call(**over, **null) == UNSUPPORTED, over
        assert b"msst_regions_label" in lib.msst_last_error(), over
    for c in (0, 1, 6, -4, 16):
        assert call(connectivity=c) == BADARG and b"connectivity" in lib.msst_last_error(), c
    assert call(Hs=32768, Ws=3, **null) == BADARG and b"null" in lib.msst_last_error()         # the limit itself is inside
    for n in names:
        assert call(**{n: None}) == BADARG and b"null" in lib.msst_last_error(), n
        assert call(**{n: ctypes.c_void_p(p.value + 2)}) == BADARG and b"misaligned" in lib.msst_last_error(), n
    for n in ("values", "labels", "scratch"):                          # int64: 8 bytes; the scratch: 16
        assert call(**{n: ctypes.c_void_p(p.value + 4)}) == BADARG and b"misaligned" in lib.msst_last_error(), n
    assert call(scratch=ctypes.c_void_p(p.value + 8)) == BADARG and b"misaligned" in lib.msst_last_error()
    need = lib.msst_regions_scratch_bytes(2, 5, 7)
    assert call(scratch_bytes=need - 1) == BADARG and b"scratch smaller" in lib.msst_last_error()


def test_merge_refuses_bad_arguments_before_launch():
    from maskedsst_amd import _lib
    lib = _lib.load()
    buf, p = _ptr()
    buf2, p2 = _ptr()
    names = ("values", "labels", "sizes", "values_out", "history", "scratch")

    def call(Bs=2, Hs=5, Ws=7, connectivity=8, mode=0, min_size=3, step=4, scratch_bytes=BIG, **ptr):
        a = {n: ptr.get(n, p2 if n == "values_out" else p) for n in names}
        return lib.msst_regions_merge(a["values"], a["labels"], a["sizes"], Bs, Hs, Ws, connectivity, mode, min_size, step, a["values_out"],
                                      a["history"], a["scratch"], scratch_bytes, None)

    null = {n: None for n in names}
    for bad in SIZES_BAD + (dict(min_size=0), dict(min_size=-2), dict(mode=1, step=0), dict(mode=1, step=-4)):
        assert call(**bad) == BADARG and call(**bad, **null) == BADARG, bad
        assert b"msst_regions_merge" in lib.msst_last_error() and b"below 1" in lib.msst_last_error(), bad
    assert call(mode=1, min_size=0, **null) == BADARG and b"null" in lib.msst_last_error()     # min_size is not read in mode 1
    assert call(mode=0, step=0, **null) == BADARG and b"null" in lib.msst_last_error()         # step is not read in mode 0
    for over in SIZES_OVER:
        assert call(**over) == UNSUPPORTED and call(**over, **null) == UNSUPPORTED, over
        assert b"msst_regions_merge" in lib.msst_last_error(), over
    for c in (0, 2, 5, 9):
        assert call(connectivity=c) == BADARG and b"connectivity" in lib.msst_last_error(), c
    for m in (-1, 2):
        assert call(mode=m) == BADARG and b"mode" in lib.msst_last_error(), m
    for n in names:
        assert call(**{n: None}) == BADARG and b"null" in lib.msst_last_error(), n
        assert call(**{n: ctypes.c_void_p(p.value + 2)}) == BADARG and b"misaligned" in lib.msst_last_error(), n
    for n in ("values", "labels", "values_out", "scratch"):
        assert call(**{n: ctypes.c_void_p(p.value + 4)}) == BADARG and b"misaligned" in lib.msst_last_error(), n
    assert call(values_out=p) == BADARG and b"values_out == values" in lib.msst_last_error()
    need = lib.msst_regions_scratch_bytes(2, 5, 7)
    assert call(scratch_bytes=need - 1) == BADARG and b"scratch smaller" in lib.msst_last_error()


# --------------------------------------------------------------------------------------------------------- the Python surface
def cpu_superpixels(Bs=2, Hs=6, Ws=5, S=4):
    from maskedsst_amd import Superpixels
    gy, gx = ru.grid(Hs, Ws, S)
    return Superpixels(torch.zeros(Bs, Hs, Ws, dtype=torch.int64), torch.zeros(Bs, gy * gx, 96), torch.zeros(Bs, gy * gx, 2),
                       torch.ones(Bs, gy * gx, dtype=torch.int32), torch.zeros(0, 2, dtype=torch.int64), S, (gy, gx))


BAD_MAPS = (torch.zeros(2, 6, 5), torch.zeros(2, 6, 5, dtype=torch.int32), torch.zeros(6, 5, dtype=torch.int64),
            torch.zeros(1, 2, 6, 5, dtype=torch.int64), torch.zeros(2, 0, 5, dtype=torch.int64),
            torch.zeros(2, 5, 6, dtype=torch.int64).permute(0, 2, 1), None, [[[0]]])


def test_label_and_sieve_refuse_bad_arguments_before_device_work():
    from maskedsst_amd import Regions, check_regions, label_regions, region_ids, sieve_classes
    good = torch.zeros(2, 6, 5, dtype=torch.int64)
    for v in BAD_MAPS:
        with pytest.raises(ValueError):
            label_regions(v)
        with pytest.raises(ValueError):
            sieve_classes(v, 4)
    with pytest.raises(ValueError):                                   # over the limits
        label_regions(torch.zeros(1, 32769, 1, dtype=torch.int64))
    for c in (0, 6, 16, 4.0, "4", True, None):
        with pytest.raises(ValueError):
            label_regions(good, connectivity=c)
        with pytest.raises(ValueError):
            sieve_classes(good, 4, connectivity=c)
    for m in (0, -1, 2.0, "3", True, None, 2 ** 31):
        with pytest.raises(ValueError):
            sieve_classes(good, m)
    for r in (-1, 1.5, "2", True, None):
        with pytest.raises(ValueError):
            sieve_classes(good, 4, rounds=r)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        label_regions(good)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sieve_classes(good, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sieve_classes(good, 1, rounds=0)
    reg = Regions(good, torch.zeros(2, 6, 5, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), 4, torch.zeros(1, dtype=torch.int32))
    for bad in (None, tuple(reg), reg._replace(labels=good.int()), reg._replace(sizes=good), reg._replace(sizes=reg.sizes[:, :, :4])):
        with pytest.raises(ValueError):
            region_ids(bad)
        with pytest.raises(ValueError):
            check_regions(bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        region_ids(reg)


def test_enforce_connectivity_refuses_bad_arguments_before_device_work():
    from maskedsst_amd import enforce_connectivity
    sp = cpu_superpixels()
    feat = torch.zeros(2, 96, 6, 5)
    for bad in (None, tuple(sp), sp.labels, sp._replace(step=5), sp._replace(step=8), sp._replace(grid=(1, 1)), sp._replace(labels=sp.labels.int()),
                sp._replace(labels=sp.labels[:, :, :4]), sp._replace(labels=sp.labels[0])):
        with pytest.raises(ValueError):
            enforce_connectivity(bad)
    for f in (torch.zeros(2, 95, 6, 5), torch.zeros(2, 96, 6, 4), torch.zeros(1, 96, 6, 5), feat.double(), feat.permute(0, 1, 3, 2), "x"):
        with pytest.raises(ValueError):
            enforce_connectivity(sp, f)
    for kw in (dict(connectivity=6), dict(connectivity=True), dict(rounds=-1), dict(rounds=2.0)):
        with pytest.raises(ValueError):
            enforce_connectivity(sp, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enforce_connectivity(sp)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enforce_connectivity(sp, feat, connectivity=8, rounds=0)


def test_finetune_parser_takes_the_region_flags():
    import finetune
    ap = finetune.build_parser()
    d = ap.parse_args(["enmap"])
    assert d.val_sieve == 0 and d.val_sieve_connectivity == 4 and d.val_superpixel_connect is False
    base = ["enmap", "--val-scenes", "4", "--val-every", "1"]
    a = ap.parse_args(base + ["--val-sieve", "9", "--val-sieve-connectivity", "8"])
    assert a.val_sieve == 9 and a.val_sieve_connectivity == 8
    finetune.check_val_sieve(a)
    finetune.check_val_sieve(d)
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--val-sieve", "9", "--val-sieve-connectivity", "6"])
    with pytest.raises(SystemExit):
        finetune.check_val_sieve(ap.parse_args(["enmap", "--val-sieve", "9"]))                    # needs --val-scenes and --val-every
    with pytest.raises(SystemExit):
        finetune.check_val_sieve(ap.parse_args(base + ["--val-sieve", "-3"]))
    c = ap.parse_args(base + ["--val-superpixel", "8", "--val-superpixel-connect"])
    assert c.val_superpixel_connect is True
    finetune.check_val_superpixel(c)
    with pytest.raises(SystemExit):
        finetune.check_val_superpixel(ap.parse_args(base + ["--val-superpixel-connect"]))        # needs --val-superpixel


# ------------------------------------------------------------------------------------------------------- the restatement itself
LABEL_SHAPES = ((1, 1), (1, 9), (9, 1), (7, 9), (17, 33))


def label_cases():
    """(name, values [Bs, Hs, Ws]): every pattern at small shapes, and batches in which the next scene continues a region"""
    for Hs, Ws in LABEL_SHAPES:
        for name in ru.PATTERNS:
            yield f"{name}-{Hs}x{Ws}", ru.pattern(name, Hs, Ws)[None]
    for seed in range(4):
        yield f"random3-batch-{seed}", np.stack([ru.pattern("random3", 7, 9, seed), ru.pattern("random3", 7, 9, seed + 10)])
    yield "one-batch", np.stack([ru.pattern("one", 5, 6)] * 2)


def test_labelling_against_scipy():
    from scipy import ndimage
    for name, values in label_cases():
        for conn in (4, 8):
            labels, sizes, count = ru.label(values, conn)
            ids, n = ru.ids_of(labels)
            structure = np.ones((3, 3), dtype=int) if conn == 8 else None
            for b in range(values.shape[0]):
                firsts = []
                for v in np.unique(values[b][values[b] >= 0]):
                    comp, k = ndimage.label(values[b] == v, structure=structure)
                    firsts += [(int(np.flatnonzero(comp.ravel() == c + 1)[0]), v, c + 1, comp) for c in range(k)]
                firsts.sort(key=lambda f: f[0])                     # scipy numbers in raster order of the first pixel; so do we
                want = np.full(values[b].shape, -1, dtype=np.int64)
                for dense, (first, v, c, comp) in enumerate(firsts):
                    want[comp == c] = dense
                    assert labels[b].ravel()[first] == first and sizes[b].ravel()[first] == int((comp == c).sum()), (name, conn)
                assert np.array_equal(ids[b], want), (name, conn)
                assert n[b] == count[b] == len(firsts) and int(sizes[b].sum()) == int((values[b] >= 0).sum()), (name, conn)
                assert np.array_equal(labels[b] == -1, values[b] < 0) and np.array_equal(sizes[b] > 0, labels[b] == np.arange(labels[b].size).reshape(labels[b].shape))


def test_labelling_against_the_pairwise_loop():
    for name, values in label_cases():
        if values.shape[1] * values.shape[2] <= 63:
            for conn in (4, 8):
                assert np.array_equal(ru.label(values, conn)[0], ru.label_pairwise(values, conn)), (name, conn)


def test_known_answers():
    # a checkerboard: every pixel its own region under 4, two regions under 8
    v = ru.pattern("checker", 6, 7)[None]
    assert ru.label(v, 4)[2].tolist() == [42] and ru.label(v, 8)[2].tolist() == [2]
    # diagonal stripes separate 4 from 8
    v = ru.pattern("diagonal", 5, 5)[None]
    assert ru.label(v, 4)[2].tolist() == [25] and ru.label(v, 8)[2].tolist() == [9]
    # the spiral and the serpentine are one long region
    for name in ("spiral", "serpentine"):
        labels, sizes, count = ru.label(ru.pattern(name, 33, 65)[None], 4)
        assert sizes.max() > 33 * 65 // 2 and labels[0, 0, 0] == 0 and sizes[0, 0, 0] == sizes.max(), name
    maps = {n: (v, m) for n, v, m in ru.sieve_maps()}
    # isolated pixels go to the field; min_size = 1 and 0 rounds are identities
    v, m = maps["isolated"]
    out, hist = ru.merge_round(v[None], 4, 0, m)
    assert bool((out == 3).all()) and hist.tolist() == [6, 5, 5, 5]
    assert np.array_equal(ru.merge_round(v[None], 4, 0, 1)[0], v[None])
    # a tie between two fields of 80 pixels: the lowest root wins
    v, m = maps["tie"]
    out, hist = ru.merge_round(v[None], 4, 0, m)
    assert int((v == 0).sum()) == int((v == 1).sum()) == 80 and out[0, 4, 8] == out[0, 4, 9] == 0 and hist.tolist() == [3, 1, 1, 2]
    # a patch whose only neighbours are small waits a round
    v, m = maps["waits"]
    one, h1 = ru.merge_round(v[None], 4, 0, m)
    two, h2 = ru.merge_round(one, 4, 0, m)
    assert one[0, 4, 4] == 2 and one[0, 3, 3] == 0 and h1.tolist() == [3, 2, 1, 8] and bool((two == 0).all()) and h2.tolist() == [2, 1, 1, 1]
    # enclosed by dead pixels: stays; -1 and -2 are kept
    v, m = maps["enclosed"]
    out, hist = ru.merge_round(v[None], 8, 0, m)
    assert np.array_equal(out[0], v) and hist.tolist() == [2, 1, 0, 0]
    # a diagonal contact joins under 8 only
    v, m = maps["diagonal_contact"]
    assert ru.merge_round(v[None], 4, 0, m)[1].tolist() == [5, 3, 3, 5] and ru.merge_round(v[None], 8, 0, m)[1].tolist() == [3, 1, 1, 5]
    frag = dict(ru.fragment_maps())
    # the larger neighbour is not eligible: the orphan goes to the eligible one
    out, hist = ru.merge_round(frag["ineligible_larger"][None], 4, 1, 1, 4)
    assert out[0, 5, 5] == 5 and out[0, 5, 6] == 15
    # two pieces of equal size: the lower root is kept
    out, _ = ru.merge_round(frag["equal_pieces"][None], 4, 1, 1, 4)
    assert out[0, 4, 4] == 5 and out[0, 7, 7] == 6
    # an id >= n_sp and a dead pixel stay and are no targets
    out, _ = ru.merge_round(frag["out_of_range"][None], 4, 1, 1, 4)
    assert out[0, 9, 9] == 16 and out[0, 10, 10] == 99 and out[0, 10, 9] == -1 and out[0, 9, 10] != 16 and out[0, 2, 2] == 0
    # a superpixel in one piece is untouched
    h = ru.home(13, 18, 4)[None]
    assert np.array_equal(ru.merge_round(h, 4, 1, 1, 4)[0], h) and ru.fragments(h, 4, 4) == 0


def merge_cases():
    """(name, values [Bs, Hs, Ws], connectivity, mode, min_size, step)"""
    for name, v, m in ru.sieve_maps():
        for conn in (4, 8):
            yield name, v[None], conn, 0, m, 8
    for conn in (4, 8):
        yield "salt", np.stack([ru.salt_blobs(24, 31, seed=1), ru.salt_blobs(24, 31, seed=2)]), conn, 0, 3, 8
    for name, v in ru.fragment_maps():
        for conn in (4, 8):
            yield name, v[None], conn, 1, 1, 4


def test_every_mutant_differs_on_a_committed_case():
    differs = {m: [] for m in ru.LABEL_MUTANTS + ru.MERGE_MUTANTS}
    for name, values in label_cases():
        for conn in (4, 8):
            ref = ru.label(values, conn)
            for m in ru.LABEL_MUTANTS:
                got = ru.label(values, conn, mutate=m)
                if any(not np.array_equal(a, b) for a, b in zip(ref, got)):
                    differs[m].append((name, conn))
    for name, values, conn, mode, min_size, step in merge_cases():
        ref = ru.merge_round(values, conn, mode, min_size, step)
        for m in ru.MERGE_MUTANTS:
            got = ru.merge_round(values, conn, mode, min_size, step, mutate=m)
            if not np.array_equal(ref[0], got[0]) or not np.array_equal(ref[1], got[1]):
                differs[m].append((name, conn))
    assert all(differs.values()), [m for m, d in differs.items() if not d]
    # and where they were meant to
    assert ("dead_row-7x9", 4) in differs["dead_bridge"] and ("one-batch", 4) in differs["scene_leak"]
    assert ("diagonal-7x9", 4) in differs["conn8_for_4"] and not any(c == 8 for _, c in differs["conn8_for_4"])
    assert ("tie", 4) in differs["ties_highest"] and ("waits", 4) in differs["flagged_target"] and ("waits", 4) in differs["sequential"]
    assert ("ineligible_larger", 4) in differs["no_cell_box"] and ("out_of_range", 4) in differs["keep_lowest_root"]
    assert ("salt", 4) in differs["size_le"]


def test_rounds_reach_a_fixed_point():
    v = np.stack([ru.salt_blobs(24, 31, seed=1), ru.salt_blobs(24, 31, seed=2)])
    out, hist = ru.rounds(v, 4, 5, 0, 4)
    still = [t for t in range(5) if hist[t, 3] == 0]
    assert hist[0, 3] > 0 and still, hist.tolist()
    again, h2 = ru.merge_round(out, 4, 0, 4)
    assert np.array_equal(again, out) and h2[3] == 0 and np.array_equal(out < 0, v < 0) and np.array_equal(out[v < 0], v[v < 0])
