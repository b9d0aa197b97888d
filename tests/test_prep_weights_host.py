"""msst_prep_weights, host side (no GPU needed): tests/prep_util.py, the reference of tests/test_gpu_prep_weights.py, is itself checked
here (round trip, the index map a bijection, torch's rounding against an integer round-to-nearest-even), then the checks the entry
point makes before it launches anything, and the ctypes declarations against include/msst.h."""
import ctypes
import re

import numpy as np
import pytest
import torch

import prep_util as pu

BADARG = -3   # include/msst.h: MSST_ERR_BADARG


def declared_arguments(header, name):
    """the number of arguments of `name`'s declaration in the header (comments removed)"""
    m = re.search(r"^(?:int|long) %s\(([^;]*)\);" % name, header, re.M)
    assert m, name
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return len([a for a in args.split(",") if a.strip()])


# every whole-fragment 2-byte (logical R, K, pack) the GPU file uses
WHOLE = sorted({pu.logical_shape(r, c, t) + (0,) for r, c, t in pu.SHAPES_PACK0} | {pu.logical_shape(r, c, t) + (1,) for r, c, t in pu.SHAPES_PACK1}
               | {pu.logical_shape(r, c, t) + (p,) for r, c, t, p in pu.SHAPES_REAL}
               | {(32, 64, 0), (32, 64, 1), (64, 32, 0), (64, 32, 1)})   # the scale_rows and special-value jobs


@pytest.mark.parametrize("R,K,pk", WHOLE, ids=lambda v: str(v))
def test_index_map_is_a_bijection_made_of_whole_lanes(R, K, pk):
    idx = pu.frag_index(R, K, pk)
    assert idx.shape == (R, K) and np.array_equal(np.sort(idx.reshape(-1)), np.arange(R * K))
    # a lane holds 8 consecutive k of one row; a fragment holds RB rows x KB k of one block
    assert np.array_equal(idx[:, 0::8] % 8, np.zeros((R, K // 8))) and np.array_equal(idx[:, 7::8] - idx[:, 0::8], np.full((R, K // 8), 7))
    RB, KB = (32, 16) if pk else (16, 32)
    frag = idx // pu.FRAG
    for r0 in range(0, R, RB):
        for k0 in range(0, K, KB):
            assert np.unique(frag[r0:r0 + RB, k0:k0 + KB]).tolist() == [(r0 // RB) * (K // KB) + k0 // KB]
    # the readers' addressing: lane l of the fragment at (row0, k0) finds its row's 8 k at byte l 16 (PBF16::ld_w, ld_w32)
    lane = idx[:RB, :KB] // 8
    want = (np.arange(KB)[None, :] // 8) * RB + np.arange(RB)[:, None]
    assert np.array_equal(lane, want)


def test_index_map_refuses_partial_fragments():
    for r, c, t in pu.SHAPES_PARTIAL0:
        R, K = pu.logical_shape(r, c, t)
        assert not pu.whole_fragments(R, K, 0)
        with pytest.raises(ValueError):
            pu.frag_index(R, K, 0)
    for R, K in [(16, 32), (48, 16), (32, 8), (33, 16)]:
        with pytest.raises(ValueError):
            pu.frag_index(R, K, 1)


@pytest.mark.parametrize("elem", ["bf16", "f16", "f32"])
def test_unpack_inverts_pack(elem):
    if elem == "f32":
        cases = [(r, c, t, p) for r, c in pu.SHAPES_F32 for t in (0, 1) for p in (0, 1)]
    else:
        cases = [(r, c, t, 0) for r, c, t in pu.SHAPES_PACK0] + [(r, c, t, 1) for r, c, t in pu.SHAPES_PACK1] + pu.SHAPES_REAL
    for rows, cols, tr, pk in cases:
        x = pu.fill_distinct(rows, cols, elem)
        n = rows * cols
        if n <= 50000:
            assert len(np.unique(x.view(torch.int32).numpy())) == n, (rows, cols)
        if elem != "f32":   # exact in the destination type
            assert torch.equal(x.to(pu.ELEMS[elem][0]).float(), x)
        bits = pu.pack(x, tr, pk, 0, 1.0, elem)
        assert bits.dtype == pu.ELEMS[elem][1] and bits.shape == (n,)
        back = pu.unpack(bits, rows, cols, tr, pk, elem)
        assert torch.equal(back.view(torch.int32), x.view(torch.int32)), (rows, cols, tr, pk)
        # a scale of 2^-3 on the first rows: still exact, so unpack returns the scaled source
        k = rows // 2 + 1
        back = pu.unpack(pu.pack(x, tr, pk, k, 0.125, elem), rows, cols, tr, pk, elem)
        want = x.clone()
        want[:k] *= 0.125
        assert torch.equal(back, want), (rows, cols, tr, pk)


def test_pack_scales_source_rows_before_the_one_rounding():
    x = pu.fill_random(32, 64, 3)
    for elem in ("bf16", "f16"):
        tdt = pu.ELEMS[elem][0]
        for tr in (0, 1):
            got = pu.unpack(pu.pack(x, tr, 0, 5, 0.3, elem), 32, 64, tr, 0, elem)
            once = x.clone()
            once[:5] = (x[:5] * torch.tensor(0.3)).to(tdt).float()
            once[5:] = x[5:].to(tdt).float()
            assert torch.equal(got, once)
            twice = (x[:5].to(tdt).float() * torch.tensor(0.3)).to(tdt).float()
            assert not torch.equal(twice, once[:5]), "0.3 is there to tell the two orders apart"
    # scale_rows past the end scales everything, 0 and negative nothing
    assert np.array_equal(pu.pack(x, 0, 0, 37, 0.3, "f32"), pu.pack(x, 0, 0, 32, 0.3, "f32"))
    assert np.array_equal(pu.pack(x, 1, 0, 0, 0.3, "f32"), pu.pack(x, 1, 0, -2, 0.3, "f32"))
    assert np.array_equal(pu.pack(x, 1, 0, 0, 0.3, "f32"), x.t().contiguous().view(torch.int32).numpy().reshape(-1))


@pytest.mark.parametrize("elem", ["bf16", "f16"])
def test_torch_rounding_is_round_to_nearest_even(elem):
    """torch's CPU conversion, the reference of the GPU tests, against rne_bits on the special values, the fp32 denormals and 20000
    random bit patterns"""
    tdt, mb = pu.ELEMS[elem][0], 7 if elem == "bf16" else 10
    rng = np.random.default_rng(17)
    pats = pu.SPECIAL["f32"] + pu.DENORMALS + rng.integers(0, 1 << 32, 20000, dtype=np.uint64).tolist()
    if elem == "f16":   # and a dense stretch across half's subnormal / normal boundary and its overflow threshold
        pats += list(range(pu._f(2.0 ** -14) - 3000, pu._f(2.0 ** -14) + 3000, 7)) + list(range(pu._f(65520.0) - 50, pu._f(65520.0) + 50))
    x = pu._from_bits(np.array(pats, dtype=np.uint32))
    got = x.to(tdt).view(torch.int16).numpy().astype(np.int64) & 0xFFFF
    want = np.array([pu.rne_bits(int(u), mb) for u in pats], dtype=np.int64)
    nan = pu.is_nan32(np.array(pats, dtype=np.uint32).view(np.int32))
    assert np.array_equal(pu.is_nan16(got, elem), nan) and np.array_equal(pu.is_nan16(want, elem), nan)
    bad = np.nonzero((got != want) & ~nan)[0]
    assert bad.size == 0, [(hex(pats[i]), hex(got[i]), hex(want[i])) for i in bad[:8]]
    # the named cases, spelled out
    one = {"bf16": 0x3F80, "f16": 0x3C00}[elem]
    eps = 2.0 ** -8 if elem == "bf16" else 2.0 ** -11
    r = lambda v: pu.rne_bits(pu._f(v), mb)   # noqa: E731
    assert r(1 + eps) == one and r(1 + 3 * eps) == one + 2 and r(-(1 + eps)) == 0x8000 | one
    assert pu.rne_bits(pu._f(1 + eps) + 1, mb) == one + 1 and pu.rne_bits(pu._f(1 + 3 * eps) - 1, mb) == one + 1
    if elem == "bf16":
        assert pu.rne_bits(0x7F7FFFFF, mb) == 0x7F80 and pu.rne_bits(0x7F7F8000, mb) == 0x7F80 and pu.rne_bits(0x7F7F7FFF, mb) == 0x7F7F
        assert pu.rne_bits(0x00400000, mb) == 0x0040 and pu.rne_bits(0x807FFFFF, mb) == 0x8080 and pu.rne_bits(0x00000001, mb) == 0
    else:
        assert r(65504.0) == 0x7BFF and pu.rne_bits(pu._f(65520.0) - 1, mb) == 0x7BFF and r(65520.0) == 0x7C00 and r(1e6) == 0x7C00
        assert r(2.0 ** -25) == 0 and r(-2.0 ** -25) == 0x8000 and pu.rne_bits(pu._f(2.0 ** -25) + 1, mb) == 1
        assert r(2.0 ** -24) == 1 and r(3 * 2.0 ** -25) == 2 and r(6e-8) == 1 and r(1e-6) == 17 and r(2.0 ** -14) == 0x0400
        assert all(pu.rne_bits(u, mb) == (u >> 16) & 0x8000 for u in pu.DENORMALS)


# ----------------------------------------------------------------------------------------------- the entry point, before the launch
def test_entry_point_refuses_on_the_host_before_any_launch():
    """the three checks run before anything is enqueued: no device is needed to see them.  In the order of the entry point: a table of
    another header revision (whatever else is passed), nothing to do, a null table"""
    from maskedsst_amd import _lib
    lib = _lib.load()
    nbytes = ctypes.sizeof(_lib.MsstPrepJob)
    table = (_lib.MsstPrepJob * 2)()    # host memory: never dereferenced by the calls below
    tab = ctypes.cast(table, ctypes.c_void_p)
    for bad in (nbytes - 8, nbytes + 8, nbytes - 1, 0, -nbytes):
        for jobs, n in ((tab, 2), (None, 2), (tab, 0), (None, -1)):
            for prec in (_lib.PREC_F32, _lib.PREC_BF16):
                assert lib.msst_prep_weights(jobs, n, bad, 512, prec, None, None) == BADARG, (bad, n)
                assert b"msst_prep_weights" in lib.msst_last_error()
    for n in (0, -1, -(1 << 31)):
        assert lib.msst_prep_weights(tab, n, nbytes, 512, _lib.PREC_BF16, None, None) == 0, n
        assert lib.msst_prep_weights(None, n, nbytes, 0, _lib.PREC_F32, None, None) == 0, n
    for n in (1, 2, 1000):
        assert lib.msst_prep_weights(None, n, nbytes, 512, _lib.PREC_BF16, None, None) == BADARG, n
        assert b"msst_prep_weights" in lib.msst_last_error()


def test_ctypes_declarations_agree_with_the_header():
    from maskedsst_amd import _lib
    header = open(_lib.HEADER_PATH).read()
    m = re.search(r"typedef struct MsstPrepJob \{(.*?)\}\s*MsstPrepJob;", header, re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []   # (C type, name) in declaration order
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = re.match(r"(const float\*|void\*|int32_t|float)\s+(.*)$", decl, re.S).groups()
        fields += [(ctype, n.strip()) for n in names.split(",")]
    ctype_of = {"const float*": ctypes.c_void_p, "void*": ctypes.c_void_p, "int32_t": ctypes.c_int32, "float": ctypes.c_float}
    assert [n for _, n in fields] == ["src", "dst", "rows", "cols", "transpose", "pack", "scale_rows", "scale"]
    assert _lib.MsstPrepJob._fields_ == [(n, ctype_of[t]) for t, n in fields]
    # two pointers, five int32, one float, no padding
    assert ctypes.sizeof(_lib.MsstPrepJob) == 40 == sum(ctypes.sizeof(t) for _, t in _lib.MsstPrepJob._fields_)
    assert [getattr(_lib.MsstPrepJob, n).offset for n, _ in _lib.MsstPrepJob._fields_] == [0, 8, 16, 20, 24, 28, 32, 36]
    # the call: (jobs, njobs, job_bytes, max_elems, prec, err_flag, stream)
    P, I = ctypes.c_void_p, ctypes.c_int
    assert _lib._SIGS["msst_prep_weights"] == (I, [P, I, I, I, I, P, P])
    assert declared_arguments(header, "msst_prep_weights") == 7
    assert re.search(r"^int msst_prep_weights\(const MsstPrepJob\* jobs, int njobs, int job_bytes, int max_elems, int prec, int32_t\* err_flag, "
                     r"void\* stream\);", header, re.M)
    lib = _lib.load()
    assert (lib.msst_prep_weights.restype, list(lib.msst_prep_weights.argtypes)) == _lib._SIGS["msst_prep_weights"]
    m = re.search(r"^#define\s+MSST_PREP_HALF\s+(\d+)", header, re.M)
    assert m and int(m.group(1)) == _lib.PREP_HALF == 256
    for name, want in (("MSST_PREC_F32", _lib.PREC_F32), ("MSST_PREC_BF16", _lib.PREC_BF16)):
        assert int(re.search(r"^#define\s+%s\s+(\d+)" % name, header, re.M).group(1)) == want
    # the documented meaning of the error word covers both packings
    doc = re.search(r"/\* Converts / transposes all matrices.*?\*/", header, re.S).group(0)
    assert "pack = 0" in doc and "pack = 1" in doc and "stay unwritten" in doc
