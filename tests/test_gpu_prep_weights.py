"""GPU: msst_prep_weights alone, bit for bit against tests/prep_util.py (int16 views for bf16 / half, int32 views for fp32; the only
leniency is the payload of a NaN), and the job table ``Engine`` builds.

Every destination of every job is a slice of ONE device buffer the test owns, prefilled with 0xFF bytes, with a guard before it and
(ceil(R / 16) ceil(K / 32) + 1) 512 elements from its start on: whatever index a 16 x 32 fragment formula can form from an element
of [R][K] lies inside.  After the call every byte outside the expected destinations must still be 0xFF and the sources unchanged."""
import ctypes

import numpy as np
import pytest
import torch

import prep_util as pu
from util import build_product, record

pytestmark = pytest.mark.gpu

HALF = 256    # include/msst.h: MSST_PREP_HALF
GUARD = 512   # elements of 0xFF in front of every destination


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def job(src, transpose=0, pack=0, scale_rows=0, scale=1.0, rows=None, cols=None, flag=0):
    """one table row: `src` fp32 [rows, cols] on the CPU; rows / cols override what the table says (malformed jobs); flag: the bits
    the kernel must OR in for it (0: a good job, its destination is compared; else it is skipped, its destination stays 0xFF)"""
    return dict(src=src, transpose=transpose, pack=pack, scale_rows=scale_rows, scale=scale, rows=src.shape[0] if rows is None else rows,
                cols=src.shape[1] if cols is None else cols, flag=flag)


def elem_of(prec, pack):
    return "f32" if prec == "fp32" else "f16" if pack & HALF else "bf16"


def _reserve(j):
    rows, cols = max(abs(j["rows"]), j["src"].shape[0]), max(abs(j["cols"]), j["src"].shape[1])
    R, K = pu.logical_shape(rows, cols, j["transpose"])
    return (-(-R // 16) * -(-K // 32) + 1) * pu.FRAG


def run(jobs, prec, max_elems=None, flag_init=0, with_flag=True):
    """lays the jobs out in one 0xFF buffer, calls msst_prep_weights once and returns everything check() needs"""
    from maskedsst_amd import _lib
    lib = _lib.load()
    esz = 4 if prec == "fp32" else 2
    starts, off = [], 0
    for j in jobs:
        off = (off + GUARD + 7) // 8 * 8
        starts.append(off)
        off += _reserve(j)
    total = off + GUARD
    buf = torch.full((total * esz,), 0xFF, dtype=torch.uint8, device="cuda")
    flat = torch.cat([j["src"].reshape(-1) for j in jobs]).contiguous()
    src = flat.cuda()
    table = (_lib.MsstPrepJob * len(jobs))()
    soff = 0
    for t, j, s in zip(table, jobs, starts):
        t.src, t.dst = src.data_ptr() + 4 * soff, buf.data_ptr() + s * esz
        t.rows, t.cols, t.transpose, t.pack, t.scale_rows, t.scale = j["rows"], j["cols"], j["transpose"], j["pack"], j["scale_rows"], j["scale"]
        soff += j["src"].numel()
    dev_table = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).cuda()
    if max_elems is None:   # the true maximum
        max_elems = max([j["rows"] * j["cols"] for j in jobs if j["rows"] > 0 and j["cols"] > 0] + [1])
    flag = torch.tensor([flag_init], dtype=torch.int32, device="cuda") if with_flag else None
    rc = lib.msst_prep_weights(P(dev_table), len(jobs), ctypes.sizeof(_lib.MsstPrepJob), max_elems, _lib.PREC_F32 if prec == "fp32" else _lib.PREC_BF16,
                               P(flag), stream())
    torch.cuda.synchronize()
    assert rc == 0, (rc, lib.msst_last_error())
    assert torch.equal(src.cpu().view(torch.int32), flat.view(torch.int32)), "sources changed"
    assert torch.equal(dev_table.cpu(), torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8)), "job table changed"
    return dict(jobs=jobs, prec=prec, esz=esz, starts=starts, buf=buf.cpu().numpy(), flag=None if flag is None else int(flag.item()), flag_init=flag_init)


def region(res, i):
    """(got bits, expected bits) of job i's destination"""
    j, esz = res["jobs"][i], res["esz"]
    n = j["src"].numel()
    got = res["buf"][res["starts"][i] * esz:(res["starts"][i] + n) * esz].view(np.int32 if esz == 4 else np.int16)
    want = pu.pack(j["src"], j["transpose"], j["pack"] & 1, j["scale_rows"], j["scale"], elem_of(res["prec"], j["pack"]))
    return got, want


def assert_same_bits(got, want, elem, what):
    nan = pu.is_nan32(want) if elem == "f32" else pu.is_nan16(want, elem)
    got_nan = pu.is_nan32(got) if elem == "f32" else pu.is_nan16(got, elem)
    assert np.array_equal(got_nan, nan), (what, "NaNs", np.nonzero(got_nan != nan)[0][:8])
    bad = np.nonzero((got != want) & ~nan)[0]
    assert bad.size == 0, (what, f"{bad.size} of {got.size} elements differ, first at {bad[:8].tolist()}: got "
                           f"{[hex(int(v) & 0xFFFFFFFF) for v in got[bad[:8]]]}, want {[hex(int(v) & 0xFFFFFFFF) for v in want[bad[:8]]]}")


def check(res, compare=True):
    """good jobs hold the reference's bits, everything else in the buffer is still 0xFF, the flag word holds the expected bits"""
    untouched = np.ones(res["buf"].size, dtype=bool)
    for i, j in enumerate(res["jobs"]):
        if j["flag"]:
            continue
        s, n, esz = res["starts"][i], j["src"].numel(), res["esz"]
        untouched[s * esz:(s + n) * esz] = False
        if compare:
            got, want = region(res, i)
            assert_same_bits(got, want, elem_of(res["prec"], j["pack"]), (i, tuple(j["src"].shape), j["transpose"], j["pack"], j["scale_rows"], j["scale"]))
    dirty = np.nonzero((res["buf"] != 0xFF) & untouched)[0]
    assert dirty.size == 0, (f"{dirty.size} bytes written outside the expected destinations, first at bytes {dirty[:4].tolist()}; the destinations "
                             f"start at bytes {[s * res['esz'] for s in res['starts']]}")
    if res["flag"] is not None:
        want = res["flag_init"]
        for j in res["jobs"]:
            want |= j["flag"]
        assert res["flag"] == want, (res["flag"], want)


def fills(rows, cols, elem, seed):
    return [pu.fill_distinct(rows, cols, elem), pu.fill_random(rows, cols, seed)]


# ----------------------------------------------------------------------------------------------- shapes and values
@pytest.mark.parametrize("fill", [0, 1], ids=["distinct", "randn"])
@pytest.mark.parametrize("elem", ["bf16", "f16"])
def test_small_shapes_every_fragment_layout(elem, fill):
    """the smallest shapes at which each mechanism exists, both packs, both orientations: one launch"""
    h = HALF if elem == "f16" else 0
    jobs = [job(fills(r, c, elem, 100 + i)[fill], t, 0 | h) for i, (r, c, t) in enumerate(pu.SHAPES_PACK0)]
    jobs += [job(fills(r, c, elem, 200 + i)[fill], t, 1 | h) for i, (r, c, t) in enumerate(pu.SHAPES_PACK1)]
    check(run(jobs, "bf16"))


@pytest.mark.parametrize("fill", [0, 1], ids=["distinct", "randn"])
@pytest.mark.parametrize("elem", ["bf16", "f16"])
def test_to_qkv_shapes_with_the_softmax_scale(elem, fill):
    """to_qkv at 2 and 8 heads, both orientations and packs, scale_rows = 2 H 64 and scale = 2^-3 (the wqkvT32 job is one of them);
    (1536, 96) takes a second trip through the grid-stride loop"""
    h = HALF if elem == "f16" else 0
    jobs = [job(fills(r, c, elem, 300 + i)[fill], t, p | h, scale_rows=2 * (r // 3), scale=0.125) for i, (r, c, t, p) in enumerate(pu.SHAPES_REAL)]
    assert max(j["src"].numel() for j in jobs) == 147456 > 64 * 256 * 8
    check(run(jobs, "bf16"))


@pytest.mark.parametrize("fill", [0, 1], ids=["distinct", "randn"])
def test_fp32_copies(fill):
    """plain row-major copies and transposes; pack = 1 is legal in fp32 mode and changes nothing"""
    jobs = [job(fills(r, c, "f32", 400 + i)[fill], t, p) for i, (r, c) in enumerate(pu.SHAPES_F32) for t in (0, 1) for p in (0, 1)]
    jobs += [job(fills(r, c, "f32", 450 + i)[fill], t, 0, scale_rows=2 * (r // 3), scale=0.125) for i, (r, c, t, _) in enumerate(pu.SHAPES_REAL[::2])]
    res = run(jobs, "fp32")
    check(res)
    for i in range(0, 4 * len(pu.SHAPES_F32), 2):   # (pack 0, pack 1) pairs: the same bits
        assert np.array_equal(region(res, i)[0], region(res, i + 1)[0])


@pytest.mark.parametrize("prec,half", [("bf16", 0), ("bf16", HALF), ("fp32", 0)], ids=["bf16", "f16", "fp32"])
def test_scale_rows_counts_source_rows_and_the_product_is_rounded_once(prec, half):
    """scale_rows in {0, 1, rows - 1, rows, rows + 5} on an untransposed and a transposed job, both packs; scale 2^-3 and 0.3 -- with
    0.3 "multiply in fp32, round once" differs in bits from "round, then multiply" (tests/test_prep_weights_host.py)"""
    rows, cols = 32, 64
    elem = elem_of(prec, half)
    jobs = []
    for scale in (0.125, 0.3):
        for tr in (0, 1):
            for pk in (0, 1):
                for n, sr in enumerate((0, 1, rows - 1, rows, rows + 5)):
                    src = pu.fill_random(rows, cols, 500 + n) if scale == 0.3 else pu.fill_distinct(rows, cols, elem)
                    jobs.append(job(src, tr, pk | half, scale_rows=sr, scale=scale))
    res = run(jobs, prec)
    check(res)
    # the boundary itself, read back through unpack: row scale_rows - 1 is scaled, row scale_rows is not
    for i, j in enumerate(jobs):
        if j["scale"] == 0.125 and 0 < j["scale_rows"] < rows:
            back = pu.unpack(region(res, i)[0], rows, cols, j["transpose"], j["pack"] & 1, elem)
            sr = j["scale_rows"]
            assert torch.equal(back[sr - 1], j["src"][sr - 1] * 0.125) and torch.equal(back[sr], j["src"][sr])


@pytest.mark.parametrize("prec,half", [("bf16", 0), ("bf16", HALF), ("fp32", 0)], ids=["bf16", "f16", "fp32"])
def test_special_values(prec, half):
    """zeros, infinities, NaNs (compared as "is a NaN"), exact ties in both directions and their fp32 neighbours, the overflow
    thresholds of bf16 and half, half's subnormal results: prep_util.SPECIAL.  No fp32 denormal is among them"""
    elem = elem_of(prec, half)
    bits = pu.SPECIAL[elem]
    assert not any(0 < (u & 0x7FFFFFFF) < 0x00800000 for u in bits)
    jobs = [job(pu.fill_cycle(bits, 32, 64), 0, 0 | half), job(pu.fill_cycle(bits, 32, 64), 1, 1 | half),
            job(pu.fill_cycle(bits[::-1], 64, 32), 1, 0 | half)]
    res = run(jobs, prec)
    check(res)
    got, want = region(res, 0)
    assert (pu.is_nan32(want) if elem == "f32" else pu.is_nan16(want, elem)).any()
    # the named cases once more, by their stored bits (what the reference says they are is checked on the host)
    src_bits = jobs[0]["src"].view(torch.int32).numpy().reshape(-1).view(np.uint32)
    at = pu.frag_index(32, 64, 0).reshape(-1) if elem != "f32" else np.arange(32 * 64)
    named = {"bf16": ((0x7F7FFFFF, 0x7F80), (0x7F7F8000, 0x7F80), (0x7F7F7FFF, 0x7F7F), (0xFF7FFFFF, 0xFF80), (pu._f(1 + 2.0 ** -8), 0x3F80),
                      (pu._f(1 + 3 * 2.0 ** -8), 0x3F82), (0x80000000, 0x8000)),
             "f16": ((pu._f(65504.0), 0x7BFF), (pu._f(65520.0) - 1, 0x7BFF), (pu._f(65520.0), 0x7C00), (pu._f(1e6), 0x7C00), (pu._f(2.0 ** -25), 0),
                     (pu._f(2.0 ** -24), 1), (pu._f(6e-8), 1), (pu._f(1e-6), 17), (pu._f(1 + 2.0 ** -11), 0x3C00), (pu._f(1 + 3 * 2.0 ** -11), 0x3C02),
                     (0x80000000, 0x8000)),
             "f32": ((0x80000000, 0x80000000), (0x7F7FFFFF, 0x7F7FFFFF), (0x00800000, 0x00800000))}[elem]
    for u, r in named:
        pos = np.nonzero(src_bits == u)[0]
        assert pos.size >= 2 and all((int(got[at[a]]) & (0xFFFFFFFF if elem == "f32" else 0xFFFF)) == r for a in pos), hex(u)


@pytest.mark.parametrize("prec,half", [("bf16", 0), ("bf16", HALF), ("fp32", 0)], ids=["bf16", "f16", "fp32"])
def test_fp32_denormal_inputs_are_kept_or_flushed_as_one(prec, half):
    """fp32 denormal inputs, the one exception to "bit for bit": per element either the round-to-nearest-even result or a zero of the
    same sign, and the same choice for every element of a job.  Job 0 converts them as they are; job 1 first multiplies them by 0.5
    (scale_rows = rows), where the product is a denormal too; job 2 multiplies them by 2^110, where the product is a normal number
    unless the multiplication flushed its input (the one job that tells in half, whose results are zeros otherwise).  The outcome is
    recorded (DESIGN.md "Operand copies" holds what an MI355X did: kept, in every job and mode)."""
    elem = elem_of(prec, half)
    src = pu.fill_cycle(pu.DENORMALS, 16, 32)
    src = torch.where(src == 0.5, torch.full_like(src, 2.0 ** -128), src)   # the padding of fill_cycle: denormals only
    assert bool(((src.abs() > 0) & (src.abs() < 2.0 ** -126)).all())
    assert bool((pu.scaled(src, 16, 0.5) != 0).sum() >= 256), "the reference keeps denormals"
    jobs = [job(src, 0, half), job(src, 0, half, scale_rows=16, scale=0.5), job(src, 0, half, scale_rows=16, scale=2.0 ** 110)]
    res = run(jobs, prec)
    check(res, compare=False)
    outcome = {}
    for i, name in enumerate(("converted", "scaled", "scaled_up")):
        got, kept = region(res, i)
        zero = kept & (np.int32(-0x80000000) if elem == "f32" else np.int16(-0x8000))
        assert bool(((got == kept) | (got == zero)).all()), (name, [hex(int(v) & 0xFFFFFFFF) for v in got[(got != kept) & (got != zero)][:8]])
        tells = kept != zero   # elements at which the two outcomes differ (none for half in jobs 0 and 1: every result is a zero)
        if not tells.any():
            outcome[name] = "zero either way"
            continue
        assert tells.sum() >= 256
        is_kept, is_zero = bool((got[tells] == kept[tells]).all()), bool((got[tells] == zero[tells]).all())
        assert is_kept or is_zero, (name, "mixed", int((got[tells] == kept[tells]).sum()), int(tells.sum()))
        outcome[name] = "kept" if is_kept else "flushed"
    print("fp32 denormal inputs,", elem, outcome)
    record("prep_weights_denormals", elem=elem, outcome=outcome)


# ----------------------------------------------------------------------------------------------- one launch, many jobs
def _mixed_table():
    """bf16 mode: eight good jobs of mixed sizes, packs, orientations and element types around one malformed job (pack 3) in the middle"""
    spec = [(384, 96, 1, 1, 0), (16, 32, 0, 0, 0), (96, 64, 0, 0, HALF), (32, 16, 0, 1, HALF), None, (1536, 96, 0, 0, 0), (64, 96, 1, 0, HALF),
            (16, 32, 1, 1, 0), (48, 96, 0, 0, 0)]
    jobs = []
    for i, s in enumerate(spec):
        if s is None:
            jobs.append(job(pu.fill_random(32, 64, 77), 0, 3, flag=1))
            continue
        r, c, t, p, h = s
        jobs.append(job(pu.fill_random(r, c, 600 + i), t, p | h, scale_rows=(2 * (r // 3) if i == 0 else 0), scale=0.125))
    return jobs


def test_one_launch_many_jobs_and_a_too_small_size_hint():
    jobs = _mixed_table()
    assert len([j for j in jobs if not j["flag"]]) >= 6 and jobs[len(jobs) // 2]["flag"] == 1
    full = run(jobs, "bf16")
    check(full)
    # max_elems = 1: one workgroup per job, the grid-stride loop covers it all the same -- identical bytes
    one = run(jobs, "bf16", max_elems=1)
    check(one)
    assert np.array_equal(one["buf"], full["buf"])
    # and a hint far too large
    big = run(jobs, "bf16", max_elems=1 << 24)
    assert np.array_equal(big["buf"], full["buf"]) and big["flag"] == 1


# ----------------------------------------------------------------------------------------------- the flag word
def _good(seed, half=0):
    return job(pu.fill_random(16, 32, seed), 0, half)


FLAG_CASES = {
    # pack values that are no packing: bit value 1
    **{f"pack{p}": ("bf16", dict(pack=p), 1) for p in (-1, 2, 3, 258, 512)},
    "fp32_pack2": ("fp32", dict(pack=2), 1), "fp32_pack-1": ("fp32", dict(pack=-1), 1),
    "rows0": ("bf16", dict(rows=0), 1), "cols0": ("bf16", dict(cols=0), 1), "rows-16": ("bf16", dict(rows=-16), 1), "cols-32": ("bf16", dict(cols=-32), 1),
    "fp32_rows0": ("fp32", dict(rows=0), 1), "fp32_rows-16": ("fp32", dict(rows=-16), 1),
    # the half flag in fp32 mode
    "fp32_half": ("fp32", dict(pack=HALF), 1), "fp32_half_pack1": ("fp32", dict(pack=HALF | 1), 1),
    # 2-byte pack 1 on a destination that is not whole 32 x 16 fragments: bit value 2
    "pack1_R16": ("bf16", dict(pack=1, shape=(16, 32)), 2), "pack1_K8": ("bf16", dict(pack=1, shape=(32, 8)), 2),
    "pack1_K24": ("bf16", dict(pack=1, shape=(32, 24)), 2), "pack1_R33": ("bf16", dict(pack=1, shape=(33, 16)), 2),
    "pack1_T_R16": ("bf16", dict(pack=1, shape=(32, 16), transpose=1), 2), "pack1_half_R48": ("bf16", dict(pack=1 | HALF, shape=(48, 16)), 2),
    # a bad pack wins over the shape
    "pack3_partial": ("bf16", dict(pack=3, shape=(8, 32)), 1),
}


@pytest.mark.parametrize("name", list(FLAG_CASES))
def test_flag_word(name):
    """a malformed job between two good ones: skipped (0xFF everywhere in and around its destination), its bits OR-ed into the word
    -- preset to 4 it comes back as 4 | bits --, the good jobs written; with err_flag = NULL the call returns 0 and still skips it"""
    prec, kw, bits = FLAG_CASES[name]
    kw = dict(kw)
    shape = kw.pop("shape", (16, 32))
    bad = job(pu.fill_random(*shape, 9), kw.pop("transpose", 0), kw.pop("pack", 0), flag=bits, **kw)
    jobs = [_good(1), bad, _good(2, HALF if prec == "bf16" else 0)]
    res = run(jobs, prec)
    check(res)
    assert res["flag"] == bits
    res = run(jobs, prec, flag_init=4)
    check(res)
    assert res["flag"] == 4 | bits
    res = run(jobs, prec, with_flag=False)
    check(res)


def test_flag_word_collects_both_bits_and_stays_zero_for_a_valid_table():
    jobs = [_good(1), job(pu.fill_random(16, 32, 2), 0, 1, flag=2), _good(3, HALF), job(pu.fill_random(16, 32, 4), 0, 7, flag=1), _good(5)]
    res = run(jobs, "bf16")
    check(res)
    assert res["flag"] == 3
    for prec in ("bf16", "fp32"):
        res = run([_good(1), job(pu.fill_random(16, 32, 2), 1, 1), _good(3)], prec)
        check(res)
        assert res["flag"] == 0


# ----------------------------------------------------------------------------------------------- partial fragments, pack 0
@pytest.mark.parametrize("elem", ["bf16", "f16"])
@pytest.mark.parametrize("shape", pu.SHAPES_PARTIAL0, ids=lambda s: "x".join(map(str, s[:2])) + ("T" if s[2] else ""))
def test_pack0_partial_fragments_are_refused(shape, elem):
    """a 2-byte destination [R][K] with R % 16 or K % 32 is no sequence of 16 x 32 fragments: the job is skipped like a partial pack 1
    job -- nothing written in or around its destination, bit value 2 set -- and its neighbours are written.

    Before the check existed such a job ran the element-wise loop with f = (r / 16) (K / 32) + k / 32 on a K that is no multiple of
    32 and without a bound on the fragment: (8, 32) put element (7, 31) at index 447 of a 256-element destination, K = 40 let (0, 32)
    and (16, 0) share fragment 1.  Those writes land in this test's own buffer (the space kept behind every destination)."""
    r, c, t = shape
    h = HALF if elem == "f16" else 0
    jobs = [_good(1, h), job(pu.fill_distinct(r, c, elem), t, h, flag=2), _good(2)]
    res = run(jobs, "bf16")
    check(res)
    assert res["flag"] == 2
    # fp32 destinations have no fragments: the same shape is an ordinary job there
    res = run([job(pu.fill_distinct(r, c, "f32"), t, 0)], "fp32")
    check(res)
    assert res["flag"] == 0


# ----------------------------------------------------------------------------------------------- the engine's job table
def _copies(eng):
    """[(layer, field, master name, transpose, pack, scale_rows, scale, elem)] of every operand copy the engine keeps"""
    from maskedsst_amd import _lib
    inner = eng.enc.heads * 64
    out = []
    for i, (sname, l) in enumerate(eng._layers()):
        lo = "f32" if eng.prec == _lib.PREC_F32 else "bf16"
        for name in ("wqkv", "wout", "w1", "w2"):
            out.append((i, name, f"{sname}.{l}.{name}", 0, 0, 0, 1.0, lo))
            out.append((i, name + "T", f"{sname}.{l}.{name}", 1, 0, 0, 1.0, lo))
        if eng.prec != _lib.PREC_F32:
            out.append((i, "wqkv32", f"{sname}.{l}.wqkv", 0, 1, 0, 1.0, "bf16"))
            out.append((i, "woutT32", f"{sname}.{l}.wout", 1, 1, 0, 1.0, "bf16"))
            out.append((i, "wqkvT32", f"{sname}.{l}.wqkv", 1, 1, 2 * inner, 0.125, "bf16"))   # q and k blocks carry 2^-3, v does not
            for name in ("wqkv", "wout", "w1", "w2"):
                out.append((i, name + "_h", f"{sname}.{l}.{name}", 0, 0, 0, 1.0, "f16"))
    return out


def _assert_copies(eng, skip=()):
    """every copy, located from the pointers of eng._bw as an offset into eng._wbuf, equals pack() of its fp32 master; the copies tile
    the buffer without overlap.  Returns {(layer, field): (byte offset, bytes)}"""
    torch.cuda.synchronize()
    wbuf = eng._wbuf.cpu().numpy()
    base = eng._wbuf.data_ptr()
    where, spans = {}, []
    for i, field, master, tr, pk, sr, scale, elem in _copies(eng):
        src = eng.fp.view(master).detach().cpu()
        esz = 4 if elem == "f32" else 2
        off = int(getattr(eng._bw[i], field)) - base
        nbytes = src.numel() * esz
        assert 0 <= off and off + nbytes <= wbuf.size and off % 16 == 0, (i, field, off)
        where[(i, field)] = (off, nbytes)
        spans.append((off, off + nbytes))
        if (i, field) in skip:
            continue
        got = wbuf[off:off + nbytes].view(np.int32 if esz == 4 else np.int16)
        assert_same_bits(got, pu.pack(src, tr, pk, sr, scale, elem), elem, (i, field))
    spans.sort()
    assert spans[0][0] == 0 and spans[-1][1] == wbuf.size and all(a[1] == b[0] for a, b in zip(spans, spans[1:])), "copies overlap or leave holes"
    return where


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("heads", [2, 8])
def test_engine_copies_follow_the_masters(heads, prec):
    model, _, _ = build_product(dict(bands=20, depth=1, B=2, heads=heads), precision=prec, device="cuda")
    eng = model.engine()
    eng.prep_weights()
    per_layer = 8 if prec == "fp32" else 15
    assert len(_copies(eng)) == 2 * per_layer == eng._njobs
    where = _assert_copies(eng)
    assert len(where) == 2 * per_layer and int(eng._prep_flag.item()) == 0
    if prec == "bf16":   # the scale sits in the q and k blocks of wqkvT32 and nowhere else
        off, nbytes = where[(0, "wqkvT32")]
        got = pu.unpack(eng._wbuf.cpu().numpy()[off:off + nbytes].view(np.int16), 3 * heads * 64, 96, 1, 1, "bf16")
        w = eng.fp.view("spatial.0.wqkv").detach().cpu()
        assert torch.equal(got[:2 * heads * 64], (w[:2 * heads * 64] * 0.125).bfloat16().float()) and torch.equal(got[2 * heads * 64:], w[2 * heads * 64:].bfloat16().float())
    # the copies follow the parameters: seeded noise on the masters in place, prep again
    before = eng._wbuf.clone()
    g = torch.Generator().manual_seed(31)
    with torch.no_grad():
        eng.fp.flat.add_((0.02 * torch.randn(eng.fp.flat.numel(), generator=g)).cuda())
    eng.prep_weights()
    _assert_copies(eng)
    assert not torch.equal(before, eng._wbuf) and int(eng._prep_flag.item()) == 0


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_engine_raises_on_a_flagged_table(prec):
    """the flag's only consumer: a table in which one job's pack is 7 makes the first prep_weights() raise, naming the flags; the
    job is skipped (its copy keeps the 0xFF put there), every other copy is right"""
    from maskedsst_amd import _lib
    model, _, _ = build_product(dict(bands=20, depth=1, B=2, heads=2), precision=prec, device="cuda")
    eng = model.engine()
    eng.ensure()
    copies = _copies(eng)
    victim = 5
    nb = ctypes.sizeof(_lib.MsstPrepJob)
    table = eng._jobs.clone()
    row = table[victim * nb:(victim + 1) * nb].cpu().numpy().copy()
    view = _lib.MsstPrepJob.from_buffer(bytearray(row.tobytes()))
    i, field = copies[victim][0], copies[victim][1]
    assert view.dst == int(getattr(eng._bw[i], field)), "the table lists the copies in the order of _copies()"
    view.pack = 7
    table[victim * nb:(victim + 1) * nb] = torch.frombuffer(bytearray(bytes(view)), dtype=torch.uint8).cuda()
    eng._jobs = table
    eng._wbuf.fill_(0xFF)
    with pytest.raises(_lib.MsstError, match=r"malformed jobs \(flags 1\)"):
        eng.prep_weights()
    where = _assert_copies(eng, skip={(i, field)})
    off, nbytes = where[(i, field)]
    assert bool((eng._wbuf[off:off + nbytes] == 0xFF).all())
