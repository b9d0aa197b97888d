"""GPU: connected regions of class maps -- msst_regions_label and msst_regions_merge (maskedsst_amd/csrc/msst_regions.hip) and
maskedsst_amd/regions.py against the numpy restatement of tests/region_util.py (flood fill; one merge round written per region).
Everything is integer: every comparison is exact, there is no tolerance.  Every output is prefilled with a sentinel, so that nothing
may be left unwritten, and the error word is read in every case: it is 0.  tests/test_regions_host.py checks the restatement itself on
the CPU (against scipy, a pairwise loop, known answers and its mutants).

The kernel's tile is 16 x 16 pixels: the shapes lie one below, at and one past it in each axis, past two tiles (33 x 65), in one long
row (1 x 4100) and at 130 x 150; the patterns of a shape run as the scenes of ONE batch, so that every call also has more than one
scene."""
import functools

import numpy as np
import pytest
import torch

import region_util as ru
import slic_util as su
from test_gpu_pca import dev, same_bits

pytestmark = pytest.mark.gpu

SMALL_SHAPES = [(1, 1), (1, 70), (70, 1), (7, 9), (15, 17), (16, 16), (17, 15), (16, 33), (33, 65)]
LARGE = {(1, 4100): ("random3", "one", "checker", "dead_row", "corners"), (130, 150): ("spiral", "serpentine", "random3", "rings")}


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@functools.lru_cache(maxsize=None)
def batch(shape, names=ru.PATTERNS):
    return np.stack([ru.pattern(n, *shape) for n in names])


@functools.lru_cache(maxsize=None)
def want_label(shape, names, conn):
    return ru.label(batch(shape, names), conn)


def raw_label(values, conn):
    """msst_regions_label with every output prefilled: (labels, sizes, count, error word) on the CPU"""
    from maskedsst_amd import _lib
    from maskedsst_amd.features import _p, _stream
    v = values if torch.is_tensor(values) else dev(values)
    Bs, Hs, Ws = v.shape
    lib = _lib.load()
    labels = torch.full((Bs, Hs, Ws), -77, dtype=torch.int64, device="cuda")
    sizes = torch.full((Bs, Hs, Ws), -77, dtype=torch.int32, device="cuda")
    count = torch.full((Bs,), -77, dtype=torch.int32, device="cuda")
    n = lib.msst_regions_scratch_bytes(Bs, Hs, Ws)
    assert n == 16 + 32 * Bs * Hs * Ws
    scratch = torch.full((n // 4,), -77, dtype=torch.int32, device="cuda")
    scratch[:4] = 0
    _lib.check(lib.msst_regions_label(_p(v), Bs, Hs, Ws, conn, _p(labels), _p(sizes), _p(count), _p(scratch), n, _stream()), "msst_regions_label")
    labels, sizes, count = labels.cpu(), sizes.cpu(), count.cpu()
    assert not bool((labels == -77).any()) and not bool((sizes == -77).any()) and not bool((count == -77).any())
    return labels, sizes, count, int(scratch[0].cpu())


def raw_merge(values, conn, mode, min_size, step):
    """label and one msst_regions_merge with every output prefilled: (values_out, history [4], error word) on the CPU"""
    from maskedsst_amd import _lib
    from maskedsst_amd.features import _p, _stream
    from maskedsst_amd.regions import _label, _scratch
    v = dev(values)
    Bs, Hs, Ws = v.shape
    lib = _lib.load()
    scratch = _scratch(v.shape, v.device)
    reg = _label(v, conn, scratch)
    out = torch.full((Bs, Hs, Ws), -77, dtype=torch.int64, device="cuda")
    hist = torch.zeros(4, dtype=torch.int32, device="cuda")
    _lib.check(lib.msst_regions_merge(_p(v), _p(reg.labels), _p(reg.sizes), Bs, Hs, Ws, conn, mode, min_size, step, _p(out), _p(hist), _p(scratch),
                                      4 * scratch.numel(), _stream()), "msst_regions_merge")
    out = out.cpu()
    assert not bool((out == -77).any()) or bool((t64(values) == -77).any())
    return out, hist.cpu().long(), int(scratch[0].cpu())


def check_label(values, want, conn, what):
    labels, sizes, count, err = raw_label(values, conn)
    assert err == 0, what
    assert torch.equal(labels, t64(want[0])), (what, (labels != t64(want[0])).nonzero()[:5].tolist())
    assert torch.equal(sizes, t64(want[1])), (what, (sizes != t64(want[1])).nonzero()[:5].tolist())
    assert torch.equal(count, t64(want[2])), (what, count.tolist(), want[2].tolist())
    return labels, sizes, count


# ---------------------------------------------------------------------------------------------------------------- 1. labelling
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_labelling_equals_the_flood_fill(shape, conn):
    check_label(batch(shape), want_label(shape, ru.PATTERNS, conn), conn, (shape, conn))


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("shape", sorted(LARGE), ids=lambda s: f"{s[0]}x{s[1]}")
def test_labelling_of_long_chains(shape, conn):
    """a long row, and a spiral and a serpentine that cross every tile border many times: the long-chain case of the union-find"""
    names = LARGE[shape]
    labels, sizes, count = check_label(batch(shape, names), want_label(shape, names, conn), conn, (shape, conn))
    if shape == (130, 150):
        assert int(sizes[0].max()) > 130 * 150 // 3 and int(sizes[1].max()) > 130 * 150 // 2      # the spiral, the serpentine: one region


def test_labelling_structure_to_the_bit():
    from maskedsst_amd import Regions, check_regions, label_regions, region_ids
    shape = (33, 65)
    v = dev(batch(shape))
    for conn in (4, 8):
        want = want_label(shape, ru.PATTERNS, conn)
        reg = label_regions(v, connectivity=conn)
        assert isinstance(reg, Regions) and reg.connectivity == conn and check_regions(reg) is reg and int(reg.error.cpu()[0]) == 0
        assert reg.labels.dtype == torch.int64 and reg.sizes.dtype == torch.int32 and reg.count.dtype == torch.int32
        assert torch.equal(reg.labels.cpu(), t64(want[0])) and torch.equal(reg.sizes.cpu(), t64(want[1])) and torch.equal(reg.count.cpu(), t64(want[2]))
        # two calls in a row: the same bits
        again = label_regions(v, connectivity=conn)
        assert torch.equal(again.labels, reg.labels) and torch.equal(again.sizes, reg.sizes) and torch.equal(again.count, reg.count)
        # a scene alone against the same scene inside the batch
        for b in (0, 5, 7, len(ru.PATTERNS) - 1):
            one = label_regions(v[b:b + 1].contiguous(), connectivity=conn)
            assert torch.equal(one.labels, reg.labels[b:b + 1]) and torch.equal(one.sizes, reg.sizes[b:b + 1]) and torch.equal(one.count, reg.count[b:b + 1])
        # dense ids by ascending root
        ids, n = region_ids(reg)
        wids, wn = ru.ids_of(want[0])
        assert ids.dtype == torch.int64 and torch.equal(ids.cpu(), t64(wids)) and torch.equal(n.cpu(), t64(wn))


def test_nothing_passes_between_scenes():
    """two batches that are equal, except that in the second a region touches the border where the next scene continues it"""
    a = np.zeros((3, 9, 20), dtype=np.int64)
    a[:, 3:6, 5:9] = 1
    b = a.copy()
    b[0, 6:, 5:9] = 1          # reaches the bottom border of scene 0 ...
    b[1, :3, 5:9] = 1          # ... and scene 1 goes on from its top border
    b[1, 4, 9:] = 1            # reaches the right border of a row; the next row starts with the same value
    b[1, 5, 0] = 1
    for conn in (4, 8):
        wa, wb = ru.label(a, conn), ru.label(b, conn)
        check_label(a, wa, conn, "apart")
        labels, sizes, count = check_label(b, wb, conn, "touching")
        assert wb[2][0] == 2 and wb[2][1] > wa[2][1] and torch.equal(labels[2], t64(wa[0][2]))


# ------------------------------------------------------------------------------------------------------------------ 2. the sieve
@pytest.mark.parametrize("conn", [4, 8])
def test_one_merge_round_equals_the_restatement(conn):
    for name, v, m in ru.sieve_maps():
        want, whist = ru.merge_round(v[None], conn, 0, m)
        out, hist, err = raw_merge(v[None], conn, 0, m, 0)
        assert err == 0 and torch.equal(out, t64(want)) and hist.tolist() == whist.tolist(), (name, hist.tolist(), whist.tolist())
    for name, v in ru.fragment_maps():
        want, whist = ru.merge_round(v[None], conn, 1, 1, 4)
        out, hist, err = raw_merge(v[None], conn, 1, 1, 4)
        assert err == 0 and torch.equal(out, t64(want)) and hist.tolist() == whist.tolist(), (name, hist.tolist(), whist.tolist())
    # every pattern of the labelling tests as a class map, across tile borders, three values and dead pixels
    v = batch((33, 65))
    for min_size in (2, 40):
        want, whist = ru.merge_round(v, conn, 0, min_size)
        out, hist, err = raw_merge(v, conn, 0, min_size, 0)
        assert err == 0 and torch.equal(out, t64(want)) and hist.tolist() == whist.tolist(), (min_size, hist.tolist(), whist.tolist())


@pytest.mark.parametrize("conn", [4, 8])
def test_sieve_classes(conn):
    from maskedsst_amd import SieveResult, sieve_classes
    for name, v, m in ru.sieve_maps():
        want, whist = ru.rounds(v[None], conn, 3, 0, m)
        res = sieve_classes(dev(v[None]), m, connectivity=conn, rounds=3)
        assert isinstance(res, SieveResult) and res.history.dtype == torch.int64 and not res.history.is_cuda and res.history.shape == (3, 4)
        assert torch.equal(res.classes.cpu(), t64(want)) and res.history.tolist() == whist.tolist(), (name, res.history.tolist(), whist.tolist())
        wl = ru.label(want, conn)
        assert torch.equal(res.regions.labels.cpu(), t64(wl[0])) and torch.equal(res.regions.sizes.cpu(), t64(wl[1])), name
        assert torch.equal(res.regions.count.cpu(), t64(wl[2])) and int(res.regions.error.cpu()[0]) == 0, name
    # the cases by name: what the sieve is for
    maps = {n: (v, m) for n, v, m in ru.sieve_maps()}
    v, m = maps["isolated"]
    assert bool((sieve_classes(dev(v[None]), m, connectivity=conn).classes == 3).all())
    v, m = maps["tie"]
    assert sieve_classes(dev(v[None]), m, connectivity=conn, rounds=1).classes[0, 4, 8:10].tolist() == [0, 0]        # the lowest root wins
    v, m = maps["waits"]
    one, two = sieve_classes(dev(v[None]), m, connectivity=conn, rounds=1), sieve_classes(dev(v[None]), m, connectivity=conn, rounds=2)
    assert int(one.classes[0, 4, 4]) == 2 and bool((two.classes == 0).all()) and two.history[:, 2].tolist() == [1, 1]
    v, m = maps["enclosed"]
    res = sieve_classes(dev(v[None]), m, connectivity=conn)
    assert torch.equal(res.classes.cpu(), t64(v[None])) and res.history[:, 2:].sum() == 0                                # it stays; -1, -2 kept


def test_sieve_structure_to_the_bit():
    from maskedsst_amd import sieve_classes
    v = np.stack([ru.salt_blobs(40, 50, seed=s) for s in (1, 2, 3)])
    vd = dev(v)
    want, whist = ru.rounds(v, 4, 5, 0, 4)
    res = sieve_classes(vd, 4, rounds=5)
    assert torch.equal(res.classes.cpu(), t64(want)) and res.history.tolist() == whist.tolist()
    assert whist[0, 3] > 0 and torch.equal(res.classes < 0, vd < 0) and torch.equal(res.classes[vd < 0], vd[vd < 0])       # -1 and -2 are kept
    assert int(res.regions.count.sum()) == int(ru.label(want, 4)[2].sum())
    # two calls; a scene alone against the same scene inside the batch
    again = sieve_classes(vd, 4, rounds=5)
    assert torch.equal(again.classes, res.classes) and torch.equal(again.history, res.history) and torch.equal(again.regions.labels, res.regions.labels)
    alone = [sieve_classes(vd[b:b + 1].contiguous(), 4, rounds=5) for b in range(3)]
    for b in range(3):
        assert torch.equal(alone[b].classes, res.classes[b:b + 1]) and torch.equal(alone[b].regions.labels, res.regions.labels[b:b + 1])
        assert torch.equal(alone[b].regions.sizes, res.regions.sizes[b:b + 1])
    assert torch.equal(sum(a.history for a in alone), res.history)
    # after a round with 0 changed pixels every later round reproduces all outputs
    still = [t for t in range(5) if res.history[t, 3] == 0]
    assert still and still[0] < 4, res.history.tolist()
    a, b = sieve_classes(vd, 4, rounds=still[0] + 1), sieve_classes(vd, 4, rounds=still[0] + 2)
    assert torch.equal(a.classes, b.classes) and torch.equal(a.regions.labels, b.regions.labels) and torch.equal(a.regions.sizes, b.regions.sizes)
    assert torch.equal(a.regions.count, b.regions.count) and b.history[-1].tolist() == a.history[-1].tolist()
    # min_size = 1 and rounds = 0: the input, bit for bit, with its regions
    wl = ru.label(v, 8)
    for res in (sieve_classes(vd, 1, connectivity=8), sieve_classes(vd, 9, connectivity=8, rounds=0)):
        assert torch.equal(res.classes, vd) and torch.equal(res.regions.labels.cpu(), t64(wl[0])) and torch.equal(res.regions.count.cpu(), t64(wl[2]))
    assert sieve_classes(vd, 9, rounds=0).history.shape == (0, 4) and sieve_classes(vd, 1).history[:, 1:].sum() == 0


# ---------------------------------------------------------------------------------------------------------------- 3. fragments
def superpixels_of(labels, S):
    from maskedsst_amd import Superpixels
    Bs, Hs, Ws = labels.shape
    gy, gx = ru.grid(Hs, Ws, S)
    return Superpixels(dev(labels), None, None, torch.zeros(Bs, gy * gx, dtype=torch.int32, device="cuda"), torch.zeros(0, 2, dtype=torch.int64),
                       S, (gy, gx))


@pytest.mark.parametrize("conn", [4, 8])
def test_enforce_connectivity_on_hand_built_maps(conn):
    from maskedsst_amd import ConnectedSuperpixels, enforce_connectivity
    names, maps = zip(*ru.fragment_maps())
    v = np.stack(maps)
    want, whist = ru.rounds(v, conn, 3, 1, 1, 4)
    con = enforce_connectivity(superpixels_of(v, 4), connectivity=conn, rounds=3)
    assert isinstance(con, ConnectedSuperpixels) and con.superpixels.centroids is None and con.superpixels.positions is None
    assert con.superpixels.step == 4 and con.superpixels.grid == (4, 4)
    assert torch.equal(con.superpixels.labels.cpu(), t64(want)), [n for n, a, b in zip(names, con.superpixels.labels.cpu(), t64(want)) if not torch.equal(a, b)]
    assert con.history.tolist() == whist.tolist()
    wl = ru.label(want, conn)
    assert torch.equal(con.regions.labels.cpu(), t64(wl[0])) and torch.equal(con.regions.count.cpu(), t64(wl[2]))
    counts = np.stack([np.bincount(w[(w >= 0) & (w < 16)], minlength=16) for w in want])
    assert torch.equal(con.superpixels.counts.cpu(), t64(counts.astype(np.int32)))
    got = dict(zip(names, con.superpixels.labels.cpu()))
    assert got["ineligible_larger"][5, 5] == 5 and got["equal_pieces"][4, 4] == 5 and got["equal_pieces"][7, 7] == 6
    assert got["out_of_range"][9, 9] == 16 and got["out_of_range"][10, 10] == 99 and got["out_of_range"][10, 9] == -1
    # a map in one piece per id is untouched, whatever the rounds
    h = np.stack([ru.home(13, 18, 4)] * 2)
    same = enforce_connectivity(superpixels_of(h, 4), connectivity=conn)
    assert torch.equal(same.superpixels.labels.cpu(), t64(h)) and same.history[:, 1:].sum() == 0


FIT_CASE, FIT_COMPACTNESS, FIT_ITERS = su.REAL_CASES[0], 0.05, 4


def test_enforce_connectivity_after_a_real_fit():
    """fit_superpixels on the planted Voronoi fields of tests/test_gpu_slic.py at a low compactness, so that fragments occur"""
    from maskedsst_amd import enforce_connectivity, fit_superpixels, superpixel_classify, superpixel_pool
    Hs, Ws, S = FIT_CASE
    feat, cover = su.real_case(FIT_CASE)
    # on the CPU, from the restatement alone: the committed case has fragments
    cpu_labels = su.fit(feat, cover, S, FIT_COMPACTNESS, FIT_ITERS)[0]
    assert ru.fragments(cpu_labels, 4, S) >= 1
    fd, cd = dev(feat), dev(cover)
    sp = fit_superpixels(fd, cd, step=S, compactness=FIT_COMPACTNESS, iters=FIT_ITERS)
    before = sp.labels.cpu().numpy()
    assert ru.fragments(before, 4, S) >= 1
    for conn in (4, 8):
        con = enforce_connectivity(sp, fd, connectivity=conn)
        want, whist = ru.rounds(before, conn, 4, 1, 1, S)
        assert con.history.tolist() == whist.tolist() and whist[0, 2] > 0
        new = con.superpixels
        assert torch.equal(new.labels.cpu(), t64(want)) and torch.equal(new.labels == -1, sp.labels == -1)
        # every id whose fragments all had a candidate (in the first round, from the restatement) is one region in the device's result
        gy, gx = ru.grid(Hs, Ws, S)
        roots = new.labels.cpu().numpy().copy()
        roots[con.regions.sizes.cpu().numpy() == 0] = -1            # the id at a root pixel, -1 elsewhere
        checked = 0
        for b in range(su.REAL_BS):
            regs = ru.regions_of(before[b], conn)
            live = ru._flag(regs, 1, 1, gy * gx, None)
            stuck = {g.value for r, g in regs.items() if live[r] and g.flagged and ru._winner(g, regs, live, 1, S, gx, None) is None}
            pieces = np.bincount(roots[b][roots[b] >= 0], minlength=gy * gx)
            for k in range(gy * gx):
                if k not in stuck and pieces[k]:
                    assert pieces[k] == 1, (conn, b, k)
                    checked += 1
        assert checked > 0
        assert int(con.regions.count.sum()) - int((new.counts > 0).sum()) == ru.fragments(want, conn, S)
        # nothing fell outside the 3 x 3 cells: an all-ones map pools to exactly 1 in every non-empty superpixel, the counts sum to the live pixels
        ones = torch.ones(su.REAL_BS, 3, Hs, Ws, device="cuda")
        table = superpixel_pool(new, ones)
        full = new.counts > 0
        assert bool((table[full] == 1.0).all()) and bool(torch.isnan(table[~full]).all())
        assert int(new.counts.sum()) == int((sp.labels >= 0).sum()) and new.counts.dtype == torch.int32
        assert new.centroids.shape == sp.centroids.shape and bool(torch.isfinite(new.centroids[full]).all()) and new.positions is None
        assert same_bits(new.centroids, superpixel_pool(new, fd))     # NaN rows for the empty superpixels: compared as bits
        res = superpixel_classify(new, ones)
        assert torch.equal(res.classes == -1, sp.labels == -1)       # no pixel is dropped


# --------------------------------------------------------------------------------------------------------------------- 4. scripts
def test_finetune_region_flags_script():
    """finetune.py --val-sieve and --val-superpixel-connect: one more line each per validation pass, the existing lines as they were"""
    import sys
    from test_gpu_pca import child
    out = child([sys.executable, "finetune.py", "--steps", "1", "--val-scenes", "4", "--val-every", "1", "--val-sieve", "6",
                 "--val-sieve-connectivity", "8", "--val-superpixel", "8", "--val-superpixel-connect"], 600)
    lines = [l.split() for l in out.splitlines()]
    sieve = [e for e in lines if e[:2] == ["val-sieve", "step"]]
    assert [e[2] for e in sieve] == ["1"], out
    e = sieve[0]
    assert e[3:5] == ["min_size", "6"] and e[5] == "regions_before" and e[7] == "regions_after" and 0 < int(e[8]) <= int(e[6]), e
    assert e[9] == "acc_before" and 0.0 <= float(e[10]) <= 1.0 and e[11] == "acc_after" and 0.0 <= float(e[12]) <= 1.0, e
    assert e[13] == "changed" and int(e[14]) >= 0 and e[15] == "pixels" and int(e[16]) > 0 and e[17:] == ["scenes", "4"], e
    names = [e[0] for e in lines if e and e[0].startswith("val-superpixel")]
    assert names == ["val-superpixel", "val-superpixel-connected"], out               # the new line follows the existing one
    e = next(e for e in lines if e[:1] == ["val-superpixel-connected"])
    assert e[1:3] == ["step", "1"] and e[3] == "fragments_before" and e[5] == "fragments_after" and 0 <= int(e[6]) <= int(e[4]), e
    assert e[7] == "acc_after" and 0.0 <= float(e[8]) <= 1.0 and e[9] == "pixels" and e[11:] == ["scenes", "4"], e


def test_regions_time_script():
    """tools/regions_time.py --quick: exit 0 and one JSON line per map, nothing appended; the three routes agree"""
    import json
    import os
    import sys
    from test_gpu_pca import child
    out = child([sys.executable, os.path.join("tools", "regions_time.py"), "--quick"], 300)
    rows = [json.loads(l) for l in out.splitlines() if l.strip()]
    assert [(r["tool"], r["shape"], r["map"]) for r in rows] == [("regions_time", "4x64x64", "blobs"), ("regions_time", "4x64x64", "superpixels")], out
    for r in rows:
        assert r["error_word"] == 0 and r["scipy_agrees"] and r["torch_agrees"] and r["regions"] > 0, r
        assert r["label_us"] > 0 and r["scipy_label_us"] > 0 and r["torch_label_us"] > 0, r
    assert rows[0]["sieve_us"] > 0 and rows[0]["regions_after"] < rows[0]["regions"] and rows[1]["connect_us"] > 0
