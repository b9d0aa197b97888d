"""GPU: SLIC superpixels and object-based class maps -- msst_slic_assign, msst_slic_update, msst_slic_pool, msst_slic_pool_finish and
msst_slic_broadcast (maskedsst_amd/csrc/msst_slic.hip) and maskedsst_amd/superpixel.py against the float64 restatement of
tests/slic_util.py: assignment, update and pooling exact on whole-number inputs (no tolerance: every border, every step, every cause
of a dead pixel, ties, empty centres), every iteration of real-valued fits teacher-forced against float64, the structure of the fit
to the bit, the route through the model and the scripts.  The bars are 4 x the errors measured on the MI355X
(profiles/slic_parity_measured.jsonl); tests/test_slic_host.py checks on the CPU that they still tell the mutated
restatements apart.  Every output is prefilled with a sentinel, so that nothing may be left unwritten.

Measured on the MI355X (profiles/slic_parity_measured.jsonl), the largest absolute error over 8 teacher-forced iterations, cases
19 x 27 at S = 4 / 33 x 41 at S = 8 / 35 x 50 at S = 16: winning score 2.0e-7 / 2.1e-7 / 2.2e-7, centroid 3.4e-8 / 5.1e-8 / 2.9e-8,
offset 1.1e-7 / 2.4e-7 / 4.7e-7, bias 8.4e-8 / 1.1e-7 / 7.0e-8.  The bars are 4 x those numbers; the gap under which a pixel's label
is not compared is the score bar."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import slic_util as su
from test_gpu_pca import child, dev, make_model, same_bits

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def dev_centres(cen):
    from maskedsst_amd import SlicCentres
    return SlicCentres(dev(cen["cent"].astype(np.float32)), dev(cen["off"].astype(np.float32)), dev(cen["bias"].astype(np.float32)),
                       dev(cen["counts"].astype(np.int32)))


def host_centres(c):
    return dict(cent=c.centroids.cpu().numpy().astype(np.float64), off=c.offsets.cpu().numpy().astype(np.float64),
                bias=c.bias.cpu().numpy().astype(np.float64), counts=c.counts.cpu().numpy().astype(np.int64))


def raw_assign(feat, cover, S, cen, hl, prev=None, slab=True):
    """msst_slic_assign with every output prefilled: (labels int64 on the CPU, moved or None, best on the CPU, slab on the device)"""
    from maskedsst_amd import _lib
    from maskedsst_amd.features import _p, _stream
    f = feat if torch.is_tensor(feat) else dev(feat)
    c = None if cover is None else (cover if torch.is_tensor(cover) else dev(cover))
    Bs, _, Hs, Ws = f.shape
    lib = _lib.load()
    labels = torch.full((Bs, Hs, Ws), -77, dtype=torch.int64, device="cuda")
    best = torch.full((Bs, Hs, Ws), SENTINEL, device="cuda")
    pv = None if prev is None else (prev if torch.is_tensor(prev) else dev(prev))
    moved = torch.zeros(1, dtype=torch.int32, device="cuda") if prev is not None else None
    n = lib.msst_slic_scratch_floats(Bs, Hs, Ws, S, 98)
    sl = torch.full((n,), SENTINEL, device="cuda") if slab else None
    cc = cen if cen is not None else (None,) * 4
    _lib.check(lib.msst_slic_assign(_p(f), _p(c), Bs, 96, Hs, Ws, S, float(hl), _p(cc[0]), _p(cc[1]), _p(cc[2]), _p(cc[3]), _p(labels), _p(pv),
                                    _p(moved), _p(best), _p(sl), n if slab else 0, _stream()), "msst_slic_assign")
    labels, best = labels.cpu(), best.cpu()
    assert not bool((labels == -77).any()) and not bool((best == SENTINEL).any())
    if slab:
        assert not bool((sl == SENTINEL).any())
    return labels, None if moved is None else int(moved.cpu()[0]), best, sl


def raw_pool(maps, labels, S):
    """the three pooling launches with every output prefilled: (table, region classes, classes) on the CPU"""
    from maskedsst_amd import _lib
    from maskedsst_amd.features import _p, _stream
    m, lab = dev(maps), dev(labels)
    Bs, C, Hs, Ws = m.shape
    gy, gx = su.grid(Hs, Ws, S)
    lib = _lib.load()
    n = lib.msst_slic_scratch_floats(Bs, Hs, Ws, S, C)
    slab = torch.full((n,), SENTINEL, device="cuda")
    table = torch.full((Bs, gy * gx, C), SENTINEL, device="cuda")
    region = torch.full((Bs, gy * gx), -77, dtype=torch.int64, device="cuda")
    classes = torch.full((Bs, Hs, Ws), -77, dtype=torch.int64, device="cuda")
    _lib.check(lib.msst_slic_pool(_p(m), _p(lab), Bs, C, Hs, Ws, S, _p(slab), n, _stream()), "msst_slic_pool")
    assert not bool((slab == SENTINEL).any())
    _lib.check(lib.msst_slic_pool_finish(_p(slab), n, Bs, C, Hs, Ws, S, _p(table), _p(region), _stream()), "msst_slic_pool_finish")
    _lib.check(lib.msst_slic_broadcast(_p(lab), _p(region), Bs, Hs, Ws, S, _p(classes), _stream()), "msst_slic_broadcast")
    table, region, classes = table.cpu(), region.cpu(), classes.cpu()
    assert not bool((table == SENTINEL).any()) and not bool((region == -77).any()) and not bool((classes == -77).any())
    return table, region, classes


def equal_with_nan(got, want32):
    return torch.equal(torch.isnan(got), torch.isnan(want32)) and torch.equal(torch.nan_to_num(got, nan=0.0), torch.nan_to_num(want32, nan=0.0))


# -------------------------------------------------------------------------------------------------- 1. exact, no tolerance
@pytest.mark.parametrize("S", su.INT_STEPS)
@pytest.mark.parametrize("shape", su.INT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_assign_and_update_are_exact_on_whole_numbers(shape, S):
    from maskedsst_amd import superpixel_update
    Hs, Ws = shape
    for kind in su.DEAD_KINDS:
        feat, cover, dead, cen, hl, prev = su.int_case(shape, S, kind)
        want, want_best, _ = su.assign(feat, cover, cen, S, hl)
        assert np.array_equal(want == -1, dead)
        dc = dev_centres(cen)
        labels, moved, best, slab = raw_assign(feat, cover, S, dc, hl, prev)
        assert torch.equal(labels, t64(want)), (kind, (labels != t64(want)).nonzero()[:5])
        assert moved == int((want != prev).sum()), kind
        assert equal_with_nan(best, t64(want_best.astype(np.float32))), kind
        if kind == "none":                                           # without a cover map: the same
            l2, _, b2, _ = raw_assign(feat, None, S, dc, hl, slab=False)
            assert torch.equal(l2, labels) and equal_with_nan(b2, best)
        # ---- the update from the kernel's own partial sums
        ref = su.update(feat, cover, want, S, cen)
        empty = superpixel_update(slab, (su.INT_BS, Hs, Ws), S, dc)
        got = host_centres(dc)
        assert int(empty.cpu()[0]) == int((ref["counts"] == 0).sum()), kind
        assert np.array_equal(got["counts"], ref["counts"]), kind
        assert np.array_equal(got["cent"], ref["cent"].astype(np.float32).astype(np.float64)), kind     # the float64 quotient rounded once
        assert np.array_equal(got["off"], ref["off"].astype(np.float32).astype(np.float64)), kind
        whole = (ref["cent"] == np.round(ref["cent"])).all(axis=2)
        assert whole.any() and np.array_equal(got["bias"][whole], ref["bias"][whole]), kind
        if kind in ("cell", "all"):                                  # an empty centre keeps what it had
            gone = ref["counts"] == 0
            assert gone.any() and np.array_equal(got["cent"][gone], cen["cent"][gone]) and np.array_equal(got["bias"][gone], cen["bias"][gone])
        # ---- the home mode
        home, _, hb, hslab = raw_assign(feat, cover, S, None, 0.0)
        assert torch.equal(home, t64(su.home_labels(~dead, S))) and bool(torch.isnan(hb).all())
        hc = dev_centres(su.new_centres(su.INT_BS, cen["counts"].shape[1]))
        superpixel_update(hslab, (su.INT_BS, Hs, Ws), S, hc)
        href = su.update(feat, cover, su.home_labels(~dead, S), S, su.new_centres(su.INT_BS, cen["counts"].shape[1]))
        hgot = host_centres(hc)
        assert np.array_equal(hgot["counts"], href["counts"]) and np.array_equal(hgot["cent"], href["cent"].astype(np.float32).astype(np.float64))
        assert np.array_equal(hgot["off"], href["off"].astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("C", su.POOL_CHANNELS)
def test_pooling_is_exact_on_whole_numbers(C):
    for shape, S in (((17, 33), 4), ((9, 17), 8), ((17, 33), 16), ((1, 1), 4), ((7, 9), 16)):
        feat, cover, dead, cen, hl, _ = su.int_case(shape, S, "cell" if shape[0] > 7 else "corner")
        labels, _, _ = su.assign(feat, cover, cen, S, hl)
        n_sp = cen["counts"].shape[1]
        maps = su.int_maps(shape, C)
        want_t, want_r, want_c = su.pool(maps, labels, n_sp)
        table, region, classes = raw_pool(maps, labels, S)
        assert equal_with_nan(table, t64(want_t.astype(np.float32))), (shape, S)
        assert torch.equal(region, t64(want_r)) and torch.equal(classes, t64(want_c)), (shape, S)
        if shape[0] > 7:
            assert np.isnan(want_t).all(axis=2).any() and (want_r == -1).any()      # an empty superpixel
        if C > 1 and shape[1] > 1:
            assert np.isneginf(want_t[:, :, C - 1]).any() and not (want_r == C - 1)[np.isneginf(want_t[:, :, C - 1])].any()
        if C > 1 and shape[0] > 7:
            srt = np.sort(np.nan_to_num(want_t, nan=-np.inf), axis=2)
            assert (srt[:, :, -1] == srt[:, :, -2]).any()                               # ties among the region scores


# ------------------------------------------------------------------------------------- 2. real-valued, one step at a time
@pytest.mark.parametrize("case", su.REAL_CASES, ids=su.case_name)
def test_every_iteration_teacher_forced_against_float64(case):
    """every iteration of a fit by the low-level launches; the float64 restatement assigns from the device's own centres of the
    iteration before and updates from the device's own labels"""
    from maskedsst_amd import fit_superpixels, superpixel_update
    from maskedsst_amd.superpixel import new_centres, slic_hl
    Hs, Ws, S = case
    feat, cover = su.real_case(case)
    fd, cd = dev(feat), dev(cover)
    gy, gx = su.grid(Hs, Ws, S)
    hl = slic_hl(su.REAL_COMPACTNESS, S)
    assert hl == su.hl_of(su.REAL_COMPACTNESS, S)
    live = su.live_map(feat, cover)
    cen = new_centres(su.REAL_BS, gy * gx, "cuda")
    labels, _, _, slab = raw_assign(fd, cd, S, None, 0.0)
    assert np.array_equal(labels.numpy(), su.home_labels(live, S))
    superpixel_update(slab, (su.REAL_BS, Hs, Ws), S, cen)
    err = dict(score=0.0, centroid=0.0, offset=0.0, bias=0.0)
    prev64 = su.new_centres(su.REAL_BS, gy * gx)
    history, steps = [], []

    def compare_centres(lab, before):
        got = host_centres(cen)
        want = su.update(feat, cover, lab, S, before)
        assert np.array_equal(got["counts"], want["counts"])
        err["centroid"] = max(err["centroid"], su.abs_err(got["cent"], want["cent"]))
        err["offset"] = max(err["offset"], su.abs_err(got["off"], want["off"]))
        err["bias"] = max(err["bias"], su.abs_err(got["bias"], want["bias"]))
        return got

    held = compare_centres(labels.numpy(), prev64)
    for t in range(su.REAL_ITERS):
        new, moved, best, slab = raw_assign(fd, cd, S, cen, hl, dev(labels.numpy()))
        want, want_best, margin = su.assign(feat, cover, held, S, hl)
        assert np.array_equal(new.numpy() == -1, ~live)
        err["score"] = max(err["score"], su.abs_err(best.numpy(), want_best))
        steps.append((new.numpy(), want, margin))
        empty = superpixel_update(slab, (su.REAL_BS, Hs, Ws), S, cen)
        assert moved == int((new != labels).sum())
        history.append((moved, int(empty.cpu()[0])))
        held = compare_centres(new.numpy(), held)
        assert history[-1][1] == int((held["counts"] == 0).sum())
        labels = new
    bar = su.check(su.case_name(case), err)
    if bar is not None:
        for got, want, margin in steps:
            sure = live & (margin >= bar["score"])
            assert np.array_equal(got[sure], want[sure]), int((got[sure] != want[sure]).sum())
            assert (live & ~sure).sum() <= su.MARGIN_SHARE * live.sum()
    assert sum(m for m, _ in history) > 0
    # ---- the fit is these launches: the same bits
    sp = fit_superpixels(fd, cd, step=S, compactness=su.REAL_COMPACTNESS, iters=su.REAL_ITERS)
    assert sp.history.dtype == torch.int64 and not sp.history.is_cuda and sp.history.tolist() == [list(h) for h in history]
    assert torch.equal(sp.labels.cpu(), labels) and same_bits(sp.centroids, cen.centroids) and torch.equal(sp.counts, cen.counts)
    assert sp.step == S and sp.grid == (gy, gx) and sp.labels.dtype == torch.int64 and sp.counts.dtype == torch.int32
    assert np.abs(sp.positions.cpu().numpy() - su.positions(held, Hs, Ws, S)).max() < 1e-5


# ----------------------------------------------------------------------------------------------------- 3. structure, to the bit
def test_structure_to_the_bit():
    from maskedsst_amd import fit_superpixels, superpixel_classify, superpixel_pool
    case = su.REAL_CASES[0]
    Hs, Ws, S = case
    feat, cover = su.real_case(case)
    feat = np.concatenate([feat, su.real_case(case, seed=9)[0][:1]])
    cover = np.concatenate([cover, cover[:1]])
    fd, cd = dev(feat), dev(cover)
    maps = dev(np.random.default_rng(3).normal(size=(3, 17, Hs, Ws)).astype(np.float32))
    all3 = fit_superpixels(fd, cd, step=S, iters=4)
    pool3 = superpixel_pool(all3, maps)
    # a scene alone and inside a batch of three
    for b in range(3):
        one = fit_superpixels(fd[b:b + 1].contiguous(), cd[b:b + 1].contiguous(), step=S, iters=4)
        assert torch.equal(one.labels, all3.labels[b:b + 1]) and same_bits(one.centroids, all3.centroids[b:b + 1].contiguous())
        assert torch.equal(one.counts, all3.counts[b:b + 1]) and same_bits(one.positions, all3.positions[b:b + 1].contiguous())
        assert same_bits(superpixel_pool(one, maps[b:b + 1].contiguous()), pool3[b:b + 1].contiguous())
    # two calls: the same bits
    again = fit_superpixels(fd, cd, step=S, iters=4)
    assert torch.equal(again.labels, all3.labels) and same_bits(again.centroids, all3.centroids) and torch.equal(again.history, all3.history)
    res, res2 = superpixel_classify(all3, maps), superpixel_classify(again, maps)
    assert same_bits(res.region_scores, pool3) and same_bits(res2.region_scores, pool3) and torch.equal(res.classes, res2.classes)
    assert torch.equal(res.classes == -1, all3.labels == -1) and torch.equal(res.region_classes == -1, all3.counts == 0)
    # after an iteration with moved == 0 one more changes no output
    hist = fit_superpixels(fd, cd, step=S, iters=12).history
    still = [t for t in range(12) if hist[t, 0] == 0]
    assert still and still[0] < 11, hist.tolist()
    a, b = fit_superpixels(fd, cd, step=S, iters=still[0] + 1), fit_superpixels(fd, cd, step=S, iters=still[0] + 2)
    assert b.history[-1].tolist() == a.history[-1].tolist() and torch.equal(a.labels, b.labels) and same_bits(a.centroids, b.centroids)
    assert same_bits(a.positions, b.positions) and torch.equal(a.counts, b.counts)
    # iters = 0: the home labels and the cell means
    home = fit_superpixels(fd, cd, step=S, iters=0)
    live = su.live_map(feat, cover)
    assert home.history.shape == (0, 2) and np.array_equal(home.labels.cpu().numpy(), su.home_labels(live, S))
    ref = su.update(feat, cover, su.home_labels(live, S), S, su.new_centres(3, home.counts.shape[1]))
    assert np.array_equal(home.counts.cpu().numpy(), ref["counts"]) and np.abs(home.centroids.cpu().numpy() - ref["cent"]).max() < 1e-6
    # cover all zero: labels all -1, counts all 0
    none = fit_superpixels(fd, torch.zeros_like(cd), step=S, iters=2)
    assert bool((none.labels == -1).all()) and bool((none.counts == 0).all()) and none.history.tolist() == [[0, int(none.counts.numel())]] * 2
    dead = superpixel_classify(none, maps)
    assert bool((dead.classes == -1).all()) and bool(torch.isnan(dead.region_scores).all()) and bool((dead.region_classes == -1).all())
    # where in a scene a cell lies does not matter: the scene as the right end of a wide one whose rest is dead
    wide = torch.zeros(1, 96, Hs, 4096 + Ws, device="cuda")
    wide[:, :, :, 4096:] = fd[:1]
    wcov = torch.zeros(1, Hs, 4096 + Ws, dtype=torch.int32, device="cuda")
    wcov[:, :, 4096:] = cd[:1]
    far = fit_superpixels(wide, wcov, step=S, iters=4)
    gy, gx = all3.grid
    near_lab = all3.labels[0]
    shift = torch.where(near_lab >= 0, (near_lab // gx) * far.grid[1] + near_lab % gx + 4096 // S, near_lab)
    assert torch.equal(far.labels[0, :, 4096:], shift)
    assert same_bits(far.centroids.view(gy, far.grid[1], 96)[:, 4096 // S:].contiguous(), all3.centroids[0].view(gy, gx, 96))
    assert torch.equal(far.history, fit_superpixels(fd[:1].contiguous(), cd[:1].contiguous(), step=S, iters=4).history + torch.tensor([0, gy * 4096 // S]))


# ------------------------------------------------------------------------------------------------------- 4. through the model
@pytest.mark.parametrize("stride", [8, 5])
def test_superpixel_scene_through_the_model(stride):
    from maskedsst_amd import KnnBank, SuperpixelScene, fit_gaussian, fit_superpixels, knn_classify, superpixel_classify, superpixel_scene
    model = make_model()
    model.train()
    g = torch.Generator().manual_seed(3)
    scene = torch.randn(2, 50, 16, 16, generator=g).cuda()
    _, logits = model.predict_scene(scene, stride=stride, return_logits=True)
    emb = model.encode_scene(scene, stride=stride, normalize=True)
    covered = emb.cover > 0
    assert bool(covered.all()) == (stride == 8)
    sp = fit_superpixels(emb, step=4, iters=3)
    want = superpixel_classify(sp, logits)
    res = model.superpixel_scene(scene, logits, stride=stride, step=4, iters=3)
    assert isinstance(res, SuperpixelScene) and model.training and torch.equal(res.cover, emb.cover)
    assert torch.equal(res.superpixels.labels, sp.labels) and same_bits(res.superpixels.centroids, sp.centroids)
    assert torch.equal(res.superpixels.history, sp.history) and res.superpixels.grid == (4, 4)
    assert torch.equal(res.classes, want.classes) and same_bits(res.region_scores, want.region_scores)
    assert torch.equal(res.classes == -1, ~covered) and torch.equal(sp.labels == -1, ~covered)
    other = superpixel_scene(model, scene, logits, embedding=emb, step=4, iters=3)       # the embedding handed over: no second pass
    assert torch.equal(other.classes, res.classes) and same_bits(other.region_scores, res.region_scores)
    bare = model.superpixel_scene(scene, embedding=emb, step=4, iters=3)
    assert bare.classes is None and bare.region_scores is None and torch.equal(bare.superpixels.labels, sp.labels)
    # a superpixel's mean feature is a row for the row classifiers
    rows = sp.centroids.reshape(-1, 96)
    lab = (torch.arange(rows.shape[0], device="cuda") % 3).long()
    bank = KnnBank(rows, lab, 3)
    out = knn_classify(bank, rows, k=1)
    assert out.classes.shape == (rows.shape[0],) and bool(((out.classes >= 0) & (out.classes < 3)).all())
    raw = model.encode_scene(scene, stride=stride, normalize=False)
    pixels = raw.features.permute(0, 2, 3, 1)[covered].contiguous()
    clf = fit_gaussian(KnnBank(pixels, (torch.arange(pixels.shape[0], device="cuda") % 3).long(), 3), covariance="tied")
    got = clf.classify(fit_superpixels(raw, step=4, iters=3).centroids.reshape(-1, 96))
    assert got.classes.shape == (rows.shape[0],) and bool(((got.classes >= -1) & (got.classes < 3)).all())


# --------------------------------------------------------------------------------------------------------------------- 5. scripts
def test_finetune_val_superpixel_script():
    """finetune.py --val-superpixel: one more line per validation pass"""
    out = child([sys.executable, "finetune.py", "--steps", "1", "--val-scenes", "4", "--val-every", "1", "--val-superpixel", "8"], 600)
    lines = [l.split() for l in out.splitlines() if l.startswith("val-superpixel step ")]
    assert [e[2] for e in lines] == ["1"], out
    e = lines[0]
    assert e[3:5] == ["sp_step", "8"] and e[5] == "superpixels" and int(e[6]) > 0 and e[7] == "acc_before" and 0.0 <= float(e[8]) <= 1.0, e
    assert e[9] == "acc_after" and 0.0 <= float(e[10]) <= 1.0 and e[11] == "changed" and int(e[12]) >= 0, e
    assert e[13] == "pixels" and int(e[14]) > 0 and e[15:] == ["scenes", "4"], e


def test_slic_time_script():
    """tools/slic_time.py --quick: exit 0 and ONE JSON line, nothing appended"""
    out = child([sys.executable, os.path.join("tools", "slic_time.py"), "--quick"], 300)
    lines = [l for l in out.splitlines() if l.strip()]
    assert len(lines) == 1, out
    row = json.loads(lines[0])
    assert row["tool"] == "slic_time" and row["shape"] == "4x64x64" and row["step"] == 8 and row["channels"] == 16
    assert row["fit_us"] > 0 and row["eager_fit_us"] > 0 and row["pool_us"] > 0 and row["eager_pool_us"] > 0
    assert row["labels_agree"] > 0.99 and row["pool_max_diff"] < 1e-4
