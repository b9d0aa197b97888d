"""GPU: Gaussian (QDA / LDA) classification of frozen features -- msst_gauss_score (maskedsst_amd/csrc/msst_gauss.hip) and
maskedsst_amd/gaussian.py against the restatement of tests/gauss_util.py: exact on whole-number tables (no tolerance: classes,
distances and scores to the bit, every class count and table form, both layouts, NaN rows, ties, a class that cannot win, rejection at
the distance itself), real-valued scores against float64, the fit against float64, equal bits from equal inputs, the route through the
model and the two scripts.  The bars are 4 x the errors measured on the MI355X (profiles/gauss_parity_measured.jsonl);
tests/test_gauss_host.py checks on the CPU that they still tell the mutated restatements apart."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

import gauss_util as gu
import pca_util as pu
from test_gpu_pca import child, dev, make_model, same_bits

pytestmark = pytest.mark.gpu

SENTINEL = -77


def raw_score(features, tab, max_d2=float("inf"), scores=True, out_layout=0):
    """msst_gauss_score with every output prefilled (classes with a sentinel, the floats with -12345.5, a value no result of these fixed
    cases has): (classes int32, distance, scores or None) on the CPU; nothing may be left unwritten"""
    from maskedsst_amd import _lib
    from maskedsst_amd.features import _p, _stream
    from maskedsst_amd.pca import _source
    x, layout, rows, plane = _source(features)
    nc, T = len(tab["consts"]), len(tab["centres"])
    d = {k: dev(tab[k]) for k in ("centres", "tables", "offsets", "consts")}
    ids = (ctypes.c_int32 * nc)(*[int(v) for v in tab["class_table"]])
    classes = torch.full((rows,), SENTINEL, dtype=torch.int32, device="cuda")
    distance = torch.full((rows,), -12345.5, device="cuda")
    s = None
    if scores:
        s = torch.full((x.shape[0], nc) + tuple(x.shape[2:]) if out_layout == 1 else (rows, nc), -12345.5, device="cuda")
    lib = _lib.load()
    _lib.check(lib.msst_gauss_score(_p(x), layout, rows, plane, 96, _p(d["centres"]), _p(d["tables"]), T, ctypes.cast(ids, ctypes.c_void_p),
                                    _p(d["offsets"]), _p(d["consts"]), nc, float(max_d2), _p(classes), _p(distance), _p(s), out_layout, _stream()),
               "msst_gauss_score")
    classes, distance = classes.cpu(), distance.cpu()
    assert not bool((classes == SENTINEL).any()) and not bool((distance == -12345.5).any())
    if s is not None:
        s = s.cpu()
        assert not bool((s == -12345.5).any())
    return classes, distance, s


def t32(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def check_exact(x, features, tab, max_d2=float("inf")):
    """rows x (numpy) given as `features` (rows or a map on the device) against the whole-number reference, bit for bit"""
    want_c, want_d, want_s = gu.int_reference(x, tab, max_d2)
    classes, distance, scores = raw_score(features, tab, max_d2)
    assert torch.equal(classes, t32(want_c)), (classes != t32(want_c)).nonzero()[:5]
    assert same_bits(distance, t32(want_d)) or torch.equal(torch.nan_to_num(distance, nan=-1.0), torch.nan_to_num(t32(want_d), nan=-1.0))
    assert torch.equal(torch.nan_to_num(scores, nan=-1.0, neginf=-2.0), torch.nan_to_num(t32(want_s), nan=-1.0, neginf=-2.0))
    assert torch.equal(torch.isnan(scores), torch.isnan(t32(want_s))) and torch.equal(torch.isnan(distance), torch.isnan(t32(want_d)))
    # without the scores: the same classes and distances
    c2, d2, none = raw_score(features, tab, max_d2, scores=False)
    assert none is None and torch.equal(c2, classes) and same_bits(d2, distance)
    return classes, distance, scores


# --------------------------------------------------------------------------------------------------- 1. exact on whole numbers
@pytest.mark.parametrize("form", gu.INT_FORMS)
@pytest.mark.parametrize("nc", gu.INT_NC)
def test_scores_are_exact_for_every_class_count(nc, form):
    for kind in gu.NAN_KINDS:
        x = gu.int_rows(321, kind)
        check_exact(x, dev(x), gu.int_tables(nc, form))
    x = gu.int_rows(321, "ends")
    classes, _, scores = check_exact(x, dev(x), gu.int_tables(nc, form, duplicate=True, zero_prior=True))
    if nc > 2:
        assert not bool((classes == 0).any()) and not bool((classes == nc - 1).any()) and bool(torch.isneginf(scores[1:-1, 0]).all())


@pytest.mark.parametrize("form", gu.INT_FORMS)
@pytest.mark.parametrize("M", gu.INT_ROWS)
def test_scores_are_exact_for_every_row_count(M, form):
    x = gu.int_rows(M, "ends" if M > 1 else "none")
    check_exact(x, dev(x), gu.int_tables(17, form, duplicate=True))


@pytest.mark.parametrize("case", gu.INT_ROWS_LONG, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
def test_scores_are_exact_over_several_row_blocks(case):
    M, nc, form = case
    x = gu.int_rows(M, "tile")
    check_exact(x, dev(x), gu.int_tables(nc, form))


@pytest.mark.parametrize("shape", gu.INT_MAPS)
def test_scores_are_exact_on_a_map_read_in_place(shape):
    Bs, Hs, Ws = shape
    plane = Hs * Ws
    for nc, form in ((17, "full"), (17, "tied"), (40, "grouped")):
        tab = gu.int_tables(nc, form, duplicate=True)
        for kind in gu.NAN_KINDS:
            x = gu.int_rows(Bs * plane, kind)
            xm = dev(pu.to_map(x, Bs, plane)).view(Bs, 96, Hs, Ws)
            classes, distance, scores = check_exact(x, xm, tab)
            cm, dm, sm = raw_score(xm, tab, out_layout=1)                        # ... and into a map, the layout of predict_scene's logits
            assert sm.shape == (Bs, nc, Hs, Ws) and torch.equal(cm, classes) and same_bits(dm, distance)
            back = t32(pu.from_map(sm.view(Bs, nc, plane).numpy()))
            assert torch.equal(torch.nan_to_num(back, nan=-1.0, neginf=-2.0), torch.nan_to_num(scores, nan=-1.0, neginf=-2.0))


def test_ties_go_to_the_lowest_index_and_rejection_is_strict():
    x = gu.int_rows(321)
    for form in gu.INT_FORMS:
        tab = gu.int_tables(17, form, duplicate=True)
        classes, distance, scores = check_exact(x, dev(x), tab)
        assert same_bits(scores[:, 0].contiguous(), scores[:, 16].contiguous()) and not bool((classes == 16).any()) and bool((classes == 0).any())
        k = int(torch.nonzero(classes == 0)[0])
        at = float(distance[k])
        below = float(np.nextafter(np.float32(at), np.float32(0)))
        kept = check_exact(x, dev(x), tab, max_d2=at)[0]                         # a distance of exactly max_d2 is not rejected
        cut = check_exact(x, dev(x), tab, max_d2=below)[0]                       # ... one ulp below it, it is
        assert kept[k] == 0 and cut[k] == -2 and bool((kept == -2).any())
        assert same_bits(raw_score(dev(x), tab, max_d2=below)[2], scores)        # the scores do not know about the rejection


# ------------------------------------------------------------------------------------------------------------ 2. against float64
def given(model):
    from maskedsst_amd import GaussianClassifier
    return GaussianClassifier(model["means"], model["covariances"], model["priors"], tied=model["tied"])


@pytest.mark.parametrize("case", gu.REAL_CASES, ids=lambda c: gu.real_name(*c))
def test_scores_against_float64(case):
    M, nc, form = case
    x, labels = gu.real_rows(M, nc, form)
    want_c, want_s, want_d, margin = gu.real_reference(M, nc, form)
    clf = given(gu.real_model(nc, form))
    res = clf.classify(dev(x))
    assert res.classes.dtype == torch.int64 and res.classes.shape == (M,) and res.scores.shape == (M, nc) and res.distance.shape == (M,)
    got_c = res.classes.cpu().numpy()
    err = dict(scores=gu.relmax(res.scores.cpu().numpy(), want_s), distance=gu.relmax(res.distance.cpu().numpy(), want_d))
    name = gu.real_name(M, nc, form)
    bar = gu.bars(name)
    # classes: equal on every row whose float64 top-two margin reaches the gap, 4 x the measured score error
    gap = (4.0 * err["scores"] if bar is None else bar["scores"]) * np.nanmax(np.abs(want_s))
    sure = (margin >= gap) | (want_c < 0)
    print(f"{name}: gap {gap:.3g}, {int((~sure).sum())} rows under it")
    assert gu.under_gap(margin, want_c, gap) <= gu.MARGIN_SHARE
    assert np.array_equal(got_c[sure], want_c[sure]) and int((got_c == -1).sum()) == gu.REAL_NAN_ROWS
    assert ((got_c >= 0) | (want_c < 0)).all()
    gu.check(name, err)
    # the distance is the d2 of the predicted class: the score turned round (fp32: the constant and the halving round once)
    ok = got_c >= 0
    s_at = res.scores.cpu().numpy()[ok, got_c[ok]].astype(np.float64)
    const = clf._host["consts"].astype(np.float64)[got_c[ok]]
    d = res.distance.cpu().numpy()[ok].astype(np.float64)
    assert np.abs((const - 0.5 * d) - s_at).max() <= 2.0 ** -23 * np.abs(s_at).max()
    # rejection at the bank's own quantile, and classify without scores
    limit = float(np.quantile(want_d[want_c >= 0], 0.9))
    cut = clf.classify(dev(x), scores=False, max_distance=limit)
    assert cut.scores is None and same_bits(cut.distance, res.distance)
    want_cut = np.where((res.distance.cpu().numpy() > np.float32(limit)) & ok, -2, got_c)
    assert np.array_equal(cut.classes.cpu().numpy(), want_cut) and 0.05 < (want_cut == -2).mean() < 0.15


# ------------------------------------------------------------------------------------------------------------------------ 3. the fit
def make_bank(x, labels, nc):
    from maskedsst_amd import KnnBank
    return KnnBank(dev(x), torch.from_numpy(labels).cuda(), nc)


def fit_dict(clf):
    return dict(means=clf.means.cpu().double().numpy(), covariances=clf.pooled_covariance if clf.tied else clf.covariances,
                pooled=clf.pooled_covariance, logdet=clf.logdet, priors=clf.priors)


@pytest.mark.parametrize("case", gu.FIT_CASES, ids=lambda c: gu.fit_name(*c))
def test_fit_against_float64(case):
    from maskedsst_amd import fit_gaussian
    covariance, shrinkage = case
    x, labels, nc = gu.fit_bank()
    ref = gu.fit64(x, labels, nc, covariance, shrinkage)
    bank = make_bank(x, labels, nc)
    clf = fit_gaussian(bank, covariance=covariance, shrinkage=shrinkage)
    assert clf.tied == (covariance == "tied") and np.array_equal(clf.counts, ref["counts"]) and clf.counts.dtype == np.int64
    assert clf.priors[2] == 0 and np.isnan(clf.logdet).sum() == (0 if clf.tied else 1) and (clf.covariances is None) == clf.tied
    gu.check(gu.fit_name(covariance, shrinkage), gu.fit_errors(fit_dict(clf), ref))
    # the empty class is never predicted and scores -inf; a second fit repeats every bit
    res = clf.classify(bank)
    assert not bool((res.classes == 2).any()) and bool(torch.isneginf(res.scores[:, 2]).all()) and bool(torch.isfinite(res.scores[:, [0, 1, 3, 4, 5]]).all())
    assert float((res.classes.cpu() == torch.from_numpy(labels)).double().mean()) > 0.99
    again = fit_gaussian(bank, covariance=covariance, shrinkage=shrinkage)
    assert same_bits(again.means, clf.means) and np.array_equal(again.pooled_covariance, clf.pooled_covariance)
    assert all(np.array_equal(again._host[k], clf._host[k]) for k in clf._host)
    for priors in ("uniform", [1.0, 2.0, 5.0, 1.0, 0.0, 1.0]):
        other = fit_gaussian(bank, covariance=covariance, shrinkage=shrinkage, priors=priors)
        want = gu.fit64(x, labels, nc, covariance, shrinkage, priors=priors)["priors"]
        assert np.abs(other.priors - want).max() < 1e-15 and other.priors[2] == 0
        if priors != "uniform":
            assert other.priors[4] == 0 and not bool((other.classify(bank, scores=False).classes == 4).any())


def test_fit_class_count_rules():
    from maskedsst_amd import fit_gaussian
    x, labels, nc = gu.fit_bank(single=True)
    bank = make_bank(x, labels, nc)
    with pytest.raises(ValueError, match="class 5"):
        fit_gaussian(bank)
    with pytest.raises(ValueError, match="class 5"):
        fit_gaussian(bank, shrinkage=0.5)
    ref = gu.fit64(x, labels, nc, "tied")
    clf = fit_gaussian(bank, covariance="tied")                                  # a class of one row has a mean: a tied fit takes it
    gu.check(gu.fit_name("tied", 0.0, single=True), gu.fit_errors(fit_dict(clf), ref))
    assert clf.counts[5] == 1 and same_bits(clf.means[5].cpu(), torch.from_numpy(x[labels == 5][0]))
    full = fit_gaussian(bank, shrinkage=1.0)                                     # ... and so does full with the pooled covariance alone
    assert not full.tied and np.array_equal(full.covariances[5], clf.pooled_covariance)
    with pytest.raises(ValueError, match="ddof"):
        fit_gaussian(make_bank(x[:3], np.array([0, 1, 2]), 3), covariance="tied")      # no class has more than ddof rows
    from maskedsst_amd import KnnBank
    holed = KnnBank.__new__(KnnBank)                                             # (the constructor would refuse it: built past it)
    xn = x.copy()
    xn[int(np.nonzero(labels == 3)[0][0]), 7] = np.nan
    holed.features, holed.labels, holed.n_classes = dev(xn), torch.from_numpy(labels).to(torch.int32).cuda(), nc
    with pytest.raises(ValueError, match="class 3 .* finite"):
        fit_gaussian(holed, covariance="tied")
    flat = np.zeros((40, 96), dtype=np.float32)
    with pytest.raises(ValueError, match="eigenvalue"):
        fit_gaussian(make_bank(flat, np.arange(40) % 2, 2))


def test_trace_identity_and_threshold():
    """under full covariances with shrinkage 0 and nothing at the floor the own-class distances of the fitted rows sum to
    sum_c (n_c - ddof) x 96; threshold is the quantile of those distances"""
    from maskedsst_amd import fit_gaussian
    x, labels, nc = gu.fit_bank()
    bank = make_bank(x, labels, nc)
    clf = fit_gaussian(bank)
    own = clf.own_distance(bank)
    assert own.shape == (len(x),) and bool(torch.isfinite(own).all())
    total, want = float(own.double().sum()), float((clf.counts[clf.counts > 0] - 1).sum() * 96)
    gu.check("trace_full", dict(trace=abs(total - want) / want))
    # own_distance is the distance classify reports wherever the row's own class wins (the same bits: a class alone or among all)
    res = clf.classify(bank, scores=False)
    hit = res.classes == torch.from_numpy(labels).cuda()
    assert float(hit.double().mean()) > 0.99 and same_bits(own[hit], res.distance[hit])
    srt = np.sort(own.cpu().numpy())
    for q in (0.5, 0.99, 1.0):
        t = clf.threshold(bank, quantile=q)
        assert t == float(srt[int(np.ceil(q * len(srt))) - 1]) and abs(float((own <= t).double().mean()) - q) <= 1.0 / len(srt)
    kept = clf.classify(bank, scores=False, max_distance=clf.threshold(bank, 0.99))
    assert abs(float((kept.classes == -2).double().mean()) - 0.01) < 2e-3


# ------------------------------------------------------------------------------------------------------------------- 4. equal bits
@pytest.mark.parametrize("form", ["full", "tied"])
def test_equal_inputs_give_equal_bits(form):
    M, nc = 3000, 16
    x, _ = gu.real_rows(M, nc, form)
    clf = given(gu.real_model(nc, form))
    xd = dev(x)
    a, b = clf.classify(xd), clf.classify(xd)
    assert torch.equal(a.classes, b.classes) and same_bits(a.scores, b.scores) and same_bits(a.distance, b.distance)
    lean = clf.classify(xd, scores=False)
    assert lean.scores is None and torch.equal(lean.classes, a.classes) and same_bits(lean.distance, a.distance)
    for k in (0, 29, 1000, 2999):                                                # a row alone (row 29 has a NaN channel)
        one = clf.classify(xd[k:k + 1].contiguous())
        assert torch.equal(one.classes, a.classes[k:k + 1]) and same_bits(one.scores[0], a.scores[k]) and same_bits(one.distance[0], a.distance[k])
    part = clf.classify(xd[1000:1130].contiguous())                              # other tiles, another batch
    assert same_bits(part.scores, a.scores[1000:1130].contiguous()) and same_bits(part.distance, a.distance[1000:1130].contiguous())
    xm = dev(pu.to_map(x, 3, 1000)).view(3, 96, 40, 25)                          # inside a map
    m = clf.classify(xm)
    assert torch.equal(m.classes, a.classes) and same_bits(m.scores, a.scores) and same_bits(m.distance, a.distance)


# ----------------------------------------------------------------------------------------------------------- 5. through the model
@pytest.mark.parametrize("stride", [8, 5])
def test_scene_call_through_the_model(stride):
    from maskedsst_amd import GaussianScene, KnnBank, fit_gaussian, gaussian_predict_scene
    model = make_model()
    model.train()
    g = torch.Generator().manual_seed(3)
    scene = torch.randn(2, 50, 16, 16, generator=g).cuda()
    emb = model.encode_scene(scene, stride=stride, normalize=False)
    covered = emb.cover > 0
    assert bool(covered.all()) == (stride == 8)                              # stride 5: rows and columns 13 .. 15 lie in no window
    rows = emb.features.permute(0, 2, 3, 1).reshape(-1, 96).contiguous()
    labels = (torch.arange(rows.shape[0]) % 3).cuda()
    keep = covered.reshape(-1)
    for covariance in ("tied", "full"):
        clf = fit_gaussian(KnnBank(rows[keep].contiguous(), labels[keep], 3), covariance=covariance, shrinkage=0.0 if covariance == "tied" else 0.5)
        limit = clf.threshold(KnnBank(rows[keep].contiguous(), labels[keep], 3), 0.9)
        for md in (None, limit):
            res = model.gaussian_predict_scene(scene, clf, stride=stride, max_distance=md)
            assert isinstance(res, GaussianScene) and model.training and torch.equal(res.cover, emb.cover)
            assert res.classes.shape == (2, 16, 16) and res.classes.dtype == torch.int64 and res.scores.shape == (2, 3, 16, 16) and res.distance.shape == (2, 16, 16)
            flat = clf.classify(rows, max_distance=md)
            assert torch.equal(res.classes.reshape(-1), flat.classes) and same_bits(res.distance.reshape(-1), flat.distance)
            assert same_bits(res.scores.permute(0, 2, 3, 1).reshape(-1, 3).contiguous(), flat.scores)
            assert torch.equal(res.classes == -1, ~covered) and torch.equal(torch.isnan(res.distance), ~covered)
            assert torch.equal(torch.isnan(res.scores).all(dim=1), ~covered) and torch.equal(torch.isnan(res.scores).any(dim=1), ~covered)
            assert bool(((res.classes == -2) == ((res.distance > limit) & covered)).all()) if md is not None else not bool((res.classes == -2).any())
            other = gaussian_predict_scene(model, scene, clf, stride=stride, max_distance=md)
            assert torch.equal(other.classes, res.classes) and same_bits(other.scores, res.scores) and same_bits(other.distance, res.distance)


# ------------------------------------------------------------------------------------------------------------------------ 6. scripts
@pytest.mark.parametrize("covariance", ["full", "tied"])
def test_finetune_val_gauss_script(covariance):
    """finetune.py --val-gauss: one more line per validation pass"""
    out = child([sys.executable, "finetune.py", "--steps", "1", "--val-scenes", "4", "--val-every", "1", "--val-gauss", covariance], 600)
    lines = [l.split() for l in out.splitlines() if l.startswith("val-gauss step ")]
    assert [e[2] for e in lines] == ["1"], out
    e = lines[0]
    assert e[3:5] == ["cov", covariance] and e[5] == "gauss_acc" and 0.0 <= float(e[6]) <= 1.0, e
    assert e[7] == "mean_d2" and float(e[8]) > 0 and e[9] == "rejected" and 0.0 <= float(e[10]) <= 1.0, e
    assert e[11] == "bank_pixels" and int(e[12]) > 0 and e[13] == "test_pixels" and int(e[14]) > 0 and e[15:] == ["scenes", "4"], e


def test_gauss_time_script():
    """tools/gauss_time.py --smoke: exit 0 and ONE JSON line, nothing appended"""
    out = child([sys.executable, os.path.join("tools", "gauss_time.py"), "--smoke"], 300)
    lines = [l for l in out.splitlines() if l.strip()]
    assert len(lines) == 1, out
    row = json.loads(lines[0])
    assert row["tool"] == "gauss_time" and row["Q"] == 8192 and row["nc"] == 16 and row["covariance"] == "full"
    assert row["hip_us"] > 0 and row["eager_us"] > 0 and isinstance(row["eager_faster"], bool)
