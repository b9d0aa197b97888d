"""GPU: Gaussian mixtures (EM) of frozen features -- msst_gmm_posterior, msst_gmm_moments, msst_gmm_update
(maskedsst_amd/csrc/msst_gmm.hip) and maskedsst_amd/mixture.py against the float64 restatement of tests/gmm_util.py: exact on
whole-number data with hard responsibilities (no tolerance: n, s1, s2, the counted rows and a zero sum of lse, every component count,
both layouts, NaN rows, a starved component, a row without any finite score), the posterior alone, the M-step and whole fits
teacher-forced (float64 takes the DEVICE'S OWN scores and centres, so that the fp32 error of the scores does not pile up over the
iterations), equal bits from equal inputs, and the route through the model.  The bars are 4 x the errors measured on the MI355X
(profiles/gmm_parity_measured.jsonl); tests/test_gmm_host.py checks on the CPU that they still catch the mutants.

The planted cases and what they exercise are described in tests/gmm_util.py (CASES, planted, nearest_init)."""
import json
import sys

import numpy as np
import pytest
import torch

import gmm_util as gu
from test_gpu_pca import child, dev, make_model, same_bits

pytestmark = pytest.mark.gpu

ROW = 1 + 96 + 96 * 96
NAMES = ("weights", "means", "covariances", "tables", "logdet", "consts")


def partition(rows):
    """(workgroups, tiles) of a row count, read from the slab size the library reports"""
    from maskedsst_amd.mixture import gmm_scratch_floats
    return gmm_scratch_floats(rows, 1) // (ROW + 2), (rows + 63) // 64


def two_tile_rows():
    """the smallest row count at which at least two workgroups take part and one of them owns two tiles"""
    for tiles in range(1, 4096):
        rows = 64 * (tiles - 1) + 1
        nwg, t = partition(rows)
        if nwg >= 2 and t > nwg:
            return rows
    raise AssertionError("no such row count")


def device_state(old):
    return {name: dev(np.asarray(old[name], dtype=np.float32)) for name in NAMES}


def host_state(state):
    return {name: state[name].cpu().numpy().astype(np.float64) for name in NAMES}


def raw_m_step(features, scores, state, covariance="full", reg_covar=1e-6, min_count=1.0):
    """msst_gmm_moments and msst_gmm_update with the slab and raw prefilled with NaN, in place on `state`: (record, raw) on the CPU;
    nothing of raw may be left unwritten"""
    from maskedsst_amd.mixture import gmm_moments, gmm_scratch_floats, gmm_update
    from maskedsst_amd.pca import _source
    _, _, rows, _ = _source(features)
    k = state["means"].shape[0]
    slab = torch.full((gmm_scratch_floats(rows, k),), float("nan"), device="cuda")
    raw = torch.full((k, ROW), float("nan"), device="cuda")
    record = torch.zeros(4, device="cuda")
    gmm_moments(features, scores, state["means"], slab)
    gmm_update(slab, rows, state, covariance, reg_covar, min_count, record, raw)
    rec = record.cpu()
    raw = raw.cpu()
    assert not bool(torch.isnan(raw).any())
    return (float(rec[0]),) + tuple(rec[1:].view(torch.int32).tolist()), raw


# --------------------------------------------------------------------------------------------------- 1. exact on whole numbers
def int_case(rows, K, kind, seed):
    """whole-number rows in [-3, 3] (float32, NaN rows by kind), whole-number centres in [-2, 2], a label per row"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-3, 4, (rows, 96)).astype(np.float32)
    centres = rng.integers(-2, 3, (K, 96)).astype(np.float32)
    labels = rng.integers(0, K, rows)
    if kind == "ends":
        x[0, 5] = np.nan
        x[-1, 95] = np.inf
    elif kind == "tile" and rows > 64:
        x[64:128, 17] = np.nan
    elif kind == "all":
        x[:, 0] = np.nan
    return x, centres, labels


def as_map(x):
    """rows [M, 96] as a one-scene map [1, 96, 1, M]"""
    return np.ascontiguousarray(x.T).reshape(1, 96, 1, -1)


def check_exact(x, centres, labels, features, dead=()):
    K = len(centres)
    scores = gu.hard_scores(labels, K).astype(np.float32)
    scores[list(dead)] = -np.inf
    start = gu.start_params(K, centres)                         # values a kept component is recognised by
    state = device_state(start | dict(consts=np.zeros(K), tables=2.0 * start["tables"], covariances=5.0 * start["covariances"],
                                      logdet=np.full(K, 3.0)))
    before = host_state(state)
    rec, raw = raw_m_step(features, dev(scores), state, reg_covar=0.5)
    counted = np.isfinite(x).all(axis=1)
    counted[list(dead)] = False
    assert rec[1] == int(counted.sum()) and (rec[0] == 0.0 if counted.any() else np.isnan(rec[0]))
    xs = np.where(counted[:, None], x, 0.0).astype(np.float64)
    starved = 0
    after = host_state(state)
    for c in range(K):
        sel = counted & (labels == c)
        d = xs[sel] - centres[c].astype(np.float64)
        s2 = d.T @ d
        assert np.abs(s2).max() < 2 ** 24
        assert raw[c, 0] == float(sel.sum())
        assert np.array_equal(raw[c, 1:97].numpy(), d.sum(axis=0).astype(np.float32))
        assert np.array_equal(raw[c, 97:].view(96, 96).numpy(), s2.astype(np.float32))
        assert after["weights"][c] == np.float32(sel.sum() / max(1, counted.sum()))
        if not sel.any():          # starved: kept bit for bit
            starved += 1
            for name in ("means", "tables", "covariances", "logdet"):
                assert np.array_equal(after[name][c], before[name][c]), name
            assert after["weights"][c] == 0.0 and after["consts"][c] == -np.inf
        else:
            assert np.array_equal(after["covariances"][c], after["covariances"][c].T) and not np.triu(after["tables"][c], 1).any()
    assert rec[2] == starved and rec[3] == 0
    return rec, raw


@pytest.mark.parametrize("K", [1, 2, 3, 16, 17, 32])
def test_moments_are_exact_on_whole_numbers(K):
    long_rows = two_tile_rows()
    nwg, tiles = partition(long_rows)
    assert nwg >= 2 and tiles > nwg and partition(long_rows - 64)[1] <= partition(long_rows - 64)[0]
    for rows in (1, 63, 64, 65, 129, long_rows):
        for kind in (("ends",) if rows == long_rows else ("none", "ends", "tile", "all")):
            x, centres, labels = int_case(rows, K, kind, 100 * K + rows % 97)
            if K > 1:
                labels[labels == K - 1] = 0                     # the last component has no row: starved
            dead = (rows // 2,) if rows > 2 else ()             # a row whose scores are all -inf: skipped, not counted
            a = check_exact(x, centres, labels, dev(x), dead)
            b = check_exact(x, centres, labels, dev(as_map(x)), dead)
            assert repr(a[0]) == repr(b[0]) and same_bits(a[1], b[1])       # both layouts: the same bits (a record may hold NaN)


# --------------------------------------------------------------------------------------------------- 2. the posterior alone
def posterior_scores(K, rows=333, seed=0):
    rng = np.random.default_rng(seed)
    s = (-5000.0 + 30.0 * rng.standard_normal((rows, K))).astype(np.float32)
    if K > 1:
        s[::7, rng.integers(0, K)] = -np.inf                    # a component of weight 0
        s[3::11, 1] = s[3::11, 0] = s[3::11].max(axis=1)        # two equal maxima
        s[5] = -np.inf                                          # no finite score
    s[9] = np.nan
    s[11::13] = (0.01 * rng.standard_normal((len(s[11::13]), K))).astype(np.float32)   # near-uniform responsibilities
    return s


@pytest.mark.parametrize("K", [1, 2, 3, 16, 32, 128])
def test_posterior_against_float64(K):
    from maskedsst_amd.mixture import gmm_posterior
    s = posterior_scores(K)
    rows = len(s)
    want_lse, want_p = gu.posterior(s.astype(np.float64))
    lse, p = gmm_posterior(dev(s), 0, rows, 1, K)
    lse, p = lse.cpu().numpy().astype(np.float64), p.cpu().numpy().astype(np.float64)
    assert np.array_equal(np.isnan(lse), np.isnan(want_lse)) and np.array_equal(np.isneginf(lse), np.isneginf(want_lse))
    assert np.array_equal(np.isnan(p), np.isnan(want_p)) and np.isnan(lse[9]) and (K == 1 or (lse[5] == -np.inf and not p[5].any()))
    fin = np.isfinite(want_lse)
    if K == 1:
        assert np.array_equal(lse[fin], s[fin, 0].astype(np.float64)) and (p[fin] == 1.0).all()
    assert (p[fin][np.isneginf(s[fin])] == 0.0).all()           # a score of -inf contributes exactly 0
    err = dict(lse=float((np.abs(lse[fin] - want_lse[fin]) / (1.0 + np.abs(want_lse[fin]))).max()),
               probs=float(np.abs(p[fin] - want_p[fin]).max()), prob_sum=float(np.abs(p[fin].sum(axis=1) - 1.0).max()))
    gu.check(f"posterior_{K}", err)


@pytest.mark.parametrize("K", [3, 32])
def test_posterior_row_has_the_same_bits_alone_in_a_batch_and_in_a_map(K):
    from maskedsst_amd.mixture import gmm_posterior
    s = posterior_scores(K, rows=2 * 7 * 9)
    lse, p = gmm_posterior(dev(s), 0, len(s), 1, K)
    for q in (0, 3, 5, 9, 64, len(s) - 1):
        l1, p1 = gmm_posterior(dev(s[q:q + 1]), 0, 1, 1, K)
        assert same_bits(l1, lse[q:q + 1]) and same_bits(p1, p[q:q + 1])
    smap = dev(np.ascontiguousarray(s.reshape(2, 63, K).transpose(0, 2, 1)).reshape(2, K, 7, 9))
    lm, pm = gmm_posterior(smap, 1, len(s), 63, K, out_layout=1)
    assert same_bits(lm, lse) and pm.shape == smap.shape and same_bits(pm.reshape(2, K, 63).permute(0, 2, 1).reshape(-1, K).contiguous(), p)
    _, pr = gmm_posterior(smap, 1, len(s), 63, K, out_layout=0)
    assert same_bits(pr, p)
    lonly, none = gmm_posterior(dev(s), 0, len(s), 1, K, probs=False)
    assert none is None and same_bits(lonly, lse)


# --------------------------------------------------------------------------------------------------- 3. the M-step, teacher-forced
@pytest.fixture(scope="module")
def planted():
    return {case: gu.planted(case) for case in gu.CASES}


def forced_step(x, xd, scores, state, covariance, case):
    """one device M-step from given fp32 scores (numpy) in place on `state` against float64 from the same scores and centres"""
    old = host_state(state)
    want, want_rec, _ = gu.m_step(x, scores.astype(np.float64), old, covariance, gu.TEST_REG_COVAR)
    rec, raw = raw_m_step(xd, dev(scores), state, covariance, gu.TEST_REG_COVAR)
    assert rec[1:] == tuple(want_rec[1:])
    got = host_state(state)
    err = gu.m_step_errors(got, want)
    err["history"] = abs(rec[0] - want_rec[0]) / (1.0 + abs(want_rec[0]))
    err["consts"] = float((np.abs(got["consts"] - want["consts"]) / (1.0 + np.abs(want["consts"]))).max())
    for c in range(len(old["weights"])):
        assert np.array_equal(got["covariances"][c], got["covariances"][c].T)
        if covariance == "diag":
            assert not (got["covariances"][c] - np.diag(np.diag(got["covariances"][c]))).any()
    gu.check(case, err)


def device_scores(xd, state):
    from maskedsst_amd.gaussian import gauss_score
    k = state["means"].shape[0]
    _, _, s = gauss_score(xd, state["means"], state["tables"], range(k), torch.zeros(k, 96, device="cuda"), state["consts"], scores=True)
    return s.cpu().numpy()


@pytest.mark.parametrize("covariance", ["full", "diag"])
@pytest.mark.parametrize("case", ["A", "B", "C"])
def test_m_step_against_float64_from_the_devices_own_scores(case, covariance, planted):
    x, _, _ = planted[case]
    K = gu.CASES[case]["K"]
    xd = dev(x)
    labels, centres = gu.nearest_init(x, K, 5)
    state = device_state(gu.start_params(K, centres) | dict(consts=np.zeros(K)))
    forced_step(x, xd, gu.hard_scores(labels, K).astype(np.float32), state, covariance, f"mstep_hard_{case}_{covariance}")
    for it in range(2):                                         # soft responsibilities, from the device's own scores
        forced_step(x, xd, device_scores(xd, state), state, covariance, f"mstep_soft{it}_{case}_{covariance}")


# --------------------------------------------------------------------------------------------------- 4. whole fits, teacher-forced
@pytest.mark.parametrize("init", ["kmeans", "rows"])
@pytest.mark.parametrize("case", ["A", "B"])
def test_fit_teacher_forced_at_every_iteration(case, init, planted):
    """init "kmeans": the default route, which on these planted cases starts next to the optimum; "rows": a KMeans of K random rows
    (tests/gmm_util.py: nearest_init), a poor start from which the responsibilities stay soft for several iterations"""
    from maskedsst_amd import KMeans, fit_kmeans, fit_mixture
    x, _, _ = planted[case]
    K = gu.CASES[case]["K"]
    xd = dev(x)
    name = f"fit_{case}_{init}"
    if init == "kmeans":
        km = fit_kmeans(xd, K, metric="euclidean", init="kmeans++", seed=0)
    else:
        km = KMeans(dev(gu.nearest_init(x, K, 5)[1].astype(np.float32)), metric="euclidean")
    # the fit of t iterations is the prefix of every longer one: its parameters are what iteration t (0-based) starts from
    fits = {t: fit_mixture(xd, K, iters=t, reg_covar=gu.TEST_REG_COVAR, init=km) for t in range(1, gu.FIT_ITERS + 1)}
    full = fits[gu.FIT_ITERS]
    assert full.history.shape == (gu.FIT_ITERS, 4) and not full.converged
    if init == "kmeans":
        named = fit_mixture(xd, K, iters=gu.FIT_ITERS, reg_covar=gu.TEST_REG_COVAR, init="kmeans", seed=0)
        assert torch.equal(named.history, full.history) and all(same_bits(getattr(named, n), getattr(full, n)) for n in NAMES)
    # what iteration 0 starts from: the M-step of the k-means assignment about its centroids, by the documented recipe
    labels = km.assign(xd)[0].cpu().numpy()
    state = device_state(gu.start_params(K, km.centroids.cpu().numpy()) | dict(consts=np.zeros(K)))
    raw_m_step(xd, dev(gu.hard_scores(labels, K).astype(np.float32)), state, "full", gu.TEST_REG_COVAR)
    states = {0: state} | {t: {name: getattr(fits[t], name) for name in NAMES} for t in fits}
    err = dict(scores=0.0, history=0.0, weights=0.0, means=0.0, logdet=0.0, covariances=0.0, tables=0.0)
    ready = gu.committed(name)
    for t in range(gu.FIT_ITERS + 1):
        old = host_state(states[t])
        s_dev = device_scores(xd, states[t])
        s64, _ = gu.scores_of(x, old)
        err["scores"] = max(err["scores"], float(np.abs(s_dev - s64).max()))
        if t >= 1:
            gm = fits[t]
            assert torch.equal(gm.history, full.history[:t])
            assert tuple(gm.history[t - 1, 1:].tolist()) == (float(len(x)), 0.0, 0.0)
            # classes: equal wherever float64 is sure -- the gap is 4 x the committed score error, the rows left out at most 1 %
            gap = gu.bars(name)["scores"] if ready else 4.0 * err["scores"]
            top = np.sort(s64, axis=1)
            sure = (top[:, -1] - top[:, -2]) >= gap
            assert (~sure).mean() <= 0.01
            res = gm.predict(xd, probs=True)
            assert np.array_equal(res.classes.cpu().numpy()[sure], gu.classes_of(s64)[sure])
            if ready:
                _, p64 = gu.posterior(s_dev.astype(np.float64))
                assert np.abs(res.probs.cpu().numpy() - p64).max() <= gu.bars()["probs"]
        if t < gu.FIT_ITERS:                                    # iteration t of the longer fits, forced from these scores
            want, want_rec, _ = gu.m_step(x, s_dev.astype(np.float64), old, "full", gu.TEST_REG_COVAR)
            step = gu.m_step_errors(host_state(states[t + 1]), want)
            for what, v in step.items():
                err[what] = max(err[what], v)
            err["history"] = max(err["history"], abs(float(full.history[t, 0]) - want_rec[0]) / (1.0 + abs(want_rec[0])))
    print(f"{name}: mean log-likelihood per iteration {full.history[:, 0].tolist()}")
    gu.check(name, err)


# --------------------------------------------------------------------------------------------------- 5. properties
def test_two_fits_give_the_same_bits_and_check_every_the_shorter_fit(planted):
    from maskedsst_amd import fit_mixture
    x, _, _ = planted["A"]
    xd = dev(x)
    a = fit_mixture(xd, 3, iters=6, reg_covar=gu.TEST_REG_COVAR, seed=1)
    b = fit_mixture(xd, 3, iters=6, reg_covar=gu.TEST_REG_COVAR, seed=1)
    for name in NAMES:
        assert same_bits(getattr(a, name), getattr(b, name)), name
    assert torch.equal(a.history, b.history) and a.covariance == "full" and a.reg_covar == gu.TEST_REG_COVAR
    # the log-likelihood of a well separated case stops rising: check_every ends the fit early, with the bits of the shorter fit
    long = fit_mixture(xd, 3, iters=30, reg_covar=gu.TEST_REG_COVAR, seed=1, check_every=2, tol=1e-3)
    done = len(long.history)
    assert long.converged and done < 30 and done % 2 == 0
    assert float(long.history[-1, 0]) - float(long.history[-2, 0]) < 1e-3
    short = fit_mixture(xd, 3, iters=done, reg_covar=gu.TEST_REG_COVAR, seed=1)
    assert not short.converged and torch.equal(short.history, long.history)
    for name in NAMES:
        assert same_bits(getattr(short, name), getattr(long, name)), name
    diag = fit_mixture(xd, 3, covariance="diag", iters=3, reg_covar=gu.TEST_REG_COVAR)
    assert diag.covariance == "diag" and not bool((diag.covariances - torch.diag_embed(torch.diagonal(diag.covariances, dim1=1, dim2=2))).any())
    assert bool((torch.diff(diag.history[:, 0]) >= -1e-4).all())


def test_predict_on_a_map_equals_predict_on_its_rows_and_bic(planted):
    from maskedsst_amd import GaussianMixture, KnnBank, fit_mixture
    x, truth, _ = planted["A"]
    xd = dev(x)
    bank = KnnBank(xd, dev(truth), 3)
    gm = fit_mixture(bank, 3, iters=4, reg_covar=gu.TEST_REG_COVAR)
    xm = x.copy()
    xm[7, 3] = np.nan
    rows = gm.predict(dev(xm), probs=True)
    fmap = dev(np.ascontiguousarray(xm.reshape(2, 1500, 96).transpose(0, 2, 1)).reshape(2, 96, 30, 50))
    maps = gm.predict(fmap, probs=True)
    for a, b in zip(rows, maps):
        assert same_bits(a, b)
    assert rows.classes.dtype == torch.int64 and int(rows.classes[7]) == -1 and bool(torch.isnan(rows.log_likelihood[7]))
    assert bool(torch.isnan(rows.distance[7])) and bool(torch.isnan(rows.probs[7]).all()) and int((rows.classes == -1).sum()) == 1
    one = gm.predict(dev(xm[100:101]), probs=True)
    assert same_bits(one.log_likelihood, rows.log_likelihood[100:101]) and same_bits(one.probs, rows.probs[100:101])
    assert gm.predict(xd).probs is None
    # bic / aic from the same log-likelihood, 2999 counted rows
    ll = rows.log_likelihood.cpu().numpy().astype(np.float64)
    total = float(np.nansum(ll))
    assert gm.bic(dev(xm)) == pytest.approx(gu.bic(total, 2999, 3, "full"), rel=1e-12)
    assert gm.aic(dev(xm)) == pytest.approx(-2.0 * total + 2.0 * gu.n_parameters(3, "full"), rel=1e-12)
    # a mixture built from the fit's own arrays predicts the fit's classes
    again = GaussianMixture(gm.weights, gm.means, gm.covariances)
    assert again.means.is_cuda and torch.equal(again.predict(xd).classes, gm.predict(xd).classes)
    refit = fit_mixture(xd, 3, iters=1, reg_covar=gu.TEST_REG_COVAR, init=again)
    assert refit.history.shape == (1, 4) and float(refit.history[0, 0]) >= float(gm.history[-1, 0]) - 1e-3


@pytest.mark.parametrize("stride", [8, 5])
def test_mixture_scene_through_the_model(stride):
    from maskedsst_amd import MixtureScene, fit_mixture, mixture_scene
    model = make_model()
    model.train()
    g = torch.Generator().manual_seed(3)
    scene = torch.randn(2, 50, 16, 16, generator=g).cuda()
    emb = model.encode_scene(scene, stride=stride, normalize=False)
    covered = emb.cover > 0
    assert bool(covered.all()) == (stride == 8)                              # stride 5: rows and columns 13 .. 15 lie in no window
    feats = emb.features.permute(0, 2, 3, 1)[covered].contiguous()
    gm = fit_mixture(feats, 4, iters=3, reg_covar=1e-2)
    res = model.mixture_scene(scene, gm, stride=stride, probs=True)
    assert isinstance(res, MixtureScene) and model.training and torch.equal(res.cover, emb.cover)
    assert res.classes.shape == (2, 16, 16) and res.probs.shape == (2, 4, 16, 16)
    assert torch.equal(res.classes == -1, ~covered) and torch.equal(torch.isnan(res.log_likelihood), ~covered)
    assert torch.equal(torch.isnan(res.distance), ~covered) and torch.equal(torch.isnan(res.probs).all(dim=1), ~covered)
    assert torch.equal(torch.isnan(res.probs).any(dim=1), ~covered)
    flat = gm.predict(emb.features, probs=True)
    assert torch.equal(flat.classes.view(2, 16, 16), res.classes) and same_bits(flat.log_likelihood.view(2, 16, 16), res.log_likelihood)
    assert same_bits(flat.probs.view(2, 256, 4).permute(0, 2, 1).reshape(2, 4, 16, 16).contiguous(), res.probs)
    other = mixture_scene(model, scene, gm, stride=stride)
    assert other.probs is None and torch.equal(other.classes, res.classes) and same_bits(other.distance, res.distance)
    with pytest.raises(ValueError):
        model.mixture_scene(scene, "gm")


# --------------------------------------------------------------------------------------------------- 6. the two scripts
@pytest.mark.parametrize("covariance", ["full", "diag"])
def test_finetune_prints_the_val_gmm_line(covariance):
    out = child([sys.executable, "finetune.py", "--steps", "1", "--val-scenes", "4", "--val-every", "1", "--val-gmm", "4", "--val-gmm-cov",
                 covariance], 600)
    lines = [ln for ln in out.splitlines() if ln.startswith("val-gmm ")]
    assert len(lines) == 1, out[-2000:]
    e = lines[0].split()
    assert e[1:7] == ["step", "1", "k", "4", "cov", covariance], e
    assert e[7] == "cluster_acc" and 0.0 <= float(e[8]) <= 1.0 and e[9] == "purity" and 0.0 <= float(e[10]) <= 1.0
    assert e[11] == "nmi" and 0.0 <= float(e[12]) <= 1.0 and e[13] == "mean_ll" and np.isfinite(float(e[14]))
    assert e[15] == "starved" and int(e[16]) >= 0 and e[17] == "test_pixels" and int(e[18]) > 0 and e[19] == "train_pixels" and int(e[20]) > 0
    assert e[21:] == ["scenes", "4"], e
    plain = child([sys.executable, "finetune.py", "--steps", "1", "--val-scenes", "4", "--val-every", "1"], 600) if covariance == "full" else ""
    assert "val-gmm" not in plain


def test_timing_tool_smoke_run():
    out = child([sys.executable, "tools/gmm_time.py", "--smoke"], 600)
    rows = [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")]
    assert len(rows) == 1 and rows[0]["tool"] == "gmm_time" and rows[0]["M"] == 8192 and rows[0]["K"] == 4
    assert all(rows[0][n] > 0 for n in ("score_us", "moments_us", "update_us", "iter_us", "eager_us", "feat_moments_us"))
    assert rows[0]["covariances_agree"] < 1e-3
