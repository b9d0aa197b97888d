"""Gaussian mixtures (EM) of frozen features, host side (no GPU needed): the C ABI of the three msst_gmm_* calls (additive under
MSST_VERSION 109) and their argument checks (they run before any HIP call), the ValueError / RuntimeError surface of
maskedsst_amd/mixture.py, and the float64 restatement of tests/gmm_util.py: it agrees with scikit-learn where that is importable,
its log-likelihood never falls, its Cholesky route agrees with slogdet / solve, and the bars of tests/test_gpu_gmm.py (4 x what the
MI355X measured, profiles/gmm_parity_measured.jsonl) still tell it apart from each of its mutants."""
import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch

import gmm_util as gu

BADARG, UNSUPPORTED = -3, -2   # include/msst.h: MSST_ERR_BADARG, MSST_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def small():
    """a small planted mixture: 600 rows of case A's recipe, a random soft responsibility table and a nearest-row init"""
    x, truth, means = gu.planted("A")
    x = x[:600]
    labels, centres = gu.nearest_init(x, 3, 7)
    return x, labels, centres


# --------------------------------------------------------------------------------------------------------------------- C ABI
def test_c_abi_declares_and_exports_the_entry_points():
    from ctypes import c_double, c_int, c_long, c_void_p
    from maskedsst_amd import _lib
    header = open(_lib.HEADER_PATH).read()
    assert _lib.header_version() == 109   # additive: the revision does not move
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    P = c_void_p
    sigs = {"msst_gmm_scratch_floats": (c_long, [c_long, c_int]),
            "msst_gmm_posterior": (c_int, [P, c_int, c_long, c_long, c_int, P, P, c_int, P]),
            "msst_gmm_moments": (c_int, [P, c_int, c_long, c_long, c_int, P, c_int, P, P, c_long, P]),
            "msst_gmm_update": (c_int, [P, c_long, c_long, c_int, c_int, c_int, c_double, c_double] + [P] * 9)}
    for name, sig in sigs.items():
        m = re.search(r"^(?:int|long) %s\(([^;]*)\);" % name, header, re.M)
        assert m and len(m.group(1).split(",")) == len(sig[1]), name
        assert name in _lib.declared_symbols() and _lib._SIGS[name] == sig
        assert re.search(r" T %s$" % name, out, re.M)
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == sig
    import maskedsst_amd
    for n in ("GaussianMixture", "MixtureResult", "MixtureScene", "fit_mixture", "mixture_scene"):
        assert n in maskedsst_amd.__all__ and hasattr(maskedsst_amd, n), n
    assert maskedsst_amd.MixtureResult._fields == ("classes", "log_likelihood", "distance", "probs")
    assert maskedsst_amd.MixtureScene._fields == ("classes", "log_likelihood", "distance", "probs", "cover")
    assert hasattr(maskedsst_amd.ViTSpatialSpectral, "mixture_scene")
    build = __import__("maskedsst_amd.build", fromlist=["SOURCES"])
    assert "msst_gmm.hip" in build.SOURCES and "msst_gmm_core.h" in build.HEADERS


def test_scratch_floats_follow_the_partition():
    from maskedsst_amd import _lib
    lib = _lib.load()
    row = 1 + 96 + 96 * 96
    for rows, k, nwg in ((1, 1, 1), (64, 3, 1), (65, 3, 2), (512 * 64, 32, 512), (512 * 64 + 1, 2, 257), (2 ** 31 - 1, 32, 512)):
        assert lib.msst_gmm_scratch_floats(rows, k) == nwg * (k * row + 2), (rows, k)
    for rows, k in ((0, 1), (-1, 1), (2 ** 31, 1), (10, 0), (10, 33)):
        assert lib.msst_gmm_scratch_floats(rows, k) == 0


def _ptr():
    buf = (ctypes.c_char * 1024)()
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)


def test_calls_refuse_bad_arguments_before_launch():
    from maskedsst_amd import _lib
    lib = _lib.load()
    buf, p = _ptr()
    odd = ctypes.c_void_p(p.value + 2)
    big = 1 << 40

    def err():
        return lib.msst_last_error().decode()

    def post(in_layout=0, rows=128, plane=1, k=3, out_layout=0, scores=p, lse=p, probs=p):
        return lib.msst_gmm_posterior(scores, in_layout, rows, plane, k, lse, probs, out_layout, None)

    def mom(x_layout=0, rows=128, plane=1, dim=96, k=3, slab_floats=big, x=p, scores=p, centres=p, slab=p):
        return lib.msst_gmm_moments(x, x_layout, rows, plane, dim, scores, k, centres, slab, slab_floats, None)

    def upd(rows=128, dim=96, k=3, cov=0, reg=1e-6, mc=1.0, slab_floats=big, **ptr):
        a = {n: ptr.get(n, p) for n in ("slab", "centres", "tables", "covs", "logdet", "consts", "weights", "raw", "record")}
        return lib.msst_gmm_update(a["slab"], slab_floats, rows, dim, k, cov, reg, mc, a["centres"], a["tables"], a["covs"], a["logdet"],
                                   a["consts"], a["weights"], a["raw"], a["record"], None)

    for rc in (post(rows=0), post(k=0), mom(rows=0), mom(dim=0), mom(k=0), upd(rows=-1), upd(k=0), upd(cov=2), upd(cov=-1), upd(reg=-1.0),
               upd(reg=float("nan")), upd(mc=-0.5), upd(mc=float("nan"))):
        assert rc == BADARG
    for rc in (post(k=129), post(rows=2 ** 31), mom(dim=95), mom(k=33), mom(rows=2 ** 31), upd(dim=97), upd(k=33)):
        assert rc == UNSUPPORTED
    assert post(in_layout=2) == BADARG and "msst_gmm_posterior" in err()
    assert post(out_layout=-1) == BADARG
    assert post(in_layout=1, plane=5) == BADARG and post(out_layout=1, plane=0) == BADARG
    assert mom(x_layout=3) == BADARG and mom(x_layout=1, plane=7) == BADARG and "msst_gmm_moments" in err()
    for name in ("scores", "lse"):
        assert post(**{name: None}) == BADARG and post(**{name: odd}) == BADARG
    assert post(probs=odd) == BADARG
    for name in ("x", "scores", "centres", "slab"):
        assert mom(**{name: None}) == BADARG and mom(**{name: odd}) == BADARG, name
    assert mom(x=ctypes.c_void_p(p.value + 4)) == BADARG        # rows are read 16 bytes at a time
    for name in ("slab", "centres", "tables", "covs", "logdet", "consts", "weights", "record"):
        assert upd(**{name: None}) == BADARG and upd(**{name: odd}) == BADARG, name
    assert upd(raw=odd) == BADARG and "msst_gmm_update" in err()
    need = lib.msst_gmm_scratch_floats(128, 3)
    assert mom(slab_floats=need - 1) == BADARG and "msst_gmm_scratch_floats" in err()
    assert upd(slab_floats=need - 1) == BADARG and "msst_gmm_scratch_floats" in err()


# ------------------------------------------------------------------------------------------------------- the Python surface
def test_fit_mixture_and_gaussian_mixture_refuse_bad_arguments_without_a_device():
    from maskedsst_amd import GaussianMixture, KMeans, fit_mixture
    x = torch.randn(40, 96)
    for bad in (torch.randn(40, 95), torch.randn(40), torch.randn(40, 96).double(), torch.randn(40, 192)[:, ::2], "x"):
        with pytest.raises(ValueError):
            fit_mixture(bad, k=2)
    for kw in (dict(k=0), dict(k=33), dict(k=41), dict(k=2.0), dict(k=True), dict(covariance="tied"), dict(covariance="spherical"),
               dict(iters=0), dict(iters=1.5), dict(reg_covar=-1e-3), dict(reg_covar=float("nan")), dict(reg_covar="1"), dict(init="random"),
               dict(init=torch.zeros(2, 96)), dict(seed=-1), dict(seed=2 ** 32), dict(min_count=-1.0), dict(check_every=0), dict(tol=-1.0),
               dict(init=KMeans(torch.randn(2, 96).contiguous(), metric="cosine")),
               dict(init=KMeans(torch.randn(3, 96).contiguous(), metric="euclidean"))):
        with pytest.raises(ValueError):
            fit_mixture(x, **{**dict(k=2), **kw})
    with pytest.raises(RuntimeError):
        fit_mixture(x, k=2)                                   # a CPU tensor: no fallback
    eye = np.broadcast_to(np.eye(96), (2, 96, 96)).copy()
    ok = dict(weights=np.array([1.0, 3.0]), means=np.zeros((2, 96)), covariances=eye)
    gm = GaussianMixture(**ok)
    assert gm.k == 2 and gm.weights.tolist() == [0.25, 0.75] and gm.covariance == "full" and gm.history is None and not gm.converged
    with pytest.raises(ValueError):
        fit_mixture(x, k=3, init=gm)
    bad_cov = eye.copy()
    bad_cov[1, 0, 0] = -1.0
    skew = eye.copy()
    skew[0, 1, 0] = 0.1
    for kw in (dict(weights=np.array([1.0, -1.0])), dict(weights=np.zeros(2)), dict(weights=np.ones(3)), dict(means=np.zeros((2, 95))),
               dict(means=np.zeros((2, 96), dtype=np.int64)), dict(covariances=eye[:1]), dict(covariances=bad_cov), dict(covariances=skew),
               dict(means=np.full((2, 96), np.nan)), dict(covariance="tied"), dict(means=np.zeros((129, 96)))):
        with pytest.raises(ValueError):
            GaussianMixture(**{**ok, **kw})
    with pytest.raises(RuntimeError):
        gm.predict(x)


def test_gaussian_mixture_from_arrays_factorises_as_the_restatement(small):
    from maskedsst_amd import GaussianMixture
    x, labels, centres = small
    params, _, _ = gu.fit(x, labels, centres, 3, 1, reg_covar=1e-3)
    for kind in ("full", "diag"):
        gm = GaussianMixture(params["weights"], params["means"], params["covariances"], covariance=kind)
        for c in range(3):
            sigma = params["covariances"][c] if kind == "full" else np.diag(np.diag(params["covariances"][c]))
            a, logdet = gu.factor(sigma)
            assert np.abs(gm.tables[c].numpy() - a).max() <= 1e-6 * np.abs(a).max()
            assert abs(float(gm.logdet[c]) - logdet) <= 1e-6 * abs(logdet)
            assert float(gm.consts[c]) == pytest.approx(np.log(params["weights"][c]) - 0.5 * logdet - gu.LOG_2PI_HALF_DIM, rel=1e-6)
        assert not bool(torch.triu(gm.tables, 1).any())
    gm0 = GaussianMixture(np.array([0.0, 1.0, 1.0]), params["means"], params["covariances"])
    assert float(gm0.consts[0]) == float("-inf") and gm0.weights.tolist() == [0.0, 0.5, 0.5]


# ------------------------------------------------------------------------------------------------------- the restatement itself
def test_restatement_agrees_with_scikit_learn(small):
    mixture = pytest.importorskip("sklearn.mixture")
    from sklearn.mixture._gaussian_mixture import _compute_precision_cholesky, _estimate_gaussian_parameters
    x, labels, centres = small
    x64 = x.astype(np.float64)
    rng = np.random.default_rng(3)
    resp = rng.dirichlet(np.full(3, 0.3), size=len(x))
    scores = np.log(resp)
    for kind in ("full", "diag"):
        want_n, want_mu, want_cov = _estimate_gaussian_parameters(x64, resp, 1e-3, kind)
        new, rec, (N, s1, s2) = gu.m_step(x, scores, gu.start_params(3, centres), kind, 1e-3)
        assert np.allclose(N, want_n, rtol=1e-12) and np.allclose(new["means"], want_mu, rtol=0, atol=1e-11)
        got = new["covariances"] if kind == "full" else np.diagonal(new["covariances"], axis1=1, axis2=2)
        assert np.abs(got - want_cov).max() <= 1e-11 * np.abs(want_cov).max()
        assert np.allclose(new["weights"], want_n / want_n.sum(), rtol=1e-12)
        sk = mixture.GaussianMixture(n_components=3, covariance_type=kind)
        sk.weights_, sk.means_, sk.covariances_ = new["weights"], new["means"], want_cov
        sk.precisions_cholesky_ = _compute_precision_cholesky(want_cov, kind)
        s, _ = gu.scores_of(x, new)
        lse, probs = gu.posterior(s)
        assert np.abs(lse - sk.score_samples(x64)).max() <= 1e-9
        assert np.abs(probs - sk.predict_proba(x64)).max() <= 1e-9
        assert np.array_equal(gu.classes_of(s), sk.predict(x64))
        total = float(lse.sum())
        assert gu.bic(total, len(x), 3, kind) == pytest.approx(sk.bic(x64), rel=1e-12)


def test_log_likelihood_never_falls(small):
    x, labels, centres = small
    for kind in ("full", "diag"):
        _, history, _ = gu.fit(x, labels, centres, 3, 8, kind, reg_covar=1e-3)
        assert np.all(np.diff(history[:, 0]) >= -1e-10), history[:, 0]
        assert np.all(history[:, 1] == len(x)) and not history[:, 2:].any()


def test_cholesky_route_agrees_with_slogdet_and_solve(small):
    x, labels, centres = small
    params, _, _ = gu.fit(x, labels, centres, 3, 1, reg_covar=1e-3)
    s, d2 = gu.scores_of(x, params)
    for c in range(3):
        sign, logdet = np.linalg.slogdet(params["covariances"][c])
        assert sign == 1.0 and abs(params["logdet"][c] - logdet) <= 1e-10 * abs(logdet)
        d = x.astype(np.float64) - params["means"][c]
        want = (d * np.linalg.solve(params["covariances"][c], d.T).T).sum(axis=1)
        assert np.abs(d2[:, c] - want).max() <= 1e-9 * want.max()
    assert gu.factor(-np.eye(96)) is None


def test_posterior_edge_rows():
    s = np.array([[0.0, -np.inf, -np.inf], [-np.inf] * 3, [np.nan, 0.0, 0.0], [-5000.0, -5000.0, -5001.0], [1.0, 1.0, 0.0]])
    lse, p = gu.posterior(s)
    assert lse[0] == 0.0 and p[0].tolist() == [1.0, 0.0, 0.0]
    assert lse[1] == -np.inf and p[1].tolist() == [0.0, 0.0, 0.0]
    assert np.isnan(lse[2]) and np.isnan(p[2]).all()
    assert lse[3] == pytest.approx(-5000.0 + np.log(2.0 + np.exp(-1.0))) and p[3].sum() == pytest.approx(1.0)
    assert gu.classes_of(s).tolist() == [0, 0, -1, 0, 0]


# ------------------------------------------------------------------------------------------------------- the bars catch the mutants
@pytest.fixture(scope="module")
def forced():
    """what the GPU suite's teacher-forced M-steps see, with float64 scores in the device's place: case A's rows, (i) a hard
    assignment about nearest-row centres (a large delta), (ii) the scores of the parameters that step gives (soft, delta small)"""
    x, _, _ = gu.planted("A")
    labels, centres = gu.nearest_init(x, 3, 5)
    start = gu.start_params(3, centres)
    hard = gu.hard_scores(labels, 3)
    first, _, _ = gu.m_step(x, hard, start, "full", gu.TEST_REG_COVAR)
    soft, _ = gu.scores_of(x, first)
    return x, start, hard, first, soft


def _worst(errors, bars):
    """the largest error / bar over the quantities of an M-step"""
    return max(errors[name] / bars[name] for name in errors)


@pytest.mark.parametrize("mutant", ["no_reg", "no_delta", "ddof", "weights_raw", "logdet_sign", "logdet_half"])
def test_m_step_bars_catch(mutant, forced):
    x, start, hard, first, soft = forced
    bars = gu.bars()
    caught = False
    for scores, old in ((hard, start), (soft, first)):
        want, _, _ = gu.m_step(x, scores, old, "full", gu.TEST_REG_COVAR)
        got, _, _ = gu.m_step(x, scores, old, "full", gu.TEST_REG_COVAR, mutant=mutant)
        assert _worst(gu.m_step_errors(want, want), bars) < 1e-6      # the restatement itself is far inside the bars
        caught |= _worst(gu.m_step_errors(got, want), bars) > 1.0
    assert caught


def test_diag_bars_catch_kept_off_diagonals(forced):
    x, start, hard, first, soft = forced
    want, _, _ = gu.m_step(x, hard, start, "diag", gu.TEST_REG_COVAR)
    got, _, _ = gu.m_step(x, hard, start, "diag", gu.TEST_REG_COVAR, mutant="diag_keeps")
    assert not np.triu(want["covariances"], 1).any()
    assert _worst(gu.m_step_errors(got, want), gu.bars()) > 1.0


def test_exact_checks_catch_the_counting_mutants(forced):
    x, start, hard, first, soft = forced
    xn = x.copy()
    xn[5] = np.nan
    _, rec, raw = gu.m_step(xn, hard, start)
    _, rec_m, raw_m = gu.m_step(xn, hard, start, mutant="nan_counted")
    assert rec[1] == len(x) - 1 and rec_m[1] == len(x) and not np.array_equal(raw[0], raw_m[0])
    # a starved component: kept bit for bit, against zeroed
    empty = hard.copy()
    empty[hard[:, 2] == 0.0] = [0.0, -np.inf, -np.inf]
    kept, rec, _ = gu.m_step(x, empty, first)
    zeroed, _, _ = gu.m_step(x, empty, first, mutant="starved_zeroed")
    assert rec[2] == 1 and kept["weights"][2] == 0.0 and kept["consts"][2] == -np.inf
    assert np.array_equal(kept["means"][2], first["means"][2]) and np.array_equal(kept["tables"][2], first["tables"][2])
    assert kept["logdet"][2] == first["logdet"][2] and not np.array_equal(zeroed["means"][2], first["means"][2])
    # ties: two equal maxima go to the lower index
    s = np.array([[1.0, 3.0, 3.0], [2.0, 2.0, 2.0]])
    assert gu.classes_of(s).tolist() == [1, 0] and gu.classes_of(s, mutant="ties_high").tolist() == [2, 2]


def test_posterior_bars_catch_the_missing_max():
    s = np.array([[-5000.0, -5003.0, -4999.5], [-5000.0, -np.inf, -5000.0]])
    lse, p = gu.posterior(s)
    bad, _ = gu.posterior(s, mutant="lse_nomax")
    bars = gu.bars()
    assert np.isfinite(lse).all() and not (np.abs(bad - lse) / (1.0 + np.abs(lse)) <= bars["lse"]).all()


def test_real_cases_leave_few_rows_under_the_margin():
    """the fit tests skip the class of a row whose float64 top-two margin is under 4 x the measured score error: at most 1 % of the
    rows of cases A and B at every iteration, from float64 alone"""
    gap = 4.0 * gu.worst_measured()["scores"]
    for case in ("A", "B"):
        x, _, _ = gu.planted(case)
        K = gu.CASES[case]["K"]
        labels, centres = gu.nearest_init(x, K, 5)
        _, _, trace = gu.fit(x, labels, centres, K, gu.FIT_ITERS, reg_covar=gu.TEST_REG_COVAR)
        for s in trace:
            top = np.sort(s, axis=1)
            assert ((top[:, -1] - top[:, -2]) < gap).mean() <= 0.01
