"""The float64 restatement of maskedsst_amd/pca.py and maskedsst_amd/csrc/msst_pca.hip in numpy -- moments, finish, the sign and rank
rules, transform and Mahalanobis -- the fp32 / rule mutations that the committed bars must tell apart from it, the cases of
tests/test_gpu_pca.py and tests/test_pca_host.py, and the bars (4 x the errors measured on the MI355X,
profiles/pca_parity_measured.jsonl).  Nothing here needs a GPU."""
import functools
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 96
PARITY_FILE = os.path.join(ROOT, "profiles", "pca_parity_measured.jsonl")
MUTANTS = ["one_pass_fp32", "ddof0", "nan_counted", "no_correction", "mean_not_subtracted", "whiten_by_lambda", "ascending"]

INT_ROWS = [1, 63, 64, 65, 127, 321, 32833]      # 32833 = 513 tiles + 1: two tiles per workgroup
INT_MAPS = [(3, 5, 7), (3, 40, 44)]              # (Bs, Hs, Ws): planes 35 and 1760, no multiple of 64
NAN_KINDS = ["none", "ends", "tile", "all"]      # no NaN row; the first and the last row; rows 64 .. 127 (a whole tile); every row
REAL_ROWS = [3000, 32833]
REAL_FORMS = ["well", "offset"]
REAL_NAN_ROWS = 7                                # rows of a real-valued case that carry a NaN channel (the counting rule)
PROJECT_R = [1, 3, 15, 16, 17, 64, 96]
FIT_QUANTITIES = ("mean", "cov", "eigenvalues", "evr", "effective_rank")
PROJECT_ROWS = [(1, 1, 1), (65, 5, 13), (4097, 17, 241)]     # rows = Bs x plane
PROJECT_ROWS_LONG = (32833, 1, 32833)            # above 32 directions a workgroup walks several tiles from 513 tiles on


def project_shapes(r):
    return PROJECT_ROWS + ([PROJECT_ROWS_LONG] if r > 32 else [])


# ------------------------------------------------------------------------------------------------------------------------ cases
def nan_rows(M, kind):
    """the rows of an M-row case that get a NaN channel"""
    if kind == "none":
        return []
    if kind == "ends":
        return sorted({0, M - 1})
    if kind == "tile":
        return list(range(64, min(128, M))) if M > 64 else [M - 1]
    return list(range(M))


def int_case(M, kind="none", seed=0):
    """x [M, 96] float32, whole numbers in [-8, 8]: every raw sum up to 32833 rows is exact in fp32 (8 x 8 x 32833 < 2^24).  NaN rows
    keep their other channels."""
    g = np.random.default_rng(1000 + 7 * M + seed)
    x = g.integers(-8, 9, size=(M, D)).astype(np.float32)
    for i, r in enumerate(nan_rows(M, kind)):
        x[r, (5 * i + 3) % D] = np.nan
    return x


def int_centre():
    """a whole-number centre: x - centre stays exact, and the second pass's residual sum is far from zero"""
    return ((np.arange(D) % 5) - 2).astype(np.float32)


def int_moments(x, centre=None):
    """(n, s1 [96], s2 [96, 96]) of the rows without a NaN, in integers"""
    ok = ~np.isnan(x).any(axis=1)
    c = x[ok].astype(np.int64) - (0 if centre is None else centre.astype(np.int64))
    return int(ok.sum()), c.sum(axis=0), c.T @ c


def finish_exact(n, s1, s2, centre, ddof):
    """msst_feat_moments_finish on whole-number sums, operation by operation in IEEE double and rounded once: (mean, cov) float32"""
    s1, s2 = s1.astype(np.float64), s2.astype(np.float64)
    c = np.zeros(D) if centre is None else centre.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = (c + s1 / np.float64(n)).astype(np.float32)
        if n - ddof <= 0:
            return mean, np.full((D, D), np.nan, dtype=np.float32)
        cov = ((s2 - s1[:, None] * s1[None, :] / np.float64(n)) / np.float64(n - ddof)).astype(np.float32)
    return mean, cov


@functools.lru_cache(maxsize=None)
def _mixing():
    g = np.random.default_rng(77)
    q, _ = np.linalg.qr(g.standard_normal((D, D)))
    return q * np.exp(-np.arange(D) / 24.0)[None, :]      # x = z A^T: covariance Q diag(exp(-j / 12)) Q^T, condition number e^7.9 = 2.7e3


@functools.lru_cache(maxsize=None)
def _real_case(M, form):
    g = np.random.default_rng(500 + M)
    x = g.standard_normal((M, D)) @ _mixing().T
    x -= x.mean(axis=0)
    if form == "offset":
        x += 50.0
    x = x.astype(np.float32)
    for i in range(REAL_NAN_ROWS):
        x[(i * 431 + 17) % M, (11 * i) % D] = np.nan
    x.setflags(write=False)
    return x


def real_case(M, form):
    """x [M, 96] float32 (read-only, shared): unit-scale rows mixed to a condition number of 3e3, zero mean ("well") or 50 in every
    channel ("offset"), REAL_NAN_ROWS rows with a NaN channel"""
    assert form in REAL_FORMS
    return _real_case(M, form)


def case_name(M, form):
    return f"fit_{form}_{M}"


@functools.lru_cache(maxsize=None)
def project_tables(r):
    """(mean [96] float32, components [r, 96] float32): a given mean near 50 and random orthonormal rows from a float64 QR"""
    g = np.random.default_rng(900 + r)
    q, _ = np.linalg.qr(g.standard_normal((D, r)))
    mean = (50.0 + 0.25 * g.standard_normal(D)).astype(np.float32)
    return mean, np.ascontiguousarray(q.T).astype(np.float32)


@functools.lru_cache(maxsize=None)
def project_rows(M):
    """x [M, 96] float32: the offset form, one row with a NaN channel where there is more than one row"""
    g = np.random.default_rng(300 + M)
    x = (g.standard_normal((M, D)) @ _mixing().T + 50.0).astype(np.float32)
    if M > 1:
        x[M // 2, 9] = np.nan
    x.setflags(write=False)
    return x


def to_map(x, Bs, plane):
    """rows [Bs plane, C] -> the map [Bs, C, plane]"""
    return np.ascontiguousarray(x.reshape(Bs, plane, x.shape[1]).transpose(0, 2, 1))


def from_map(m):
    """the map [Bs, C, plane] -> rows [Bs plane, C]"""
    return np.ascontiguousarray(m.transpose(0, 2, 1).reshape(-1, m.shape[1]))


# ------------------------------------------------------------------------------------------------------------------ restatement
def ulp_up(v):
    """fp32 values moved one ulp away from zero"""
    v = np.asarray(v, dtype=np.float32)
    return np.nextafter(v, np.where(v >= 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))


def moments64(x, centre=None, count_nan=False):
    """(n, s1, s2) of x - centre in float64; rows with a channel that is not finite are zeroed and not counted"""
    ok = np.isfinite(x).all(axis=1)
    c = x[ok].astype(np.float64) - (0.0 if centre is None else np.asarray(centre, dtype=np.float64))
    return int(len(x) if count_nan else ok.sum()), c.sum(axis=0), c.T @ c


def finish64(n, s1, s2, centre, ddof, correction=True):
    c = np.zeros(D) if centre is None else np.asarray(centre, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = c + s1 / n
        if n - ddof <= 0:
            return mean, np.full((D, D), np.nan)
        return mean, (s2 - (np.outer(s1, s1) / n if correction else 0.0)) / (n - ddof)


def covariance64(x, ddof=1, mutant=None):
    """(count, mean, cov): the centred two-pass covariance in float64, or one of its mutations"""
    assert mutant in (None, "one_pass_fp32", "ddof0", "nan_counted", "no_correction")
    if mutant == "one_pass_fp32":       # the textbook form, every operation in fp32
        ok = np.isfinite(x).all(axis=1)
        xf = x[ok].astype(np.float32)
        n = np.float32(len(xf))
        mu = xf.sum(axis=0, dtype=np.float32) / n
        s2 = xf.T @ xf
        cov = (s2 - n * np.outer(mu, mu).astype(np.float32)) / np.float32(len(xf) - ddof)
        return len(xf), mu.astype(np.float64), cov.astype(np.float64)
    if mutant == "ddof0":
        ddof = 0
    counted = mutant == "nan_counted"
    n, s1, s2 = moments64(x, None, counted)
    mean1, _ = finish64(n, s1, s2, None, ddof)
    centre = mean1.astype(np.float32)                  # what the first finish hands the second pass
    if mutant == "no_correction":
        centre = ulp_up(centre)                        # ... so that the residual sum is not zero
    n, s1, s2 = moments64(x, centre, counted)
    mean, cov = finish64(n, s1, s2, centre, ddof, correction=mutant != "no_correction")
    return n, mean, cov


def eigen64(cov, ascending=False):
    """(eigenvalues descending, clamped at 0; components [96, 96] as rows, the entry of largest magnitude positive, ties to the lowest
    index)"""
    w, v = np.linalg.eigh(np.asarray(cov, dtype=np.float64))
    if not ascending:
        w, v = w[::-1], v[:, ::-1]
    v = v.T
    big = np.argmax(np.abs(v), axis=1)
    sign = np.where(v[np.arange(len(v)), big] < 0, -1.0, 1.0)
    return np.maximum(w, 0.0), v * sign[:, None]


def rank64(lam, rcond=1e-6):
    return int((lam > rcond * lam.max()).sum()) if lam.max() > 0 else 0


def spectrum64(lam):
    """(explained_variance_ratio, effective_rank)"""
    p = lam / lam.sum()
    q = p[p > 0]
    return p, float(np.exp(-(q * np.log(q)).sum()))


def fit64(x, ddof=1, rcond=1e-6, mutant=None):
    cov_mutant = mutant if mutant in ("one_pass_fp32", "ddof0", "nan_counted", "no_correction") else None
    n, mean, cov = covariance64(x, ddof, cov_mutant)
    lam, comp = eigen64(cov, ascending=mutant == "ascending")
    evr, erank = spectrum64(lam)
    return dict(count=n, mean=mean, cov=cov, eigenvalues=lam, components=comp, evr=evr, effective_rank=erank, rank=rank64(lam, rcond))


def project64(x, mean, comp, mutant=None):
    """(out [Q, r], sumsq [Q]) in float64; a row with a channel that is not finite gets NaN"""
    assert mutant in (None, "mean_not_subtracted")
    c = x.astype(np.float64) - (0.0 if mutant == "mean_not_subtracted" else np.asarray(mean, dtype=np.float64))
    bad = ~np.isfinite(x).all(axis=1)
    c[bad] = 0.0
    out = c @ np.asarray(comp, dtype=np.float64).T
    out[bad] = np.nan
    return out, (out * out).sum(axis=1)


def whiten64(fit, mutant=None):
    """the components of the `rank` leading directions divided by sqrt(lambda)"""
    assert mutant in (None, "whiten_by_lambda")
    m = fit["rank"]
    lam = fit["eigenvalues"][:m]
    return fit["components"][:m] / (lam if mutant == "whiten_by_lambda" else np.sqrt(lam))[:, None]


def mahalanobis64(x, fit, mutant=None):
    return project64(x, fit["mean"], whiten64(fit, mutant))[1]


# ------------------------------------------------------------------------------------------------------------------------- bars
def relmax(got, ref):
    """max abs error over max abs value of the float64 array; NaN positions must coincide and are left out"""
    got, ref = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(ref, dtype=np.float64).reshape(-1)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), "NaN positions differ"
    if nan.all():
        return 0.0
    return float(np.abs(got[~nan] - ref[~nan]).max() / max(np.abs(ref[~nan]).max(), 1e-300))


def fit_errors(got, ref):
    """the error of every compared quantity of a fit (dicts as from fit64)"""
    return {q: relmax(got[q], ref[q]) for q in FIT_QUANTITIES}


@functools.lru_cache(maxsize=None)
def measured():
    out = {}
    if os.path.exists(PARITY_FILE):
        with open(PARITY_FILE) as f:
            for line in f:
                if line.strip():
                    row = json.loads(line)
                    out[row["case"]] = row["measured"]
    return out


def bars(case):
    """4 x the committed measurement per quantity (the project's convention)"""
    m = measured().get(case)
    assert m, f"no committed measurement for {case} in {PARITY_FILE}"
    return {k: 4.0 * val for k, val in m.items()}


def note(case, err):
    """MSST_RECORD_DIR=<directory>: append a case's measured errors to pca_parity_dev.jsonl there, BEFORE the bars are asserted (the
    committed file is made from these rows); ordinary test runs write nothing"""
    d = os.environ.get("MSST_RECORD_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "pca_parity_dev.jsonl"), "a") as f:
            f.write(json.dumps(dict(case=case, measured=err)) + "\n")


def within(err, bar):
    """[(quantity, error, bar)] of the errors above their bar"""
    return [(k, e, bar[k]) for k, e in err.items() if not e <= bar[k]]
