"""The float64 restatement of maskedsst_amd/gaussian.py and maskedsst_amd/csrc/msst_gauss.hip in numpy -- the fit (per-class two-pass
covariances, the pooled covariance, shrinkage, the eigenvalue floor, the constants), the scoring in the table form and from a fit, the
rule mutations that the committed bars must tell apart from it, the cases of tests/test_gpu_gauss.py and tests/test_gauss_host.py,
and the bars (4 x the errors measured on the MI355X, profiles/gauss_parity_measured.jsonl).  Nothing here needs a GPU."""
import functools
import json
import os

import numpy as np

import pca_util as pu

ROOT = pu.ROOT
D = 96
PARITY_FILE = os.path.join(ROOT, "profiles", "gauss_parity_measured.jsonl")
LOG_2PI_HALF_D = 48.0 * np.log(2.0 * np.pi)
MUTANTS = ["no_logdet", "no_prior", "ddof0", "pooled_by_n", "whiten_by_lambda", "centre_not_subtracted", "no_floor", "ties_highest"]
MARGIN_SHARE = 0.01                              # the share of rows a real-valued case may leave under the margin gap

# ---- the exact cases: (rows, nc, form) with form "full" (T = nc, zero offsets), "tied" (T = 1) or "grouped" (T = 2, classes alternate)
INT_NC = [1, 2, 16, 17, 40, 128]
INT_FORMS = ["full", "tied", "grouped"]
INT_ROWS = [1, 63, 64, 65, 321]
# 65601 rows: three tiles a workgroup, two blocks of two tiles, the second ends after one row; 32833 rows: two tiles a workgroup, one
# two-tile block (128 tied walks one tile a block: two blocks).  Every kernel instance <class tiles, offset tiles> sees a second tile:
INT_ROWS_LONG = [(65601, 2, "full"),        # <1, 1>
                 (65601, 17, "grouped"),    # <2, 1>
                 (65601, 17, "tied"),       # <2, 2>
                 (65601, 40, "full"),       # <4, 1>
                 (65601, 40, "tied"),       # <4, 4>
                 (32833, 128, "full"),      # <8, 1>
                 (32833, 128, "tied")]      # <8, 8>
INT_MAPS = [(3, 5, 7), (3, 40, 44)]
NAN_KINDS = pu.NAN_KINDS

# ---- the real-valued cases
REAL_CASES = [(M, nc, form) for form in ("full", "tied") for M in (3000, 32833) for nc in (3, 16, 128)]
REAL_NAN_ROWS = 5
FIT_CASES = [("full", 0.0), ("full", 0.3), ("full", 1.0), ("tied", 0.0), ("tied", 0.3)]
FIT_QUANTITIES = ("means", "covariances", "pooled", "logdet", "priors")


# --------------------------------------------------------------------------------------------------------------- the exact cases
@functools.lru_cache(maxsize=None)
def int_tables(nc, form, duplicate=False, zero_prior=False):
    """dict(centres [T, 96], tables [T, 96, 96], class_table [nc], offsets [nc, 96], consts [nc]) float32 / int32: whole-number centres
    in [-2, 2], A with entries in {-1, 0, 1} and at most 4 non-zeros a row, whole-number offsets in [-3, 3] (zero in the full form),
    constants that are multiples of 0.5.  duplicate: the last class repeats class 0 (the lowest index must win); zero_prior: class 0
    (where there is another) has the constant -inf."""
    g = np.random.default_rng(4000 + 13 * nc + INT_FORMS.index(form))
    T = nc if form == "full" else 1 if form == "tied" else min(2, nc)
    centres = g.integers(-2, 3, size=(T, D)).astype(np.float32)
    tables = np.zeros((T, D, D), dtype=np.float32)
    for t in range(T):
        for j in range(D):
            cols = g.choice(D, size=g.integers(1, 5), replace=False)
            tables[t, j, cols] = g.choice([-1.0, 1.0], size=len(cols))
    class_table = (np.arange(nc) % T).astype(np.int32)
    offsets = np.zeros((nc, D), dtype=np.float32) if form == "full" else g.integers(-3, 4, size=(nc, D)).astype(np.float32)
    consts = (0.5 * g.integers(-40, 41, size=nc)).astype(np.float32)
    if zero_prior and nc > 1:
        consts[0] = -np.inf
    if duplicate and nc > 1:
        k = class_table[0]
        if form == "full":
            centres[nc - 1], tables[nc - 1] = centres[0], tables[0]
        else:
            class_table[nc - 1] = k
        offsets[nc - 1], consts[nc - 1] = offsets[0], consts[0]
    out = dict(centres=centres, tables=tables, class_table=class_table, offsets=offsets, consts=consts)
    for v in out.values():
        v.setflags(write=False)
    return out


def int_rows(M, kind="none"):
    """x [M, 96] float32, whole numbers in [-8, 8], with the NaN rows of the kind (pca_util.int_case)"""
    return pu.int_case(M, kind, seed=3)


def int_reference(x, tab, max_d2=np.inf):
    """(classes int32 [M], distance float32 [M], scores float32 [M, nc]) of the table form on whole numbers, exact: every partial sum in
    any order is asserted to stay below 2^24, so fp32 arithmetic in the kernel's order (or any other) gives these very numbers"""
    bad = ~np.isfinite(x).all(axis=1)
    xi = np.where(bad[:, None], 0, x).astype(np.float64)            # (whole numbers: float64 products and sums are exact)
    nc = len(tab["consts"])
    d2 = np.empty((len(x), nc))
    zs = {}
    for c in range(nc):
        t = int(tab["class_table"][c])
        m = tab["offsets"][c].astype(np.float64)
        if t not in zs:                                              # one projection a table
            cen, a = tab["centres"][t].astype(np.float64), tab["tables"][t].astype(np.float64)
            xc = xi - cen
            assert (np.abs(xc) @ np.abs(a).T).max() < 2 ** 24
            zs[t] = xc @ a.T
        z = zs[t]
        assert ((z * z).sum(axis=1) + (m * m).sum() + 2 * (np.abs(z) * np.abs(m)).sum(axis=1)).max() < 2 ** 24
        d2[:, c] = ((z - m) ** 2).sum(axis=1)
    consts = tab["consts"].astype(np.float64)
    scores = consts[None, :] - 0.5 * d2
    assert np.abs(scores[np.isfinite(scores)]).max(initial=0) < 2 ** 22          # multiples of 0.5 below 2^23: exact in fp32
    classes = np.argmax(scores, axis=1)                                          # (argmax: the lowest index on a tie)
    distance = d2[np.arange(len(x)), classes]
    classes = np.where(distance > max_d2, -2, classes)
    classes = np.where(bad, -1, classes).astype(np.int32)
    scores[bad] = np.nan
    distance = np.where(bad, np.nan, distance)
    return classes, distance.astype(np.float32), scores.astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ the real-valued cases
@functools.lru_cache(maxsize=None)
def _class_model(nc):
    """(means [nc, 96] near 50, covariances [nc, 96, 96], priors [nc]) float64: every class the pca_util mixing (condition number 2.7e3)
    turned by a rotation of its own in four planes and scaled by a factor in [0.5, 2]; the means 50 + 0.1 x a normal vector, many
    Mahalanobis units apart; unequal priors"""
    g = np.random.default_rng(6000 + nc)
    base = pu._mixing()
    means = 50.0 + 0.1 * g.standard_normal((nc, D))
    cov = np.empty((nc, D, D))
    for c in range(nc):
        rot = np.eye(D)
        for _ in range(4):
            i, j = g.choice(D, size=2, replace=False)
            th = g.uniform(0, 2 * np.pi)
            giv = np.eye(D)
            giv[i, i] = giv[j, j] = np.cos(th)
            giv[i, j], giv[j, i] = -np.sin(th), np.sin(th)
            rot = giv @ rot
        a = rot @ base * np.sqrt(g.uniform(0.5, 2.0))
        cov[c] = a @ a.T
        cov[c] = (cov[c] + cov[c].T) / 2
    pr = g.uniform(0.5, 2.0, size=nc)
    return means, cov, pr / pr.sum()


@functools.lru_cache(maxsize=None)
def real_model(nc, form):
    """the given arrays of a real-valued case: dict(means, covariances ([nc, 96, 96], or [96, 96] tied), priors, tied)"""
    means, cov, pr = _class_model(nc)
    return dict(means=means, covariances=cov[0] if form == "tied" else cov, priors=pr, tied=form == "tied")


@functools.lru_cache(maxsize=None)
def real_rows(M, nc, form):
    """(x [M, 96] float32 read-only, labels [M]): rows drawn from the classes of real_model, REAL_NAN_ROWS of them with a NaN channel"""
    model = real_model(nc, form)
    g = np.random.default_rng(7000 + M + nc)
    labels = g.integers(0, nc, size=M)
    x = np.empty((M, D))
    for c in range(nc):
        idx = np.nonzero(labels == c)[0]
        cov = model["covariances"] if model["tied"] else model["covariances"][c]
        w, v = np.linalg.eigh(cov)
        x[idx] = model["means"][c] + (g.standard_normal((len(idx), D)) * np.sqrt(np.maximum(w, 0))) @ v.T
    x = x.astype(np.float32)
    for i in range(REAL_NAN_ROWS):
        x[(i * 577 + 29) % M, (7 * i) % D] = np.nan
    x.setflags(write=False)
    return x, labels


def real_name(M, nc, form):
    return f"score_{form}_{nc}_{M}"


# ------------------------------------------------------------------------------------------------------------------ restatement
def whitening64(sigma, rcond=1e-6, mutant=None):
    """(A [96, 96], logdet): the eigenvectors as rows over the root of the eigenvalues floored at rcond x the largest"""
    lam, comp = pu.eigen64(sigma)
    if lam[0] <= 0:
        raise ValueError("the largest eigenvalue is 0")
    if mutant != "no_floor":
        lam = np.maximum(lam, rcond * lam[0])
    with np.errstate(divide="ignore", invalid="ignore"):
        return comp / (lam if mutant == "whiten_by_lambda" else np.sqrt(lam))[:, None], float(np.log(lam).sum())


def class_moments64(x, labels, nc, ddof=1):
    """(counts, means [nc, 96], cov [nc, 96, 96]) float64: the centred two-pass covariance of every class's rows in the bank's order,
    exactly as pca_util.covariance64 states the kernels' route (NaN where n_c - ddof <= 0; an absent class: zeros)"""
    counts = np.bincount(labels, minlength=nc).astype(np.int64)
    means, cov = np.zeros((nc, D)), np.zeros((nc, D, D))
    for c in range(nc):
        if counts[c]:
            _, means[c], cov[c] = pu.covariance64(x[labels == c], ddof)
    return counts, means, cov


def fit64(x, labels, nc, covariance="full", shrinkage=0.0, priors="empirical", ddof=1, rcond=1e-6, mutant=None):
    """the fit of maskedsst_amd.fit_gaussian in float64, or one of its mutations: dict(counts, means, class_cov, pooled, covariances
    (Sigma_c [nc, 96, 96], or [96, 96] tied), priors, logdet, tied, rcond)"""
    assert mutant in (None, "ddof0", "pooled_by_n")
    use = 0 if mutant == "ddof0" else ddof
    counts, means, cov = class_moments64(x, labels, nc, use)
    w = np.where(counts > use, counts - (0 if mutant == "pooled_by_n" else use), 0).astype(np.float64)
    pooled = sum(w[c] * cov[c] for c in range(nc) if w[c] > 0) / w.sum()
    present = counts > 0
    tied = covariance == "tied"
    if tied:
        sigma = pooled
    else:
        sigma = np.zeros((nc, D, D))
        for c in np.nonzero(present)[0]:
            sigma[c] = pooled if shrinkage == 1 else (1 - shrinkage) * cov[c] + shrinkage * pooled
    if isinstance(priors, str):
        pr = counts.astype(np.float64) if priors == "empirical" else present.astype(np.float64)
    else:
        pr = np.where(present, np.asarray(priors, dtype=np.float64), 0.0)
    pr = pr / pr.sum()
    logdet = np.full(1 if tied else nc, np.nan)
    if tied:
        logdet[0] = whitening64(pooled, rcond)[1]
    else:
        for c in np.nonzero(present)[0]:
            logdet[c] = whitening64(sigma[c], rcond)[1]
    return dict(counts=counts, means=means, class_cov=cov, pooled=pooled, covariances=sigma, priors=pr, logdet=logdet, tied=tied, rcond=rcond)


def score64(x, model, mutant=None, max_d2=np.inf):
    """(classes [M], scores [M, nc], distance [M]) float64 of rows under dict(means, covariances, priors, tied[, rcond]): the contract
    of maskedsst_amd/gaussian.py -- score_c = log prior_c - 0.5 (d2_c + logdet_c) - 48 log(2 pi) -- or one of its mutations.  A class
    with prior 0 scores -inf; a row with a channel that is not finite gets -1 / NaN."""
    assert mutant in (None, "no_logdet", "no_prior", "whiten_by_lambda", "centre_not_subtracted", "no_floor", "ties_highest")
    rcond = model.get("rcond", 1e-6)
    means, pr = np.asarray(model["means"], dtype=np.float64), np.asarray(model["priors"], dtype=np.float64)
    pr = pr / pr.sum()
    nc = len(pr)
    bad = ~np.isfinite(x).all(axis=1)
    x64 = np.where(bad[:, None], 0.0, x).astype(np.float64)
    d2 = np.zeros((len(x), nc))
    scores = np.full((len(x), nc), -np.inf)
    wm = mutant if mutant in ("whiten_by_lambda", "no_floor") else None
    shared = whitening64(model["covariances"], rcond, wm) if model["tied"] else None
    for c in range(nc):
        if pr[c] > 0:
            a, logdet = shared if model["tied"] else whitening64(model["covariances"][c], rcond, wm)
            if model["tied"]:                                            # one product for all classes (float64: nothing is lost)
                if c == np.nonzero(pr > 0)[0][0]:
                    z0 = x64 @ a.T
                z = z0 - (0.0 if mutant == "centre_not_subtracted" else means[c] @ a.T)
            else:
                z = (x64 - (0.0 if mutant == "centre_not_subtracted" else means[c])) @ a.T
            d2[:, c] = (z * z).sum(axis=1)
            scores[:, c] = ((0.0 if mutant == "no_prior" else np.log(pr[c])) - 0.5 * (d2[:, c] + (0.0 if mutant == "no_logdet" else logdet))
                            - LOG_2PI_HALF_D)
    if mutant == "ties_highest":
        classes = nc - 1 - np.argmax(scores[:, ::-1], axis=1)
    else:
        classes = np.argmax(scores, axis=1)                              # (the lowest index on a tie)
    distance = d2[np.arange(len(x)), classes]
    classes = np.where(distance > max_d2, -2, classes)
    classes = np.where(bad, -1, classes)
    scores[bad] = np.nan
    return classes, scores, np.where(bad, np.nan, distance)


@functools.lru_cache(maxsize=None)
def real_reference(M, nc, form):
    """(classes, scores, distance, margin [M]) of a real-valued case in float64: computed once, shared, read-only"""
    x, _ = real_rows(M, nc, form)
    classes, scores, distance = score64(x, real_model(nc, form))
    top = np.sort(scores, axis=1)
    margin = top[:, -1] - top[:, -2] if nc > 1 else np.full(M, np.inf)
    for a in (classes, scores, distance, margin):
        a.setflags(write=False)
    return classes, scores, distance, margin


def under_gap(margin, classes, gap):
    """the share of the scored rows (class >= 0) whose float64 top-two margin lies below the gap"""
    ok = classes >= 0
    return float((margin[ok] < gap).mean())


# ------------------------------------------------------------------------------------------------------------------------- bars
def relmax(got, ref):
    """pca_util.relmax with -inf taken as a value that must coincide (the score of a class with prior 0)"""
    got, ref = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(ref, dtype=np.float64).reshape(-1)
    inf = np.isinf(ref)
    assert np.array_equal(got[inf], ref[inf]) and np.array_equal(np.isinf(got), inf), "infinite positions differ"
    return pu.relmax(got[~inf], ref[~inf])


@functools.lru_cache(maxsize=None)
def measured():
    """the committed measurements by case, or None while the file does not exist (a run then measures and asserts no bar)"""
    if not os.path.exists(PARITY_FILE):
        return None
    out = {}
    with open(PARITY_FILE) as f:
        for line in f:
            if line.strip():
                row = json.loads(line)
                out[row["case"]] = row["measured"]
    return out


def bars(case):
    """4 x the committed measurement per quantity (the project's convention); None while nothing is committed, or -- in a measuring
    run (MSST_RECORD_DIR) only -- nothing for this case"""
    if measured() is None:
        return None
    m = measured().get(case)
    if m is None and os.environ.get("MSST_RECORD_DIR"):
        return None                                  # a measuring run records a case that is new to the file
    assert m, f"no committed measurement for {case} in {PARITY_FILE}"
    return {k: 4.0 * val for k, val in m.items()}


def note(case, err):
    """MSST_RECORD_DIR=<directory>: append a case's measured errors to gauss_parity_dev.jsonl there, BEFORE the bars are asserted"""
    d = os.environ.get("MSST_RECORD_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "gauss_parity_dev.jsonl"), "a") as f:
            f.write(json.dumps(dict(case=case, measured=err)) + "\n")


def check(case, err):
    """record, then assert the committed bars (where there are any)"""
    print(f"{case}: {err}")
    note(case, err)
    bar = bars(case)
    if bar is not None:
        assert set(bar) == set(err), (case, sorted(bar), sorted(err))
        assert pu.within(err, bar) == [], (case, pu.within(err, bar))


# ------------------------------------------------------------------------------------------------------------------- fit cases
@functools.lru_cache(maxsize=None)
def fit_bank(single=False):
    """(x [M, 96] float32, labels [M], nc = 6): rows of five classes of real_model(16) in shuffled order, with unequal counts 700, 450,
    0, 230, 520 (class 2 is empty) and class 5 with 300 rows, or -- single -- ONE row (a tied fit takes it; a full one refuses)"""
    g = np.random.default_rng(8100)
    means, cov, _ = _class_model(16)
    counts = [700, 450, 0, 230, 520, 1 if single else 300]
    xs, ls = [], []
    for c, n in enumerate(counts):
        w, v = np.linalg.eigh(cov[c])
        xs.append(means[c] + (g.standard_normal((n, D)) * np.sqrt(np.maximum(w, 0))) @ v.T)
        ls.append(np.full(n, c))
    x, labels = np.concatenate(xs).astype(np.float32), np.concatenate(ls)
    order = g.permutation(len(x))
    x, labels = np.ascontiguousarray(x[order]), labels[order]
    x.setflags(write=False)
    return x, labels, 6


def fit_name(covariance, shrinkage, single=False):
    return f"fit_{covariance}_s{shrinkage:g}" + ("_single" if single else "")


def fit_errors(got, ref):
    """the error of every compared quantity of a fit (dicts as from fit64; absent classes are left out of logdet)"""
    out = {}
    for q in FIT_QUANTITIES:
        g, r = np.asarray(got[q], dtype=np.float64), np.asarray(ref[q], dtype=np.float64)
        if q == "logdet":
            keep = ~np.isnan(r)
            assert np.array_equal(np.isnan(g), ~keep)
            g, r = g[keep], r[keep]
        out[q] = pu.relmax(g, r)
    return out
