"""A float64 numpy restatement of the contract of maskedsst_amd.mixture (the module docstring; include/msst.h): the posterior, one
M-step, a fit from a given hard assignment, BIC -- and the planted mixtures and the measured bars that tests/test_gmm_host.py and
tests/test_gpu_gmm.py share.  Nothing here imports the code under test.

Every function that a mutant can break takes `mutant`, one of MUTANTS or None: tests/test_gmm_host.py proves on the CPU that the bars
of the GPU suite still catch each of them.
"""
import json
import math
import os

import numpy as np

DIM = 96
LOG_2PI_HALF_DIM = 0.5 * DIM * math.log(2.0 * math.pi)
MUTANTS = ("no_reg", "no_delta", "ddof", "weights_raw", "lse_nomax", "logdet_sign", "logdet_half", "nan_counted", "starved_zeroed",
           "ties_high", "diag_keeps")

# What the MI355X measured against this restatement (tools/gmm_parity.py writes the file; the README quotes it).  The bar of a test is
# 4 x the measured value: the margin every suite of this line uses.
PARITY_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "gmm_parity_measured.jsonl")


FLOOR = 2.0 ** -23            # no bar sits under one fp32 rounding step: a measured 0 must not turn a later half-ulp into a failure
TEST_REG_COVAR = 1e-3         # the reg_covar of the real-valued cases: large enough that a dropped one is far over the bars
FIT_ITERS = 8                 # the iterations of the teacher-forced fits


def measured():
    """{case: {quantity: error}} from profiles/gmm_parity_measured.jsonl"""
    assert os.path.exists(PARITY_PATH), "profiles/gmm_parity_measured.jsonl is not committed: nothing to hold the device or the mutants against"
    out = {}
    with open(PARITY_PATH) as f:
        for line in f:
            if line.strip():
                row = json.loads(line)
                out[row["case"]] = row["measured"]
    return out


def committed(case):
    """whether the parity file holds a measurement of this case (a measuring run meets cases that are new to the file)"""
    return os.path.exists(PARITY_PATH) and case in measured()


def worst_measured():
    """{quantity: the largest error any case measured}"""
    worst = {}
    for m in measured().values():
        for name, v in m.items():
            worst[name] = max(worst.get(name, 0.0), float(v))
    return worst


def bars(case=None):
    """4 x the committed measurement per quantity (the project's convention), of one case or of the worst case"""
    m = worst_measured() if case is None else measured().get(case)
    assert m, f"no committed measurement for {case} in {PARITY_PATH}"
    return {name: max(4.0 * v, FLOOR) for name, v in m.items()}


def check(case, err):
    """print a case's measured errors, record them where MSST_RECORD_DIR names a directory (gmm_parity_dev.jsonl there, BEFORE anything
    is asserted), then assert the committed bars"""
    print(f"{case}: {err}")
    d = os.environ.get("MSST_RECORD_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "gmm_parity_dev.jsonl"), "a") as f:
            f.write(json.dumps(dict(case=case, measured=err)) + "\n")
        if not committed(case):
            return                                 # a measuring run records a case that is new to the file
    bar = bars(case)
    for name, v in err.items():
        assert v <= bar[name], f"{case}: {name} = {v} over the bar {bar[name]}"


# ---- the contract
def posterior(scores, mutant=None):
    """(lse [Q], probs [Q, K]) of scores [Q, K] float64: NaN for a row with a NaN score; lse = -inf and probs 0 where every score is -inf"""
    s = np.asarray(scores, dtype=np.float64)
    bad = np.isnan(s).any(axis=1)
    m = np.where(bad, 0.0, np.max(np.where(np.isnan(s), -np.inf, s), axis=1))
    dead = ~bad & np.isneginf(m)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if mutant == "lse_nomax":
            lse = np.log(np.exp(s).sum(axis=1))
        else:
            mm = np.where(dead, 0.0, m)
            lse = mm + np.log(np.exp(s - mm[:, None]).sum(axis=1))
        lse = np.where(dead, -np.inf, lse)
        probs = np.where(dead[:, None], 0.0, np.exp(s - np.where(dead, 0.0, lse)[:, None]))
    lse = np.where(bad, np.nan, lse)
    probs = np.where(bad[:, None], np.nan, probs)
    return lse, probs


def classes_of(scores, mutant=None):
    """the argmax under the total order (score descending, then index ascending); -1 for a row with a NaN score"""
    s = np.asarray(scores, dtype=np.float64)
    bad = np.isnan(s).any(axis=1)
    t = np.where(np.isnan(s), -np.inf, s)
    if mutant == "ties_high":
        c = t.shape[1] - 1 - np.argmax(t[:, ::-1], axis=1)
    else:
        c = np.argmax(t, axis=1)
    return np.where(bad, -1, c)


def factor(sigma, mutant=None):
    """(A = L^-1 lower triangular, logdet = 2 sum log L[i][i]) of Sigma = L L^T; None where the factorisation fails"""
    try:
        L = np.linalg.cholesky(sigma)
    except np.linalg.LinAlgError:
        return None
    if not np.isfinite(L).all():
        return None
    logdet = 2.0 * np.log(np.diag(L)).sum()
    if mutant == "logdet_sign":
        logdet = -logdet
    if mutant == "logdet_half":
        logdet = 0.5 * logdet
    return np.tril(np.linalg.solve(L, np.eye(sigma.shape[0]))), logdet


def scores_of(x, params):
    """(scores [Q, K], d2 [Q, K]) float64 of rows x under params (weights, means, tables, logdet); a row with a channel that is not
    finite gets NaN"""
    x = np.asarray(x, dtype=np.float64)
    K = len(params["weights"])
    d2 = np.empty((x.shape[0], K))
    for c in range(K):
        z = (x - params["means"][c].astype(np.float64)) @ params["tables"][c].astype(np.float64).T
        d2[:, c] = (z * z).sum(axis=1)
    with np.errstate(divide="ignore"):
        s = np.log(params["weights"].astype(np.float64))[None] - 0.5 * (d2 + params["logdet"].astype(np.float64)[None]) - LOG_2PI_HALF_DIM
    bad = ~np.isfinite(x).all(axis=1)
    s[bad] = np.nan
    d2[bad] = np.nan
    return s, d2


def m_step(x, scores, old, covariance="full", reg_covar=1e-6, min_count=1.0, mutant=None):
    """One M-step in float64 from given scores [Q, K] about the current means old["means"].  old: weights, means, covariances, tables,
    logdet (any float dtype).  Returns (new, record, raw): new the same five float64 arrays plus consts; record = (mean lse per counted
    row, counted rows, starved, failed); raw = (N [K], s1 [K, 96], s2 [K, 96, 96]) about the old means."""
    x = np.asarray(x, dtype=np.float64)
    K = scores.shape[1]
    lse, r = posterior(scores, mutant)
    counted = np.isfinite(x).all(axis=1) & np.isfinite(lse)
    if mutant == "nan_counted":
        counted = np.isfinite(lse)
    xs = np.where(counted[:, None], x, 0.0) if mutant != "nan_counted" else np.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0)
    r = np.where(counted[:, None], r, 0.0)
    new = {name: np.array(old[name], dtype=np.float64) for name in ("weights", "means", "covariances", "tables", "logdet")}
    N = r.sum(axis=0)
    s1 = np.zeros((K, DIM))
    s2 = np.zeros((K, DIM, DIM))
    starved = failed = 0
    total = N.sum()
    for c in range(K):
        cen = np.asarray(old["means"][c], dtype=np.float64)
        d = (xs - cen) * counted[:, None]
        s1[c] = (r[:, c:c + 1] * d).sum(axis=0)
        s2[c] = (r[:, c:c + 1] * d).T @ d
        new["weights"][c] = N[c] if mutant == "weights_raw" else (N[c] / total if total > 0 else 0.0)
        if not N[c] >= min_count:
            starved += 1
            if mutant == "starved_zeroed":
                new["means"][c] = 0.0
                new["tables"][c] = 0.0
                new["logdet"][c] = 0.0
            continue
        delta = s1[c] / N[c]
        sigma = s2[c] / ((N[c] - 1.0) if mutant == "ddof" else N[c])
        if mutant != "no_delta":
            sigma = sigma - np.outer(delta, delta)
        if mutant != "no_reg":
            sigma = sigma + reg_covar * np.eye(DIM)
        if covariance == "diag" and mutant != "diag_keeps":
            sigma = np.diag(np.diag(sigma))
        sigma = 0.5 * (sigma + sigma.T)
        f = factor(sigma, mutant)
        if f is None:
            failed += 1
            continue
        new["means"][c] = cen + delta
        new["covariances"][c] = sigma
        new["tables"][c], new["logdet"][c] = f
    with np.errstate(divide="ignore"):
        new["consts"] = np.log(new["weights"]) - 0.5 * new["logdet"] - LOG_2PI_HALF_DIM
    n = int(counted.sum())
    record = (float(lse[counted].sum() / n) if n else float("nan"), n, starved, failed)
    return new, record, (N, s1, s2)


def start_params(K, centres):
    """what a fit holds before its first M-step: unit covariances about the given centres"""
    eye = np.broadcast_to(np.eye(DIM), (K, DIM, DIM)).copy()
    return dict(weights=np.full(K, 1.0 / K), means=np.array(centres, dtype=np.float64), covariances=eye, tables=eye.copy(), logdet=np.zeros(K))


def hard_scores(labels, K):
    """the scores buffer of a hard assignment: 0 for the row's cluster, -inf elsewhere"""
    s = np.full((len(labels), K), -np.inf)
    s[np.arange(len(labels)), labels] = 0.0
    return s


def fit(x, labels, centres, K, iters, covariance="full", reg_covar=1e-6, min_count=1.0, mutant=None):
    """A float64 EM from a hard assignment: the init M-step about `centres`, then `iters` iterations.  Returns (params, history
    [iters, 4], per iteration the scores it started from)."""
    params, _, _ = m_step(x, hard_scores(labels, K), start_params(K, centres), covariance, reg_covar, min_count, mutant)
    history, trace = [], []
    for _ in range(iters):
        s, _ = scores_of(x, params)
        trace.append(s)
        params, rec, _ = m_step(x, s, params, covariance, reg_covar, min_count, mutant)
        history.append(rec)
    return params, np.array(history, dtype=np.float64), trace


def n_parameters(K, covariance):
    return K * DIM + K * (DIM * (DIM + 1) // 2 if covariance == "full" else DIM) + K - 1


def bic(total_log_likelihood, n, K, covariance):
    return -2.0 * total_log_likelihood + n_parameters(K, covariance) * math.log(n)


# ---- the planted mixtures of the teacher-forced tests
CASES = {"A": dict(K=3, sep=0.3, offset=0.0, rows=3000, seed=11),
         "B": dict(K=4, sep=0.15, offset=50.0, rows=3000, seed=12),
         "C": dict(K=16, sep=0.3, offset=0.0, rows=4161, seed=13)}
CONDITION = 300.0


def planted(case):
    """(x [rows, 96] float32, truth [rows], means [K, 96]) of a planted mixture: component means offset + sep N(0, 1), covariances
    randomly rotated with eigenvalues log-spaced from 1 down to 1 / 300, equal weights"""
    spec = CASES[case]
    rng = np.random.default_rng(spec["seed"])
    K, rows = spec["K"], spec["rows"]
    means = spec["offset"] + spec["sep"] * rng.standard_normal((K, DIM))
    lam = CONDITION ** (-np.arange(DIM) / (DIM - 1.0))
    truth = rng.integers(0, K, rows)
    x = np.empty((rows, DIM))
    for c in range(K):
        q, _ = np.linalg.qr(rng.standard_normal((DIM, DIM)))
        sel = truth == c
        x[sel] = means[c] + (rng.standard_normal((int(sel.sum()), DIM)) * np.sqrt(lam)) @ q.T
    return x.astype(np.float32), truth, means


def nearest_init(x, K, seed):
    """(labels, centres): K distinct random rows as centres and every row with its nearest one -- a deterministic init for the CPU runs"""
    rng = np.random.default_rng(seed)
    centres = np.asarray(x, dtype=np.float64)[rng.choice(len(x), K, replace=False)]
    d = ((np.asarray(x, dtype=np.float64)[:, None, :] - centres[None]) ** 2).sum(axis=2)
    return np.argmin(d, axis=1), centres


# ---- how the GPU suite measures a device M-step against this restatement (the same function serves the mutants on the CPU)
def m_step_errors(got, want):
    """{quantity: error} of a device M-step `got` against the float64 `want` (dicts of weights, means, covariances, tables, logdet)"""
    g = {k: np.asarray(v, dtype=np.float64) for k, v in got.items()}
    out = {"weights": float(np.abs(g["weights"] - want["weights"]).max()),
           "means": float((np.abs(g["means"] - want["means"]) / (1.0 + np.abs(want["means"]))).max()),
           "logdet": float((np.abs(g["logdet"] - want["logdet"]) / (1.0 + np.abs(want["logdet"]))).max())}
    cov = whiten = 0.0
    for c in range(len(want["weights"])):
        cov = max(cov, float(np.abs(g["covariances"][c] - want["covariances"][c]).max() / np.abs(want["covariances"][c]).max()))
        a = g["tables"][c]
        whiten = max(whiten, float(np.abs(a @ want["covariances"][c] @ a.T - np.eye(DIM)).max()))
    out["covariances"] = cov
    out["tables"] = whiten
    return out
