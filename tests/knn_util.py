"""The kNN evaluation restated in numpy float64 (tests/test_knn_host.py checks it on a hand-made case; tests/test_gpu_knn.py holds
the kernels against it), and the two fixtures of the GPU tests."""
import functools

import numpy as np

U = 2.0 ** -24   # unit roundoff of fp32
# seed of the random-feature fixture: one at which no query's two largest float64 votes (temperature 0.07) come closer than 1e-3
# relative at any shape below -- a property of the inputs, found on the CPU with this file alone, which the GPU test asserts
UNIT_SEED = 1

# (M, Q, k, n_classes): both sides of a 64-row tile, fewer bank rows than k, both ends of k and n_classes, a bank of several slices
SHAPES = [(1, 1, 1, 2), (5, 63, 20, 8), (63, 65, 5, 2), (64, 64, 64, 8), (65, 63, 20, 20), (1000, 300, 20, 8), (4097, 300, 20, 128),
          (4097, 130, 64, 8), (4097, 65, 1, 8)]


def sims64(bank, queries):
    """s(q, m) = sum_d q[d] bank[m][d] in float64: [Q, M]"""
    return np.asarray(queries, dtype=np.float64) @ np.asarray(bank, dtype=np.float64).T


def sim_bound(bank, queries):
    """per pair: 97 * 2^-24 * sum_d |q[d] bank[m][d]| -- the bound of a 96-term fp32 fmaf chain with margin, in float64: [Q, M]"""
    return 97 * U * (np.abs(np.asarray(queries, dtype=np.float64)) @ np.abs(np.asarray(bank, dtype=np.float64)).T)


def topk_ref(s64, k):
    """the first k bank rows of every query under the total order (similarity descending, bank index ascending): index [Q, k] int32
    (-1 past the bank's size; every slot for a query whose similarities are NaN) and their float64 similarities (-inf there)"""
    Q, M = s64.shape
    index = np.full((Q, k), -1, dtype=np.int32)
    sim = np.full((Q, k), -np.inf)
    n = min(k, M)
    for q in range(Q):
        if np.isnan(s64[q]).any():
            continue
        order = np.argsort(-s64[q], kind="stable")[:n]
        index[q, :n] = order
        sim[q, :n] = s64[q, order]
    return index, sim


def votes_ref(index, sim, labels, n_classes, temperature):
    """float64 votes [Q, n_classes] of the given neighbours: w_j = exp((s_j - s_1) / temperature) (temperature 0: 1), index -1 skipped"""
    Q, k = index.shape
    votes = np.zeros((Q, n_classes))
    sim = np.asarray(sim, dtype=np.float64)
    for q in range(Q):
        for j in range(k):
            m = index[q, j]
            if m < 0:
                break
            w = np.exp((sim[q, j] - sim[q, 0]) / temperature) if temperature > 0 else 1.0
            votes[q, labels[m]] += w
    return votes


def classes_ref(votes, index):
    """argmax with ties to the lowest class; -1 for a query without neighbours"""
    c = np.argmax(votes, axis=1).astype(np.int64)
    c[index[:, 0] < 0] = -1
    return c


@functools.lru_cache(maxsize=None)
def exact_fixture(M, Q, n_classes):
    """entries from {-2 .. 2} / 4, so that every product and partial sum is exact in fp32 (multiples of 1/16 below 2^24 / 16); bank
    rows M/2 .. M/2 + 6 are copies of row 3 (where the bank has them): ties at every place.  -> bank, queries (fp32), labels (int32)"""
    g = np.random.default_rng(1000003 * M + 1009 * Q + n_classes)
    bank = (g.integers(-2, 3, size=(M, 96)) / 4.0).astype(np.float32)
    queries = (g.integers(-2, 3, size=(Q, 96)) / 4.0).astype(np.float32)
    if M > 3:
        for m in range(M // 2, min(M, M // 2 + 7)):
            bank[m] = bank[3]
    labels = g.integers(0, n_classes, size=M).astype(np.int32)
    for a in (bank, queries, labels):
        a.setflags(write=False)
    return bank, queries, labels


@functools.lru_cache(maxsize=None)
def unit_fixture(M, Q, n_classes, seed=UNIT_SEED):
    """class means N(0, I) plus unit noise, L2-normalised, cast to fp32 -> bank, queries (fp32), labels (int32)"""
    g = np.random.default_rng(seed + 1000003 * M + 1009 * Q + n_classes)
    means = g.standard_normal((n_classes, 96))
    labels = g.integers(0, n_classes, size=M).astype(np.int32)
    qlab = g.integers(0, n_classes, size=Q)
    bank = means[labels] + g.standard_normal((M, 96))
    queries = means[qlab] + g.standard_normal((Q, 96))
    bank = (bank / np.linalg.norm(bank, axis=1, keepdims=True)).astype(np.float32)
    queries = (queries / np.linalg.norm(queries, axis=1, keepdims=True)).astype(np.float32)
    for a in (bank, queries, labels):
        a.setflags(write=False)
    return bank, queries, labels


def check_against_float64(bank, queries, labels, n_classes, k, index, sim, votes_by_t, classes_by_t, what="", assert_gap=True):
    """The rules of the random-feature test on numpy arrays: the returned neighbours (index [Q, k], sim [Q, k] fp32) and, per
    temperature, votes [Q, n_classes] and classes [Q], against float64.  Queries with a NaN channel are expected to come back
    empty.  assert_gap: also assert that no query's two largest votes come closer than 1e-3 relative (a property of the
    unit_fixture at SHAPES; other inputs pass False and are compared wherever the gap exceeds 1e-4).  Returns the measured figures."""
    Q, M = queries.shape[0], bank.shape[0]
    n = min(k, M)
    s64 = sims64(bank, queries)
    b = sim_bound(bank, queries)
    nanq = np.isnan(s64).any(axis=1)
    ref_index, ref_sim = topk_ref(s64, k)
    assert (index[nanq] == -1).all() and np.isneginf(sim[nanq]).all(), what
    assert (index[:, n:] == -1).all() and np.isneginf(sim[:, n:]).all(), what
    left_out, worst_sim, ok_q = 0, 0.0, np.flatnonzero(~nanq)
    for q in ok_q:
        idx = index[q, :n]
        assert ((idx >= 0) & (idx < M)).all(), (what, q)
        assert len(set(idx.tolist())) == n, (what, q, "an index appears twice")
        got = sim[q, :n].astype(np.float64)
        err = np.abs(got - s64[q, idx])
        assert (err <= b[q, idx]).all(), (what, q, float((err - b[q, idx]).max()))
        worst_sim = max(worst_sim, float((err / np.maximum(b[q, idx], 1e-300)).max()))
        # descending in the RETURNED similarities, ties by index
        d = np.diff(got)
        assert (d <= 0).all() and (np.diff(idx)[d == 0] > 0).all(), (what, q)
        tau = 2 * b[q].max()
        kth = ref_sim[q, n - 1]
        assert (s64[q, idx] >= kth - tau).all(), (what, q)
        if n < M:
            rest = np.sort(s64[q])[::-1][n]
            if kth - rest >= tau:
                assert set(idx.tolist()) == set(ref_index[q, :n].tolist()), (what, q)
            else:
                left_out += 1
        else:
            assert set(idx.tolist()) == set(range(M)), (what, q)
    share = left_out / max(1, len(ok_q))
    assert share <= 0.05, (what, share)   # a changed generator cannot hide the set check
    worst_vote, closest = 0.0, np.inf
    for t, votes in votes_by_t.items():
        v64 = votes_ref(index, sim, labels, n_classes, t)
        assert (votes[nanq] == 0).all() and (classes_by_t[t][nanq] == -1).all(), (what, t)
        top = np.maximum(v64.max(axis=1), 1e-300)
        rel = np.abs(votes.astype(np.float64) - v64).max(axis=1) / top
        assert (rel[~nanq] <= 1e-5).all(), (what, t, float(rel[~nanq].max()))
        worst_vote = max(worst_vote, float(rel[~nanq].max(initial=0.0)))
        c64 = classes_ref(v64, index)
        srt = np.sort(v64, axis=1)[:, ::-1]
        gap = (srt[:, 0] - srt[:, 1]) / top
        if t > 0:
            clear = ~nanq & (gap > 1e-4)
            closest = min(closest, float(gap[~nanq].min(initial=np.inf)))
            if assert_gap:   # no query of these shapes sits near a tie
                assert (gap[~nanq] >= 1e-3).all(), (what, t, float(gap[~nanq].min()))
            assert (classes_by_t[t][clear] == c64[clear]).all(), (what, t)
        else:
            # counts: exact in fp32, so the first argmax itself
            assert (votes[~nanq].astype(np.float64) == v64[~nanq]).all(), (what, t)
            assert (classes_by_t[t][~nanq] == c64[~nanq]).all(), (what, t)
    return dict(sim_err_over_bound=worst_sim, vote_rel_err=worst_vote, set_check_left_out=share, closest_vote_gap=closest)
