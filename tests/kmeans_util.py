"""k-means: the float64 restatement of msst_kmeans_assign / msst_kmeans_update / msst_kmeans_pick (maskedsst_amd/csrc/msst_kmeans.hip)
with the same rules -- one total order (score descending, cluster index ascending), a NaN row out of every sum, an empty cluster
keeps its centroid, the D^2 draw from the stateless hash of (seed, centre) -- written so that each rule can be mutated, the numpy
restatement of the hash, the case generators of tests/test_gpu_kmeans.py and the committed bars (4 x the errors measured on the
MI355X, profiles/kmeans_parity_measured.jsonl).  Nothing here needs a GPU."""
import functools
import json
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 96
PARITY_FILE = os.path.join(ROOT, "profiles", "kmeans_parity_measured.jsonl")
MUTANTS = ["ties_to_highest", "no_bias", "mean_without_normalisation", "empty_zeroed", "sum_not_divided", "prefix_off_by_one"]
EXCLUDED_SHARE = 0.01       # at most this share of a case's rows may have a float64 margin below the case's gap

INT_M = [1, 63, 64, 65, 127, 321]                 # 127: one tile short of two workgroups; 321: several workgroups + 1
INT_K = [1, 2, 15, 16, 17, 128]
# ... and 32833 = 513 tiles + 1: two tiles per workgroup (the accumulation across tiles and the prefetch), at two cluster counts
INT_SHAPES = [(M, k) for M in INT_M for k in INT_K] + [(32833, 16), (32833, 128)]
PARITY_CASES = [(metric, k) for metric in ("cosine", "euclidean") for k in (3, 16, 128)]
PARITY_M = 3000
TRAJ_CASES = [("cosine", 5, 900), ("euclidean", 16, 2000)]
TRAJ_ITERS = 20
TRAJ_SEED = {("cosine", 5): 62, ("euclidean", 16): 32}     # seeds chosen so that the float64 run moves rows for several iterations with every margin above 1e-3


# ------------------------------------------------------------------------------------------------------------------------ the hash
def _mix(x):
    x = (x * 0x9E3779B1) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def km_hash(seed, j):
    """the counter hash of (seed, centre j): two rounds of the finaliser of msst_mask.hip"""
    return _mix(_mix((int(seed) ^ 0x6B6D2B2B) & 0xFFFFFFFF) ^ int(j))


def km_hash_np(seed, j):
    """the same on numpy uint64 arrays (masked to 32 bits)"""
    def mix(x):
        x = (x * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
        x ^= x >> np.uint64(15)
        x = (x * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
        x ^= x >> np.uint64(13)
        x = (x * np.uint64(0xC2B2AE35)) & np.uint64(0xFFFFFFFF)
        x ^= x >> np.uint64(16)
        return x
    seed, j = np.asarray(seed, dtype=np.uint64), np.asarray(j, dtype=np.uint64)
    return mix(mix((seed ^ np.uint64(0x6B6D2B2B)) & np.uint64(0xFFFFFFFF)) ^ j)


def draw_u(seed, j):
    return (km_hash(seed, j) >> 8) * 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------- the restatement
def bias64(cent, metric, mutant=None):
    if metric == "cosine" or mutant == "no_bias":
        return torch.zeros(cent.shape[0], dtype=torch.float64)
    return -0.5 * (cent.double() ** 2).sum(dim=1)


def assign64(x, cent, metric, mutant=None):
    """-> dict(labels [M] int64 (-1: a row with a NaN channel), dist [M] (NaN there), score [M] (the best), margin [M] (best minus
    second best; inf for k = 1), bad [M])"""
    x, cent = x.double(), cent.double()
    bad = torch.isnan(x).any(dim=1)
    xs = torch.where(bad.unsqueeze(1), torch.zeros_like(x), x)
    s = xs @ cent.t() + bias64(cent, metric, mutant)
    k = cent.shape[0]
    if mutant == "ties_to_highest":
        labels = k - 1 - s.flip(1).argmax(dim=1)
    else:
        best = s.max(dim=1, keepdim=True).values
        labels = (s == best).double().argmax(dim=1)          # the lowest index among the equal best
    top = s.gather(1, labels.unsqueeze(1)).squeeze(1)
    if k > 1:
        rest = s.clone()
        rest.scatter_(1, labels.unsqueeze(1), float("-inf"))
        margin = top - rest.max(dim=1).values
    else:
        margin = torch.full_like(top, float("inf"))
    dist = 2.0 * (1.0 - top) if metric == "cosine" else (xs ** 2).sum(dim=1) - 2.0 * top
    dist = dist.clamp_min(0.0)
    nan = torch.full_like(dist, float("nan"))
    return dict(labels=torch.where(bad, torch.full_like(labels, -1), labels), dist=torch.where(bad, nan, dist),
                score=torch.where(bad, nan, top), margin=torch.where(bad, nan, margin), bad=bad)


def update64(x, labels, cent, metric, mutant=None):
    """-> dict(centroids [k, 96], counts [k] int64, sums [k, 96], shift (the largest displacement), empty)"""
    x, cent = x.double(), cent.double()
    k = cent.shape[0]
    ok = labels >= 0
    sums = torch.zeros(k, D, dtype=torch.float64).index_add_(0, labels[ok], x[ok])
    counts = torch.bincount(labels[ok], minlength=k)
    new = cent.clone()
    for c in range(k):
        if counts[c] == 0:
            if mutant == "empty_zeroed":
                new[c] = 0.0
            continue
        if mutant == "sum_not_divided":
            new[c] = sums[c]
        elif metric == "cosine" and mutant != "mean_without_normalisation":
            n = sums[c].norm()
            if n > 0:
                new[c] = sums[c] / n
        else:
            new[c] = sums[c] / counts[c]
    return dict(centroids=new, counts=counts, sums=sums, shift=float((new - cent).norm(dim=1).max()), empty=int((counts == 0).sum()))


def step64(x, cent, metric, prev=None, mutant=None):
    """one Lloyd iteration, teacher forced from `cent`: assign64 + update64 + the history entries"""
    a = assign64(x, cent, metric, mutant)
    u = update64(x, a["labels"], cent, metric, mutant)
    prev = torch.full_like(a["labels"], -1) if prev is None else prev
    out = dict(a)
    out.update(u)
    out["inertia"] = float(a["dist"][~a["bad"]].sum())
    out["moved"] = int((a["labels"] != prev).sum())
    return out


def unit(c):
    n = c.norm(dim=1, keepdim=True)
    return torch.where(n > 0, c / n, c)


def pick64(x, dist, chosen, seed, j, mutant=None):
    """centre j of the k-means++ seeding -> the row.  dist: the distances to the nearest of the centres chosen so far (unused for j = 0);
    rows chosen before count 0.  The inclusive prefix sums run in row order (workgroup blocks of consecutive rows first, then rows, is
    the same order)."""
    M = x.shape[0]
    h = km_hash(seed, j)
    if j == 0:
        return ((h >> 8) * M) >> 24
    d = dist.double().clone()
    d[torch.isnan(d)] = 0.0
    d[list(chosen)] = 0.0
    total = float(d.sum())
    if total == 0:
        return min(r for r in range(M) if r not in set(chosen))
    t = (h >> 8) * 2.0 ** -24 * total
    over = torch.nonzero(torch.cumsum(d, 0) > t).reshape(-1)
    row = int(over[0]) if len(over) else int(torch.nonzero(d > 0).reshape(-1)[-1])
    if mutant == "prefix_off_by_one":
        row = min(row + 1, M - 1)
    return row


def seed64(x, k, metric, seed, mutant=None):
    """the whole k-means++ seeding -> (rows [k], centroids [k, 96] float64, the largest distance total met)"""
    rows, largest = [], 0.0
    for j in range(k):
        dist = None
        if j > 0:
            cent = x[rows].double()
            dist = assign64(x, unit(cent) if metric == "cosine" else cent, metric)["dist"]
            largest = max(largest, float(dist[~torch.isnan(dist)].sum()))
        rows.append(pick64(x, dist, rows, seed, j, mutant))
    cent = x[rows].double()
    return rows, (unit(cent) if metric == "cosine" else cent), largest


def fit64(x, cent, metric, iters, mutant=None):
    """`iters` Lloyd iterations from `cent` -> dict(labels [iters, M], counts [iters, k], history [iters, 4], centroids, min_margin)"""
    cent = unit(cent.double()) if metric == "cosine" else cent.double()
    prev, labels, counts, hist, min_margin = None, [], [], [], float("inf")
    for _ in range(iters):
        s = step64(x, cent, metric, prev, mutant)
        labels.append(s["labels"])
        counts.append(s["counts"])
        hist.append([s["inertia"], float(s["moved"]), float(s["empty"]), s["shift"]])
        m = s["margin"][~s["bad"]]
        min_margin = min(min_margin, float(m.min())) if len(m) else min_margin
        prev, cent = s["labels"], s["centroids"]
    return dict(labels=torch.stack(labels), counts=torch.stack(counts), history=torch.tensor(hist, dtype=torch.float64), centroids=cent,
                min_margin=min_margin)


# ------------------------------------------------------------------------------------------------------------------- the cases
def int_case(M, k, seed=0):
    """integer data in [-8, 8]: every dot product, sum and prefix sum is exact in fp32.  Duplicated centroids and rows (the tie rule
    decides: the later copy of a duplicated centroid stays empty), a NaN row where M allows.  -> (x [M, 96] fp32, centroids
    [k, 96] fp32)"""
    g = torch.Generator().manual_seed(1000 * k + M % 1000 + seed)
    cent = torch.randint(-8, 9, (k, D), generator=g).float()
    if k >= 2:
        cent[k - 1] = cent[0]                       # a duplicate: every row of centroid 0 ties with the last one
    if k >= 15:
        cent[7] = cent[3]
    which = torch.randint(0, k, (M,), generator=g)
    x = (cent[which] + torch.randint(-1, 2, (M, D), generator=g)).clamp(-8, 8)
    if M >= 3:
        x[M // 2] = x[0]                            # duplicated rows
    if M >= 8:
        x[3, 17] = float("nan")
    if M >= 70:
        x[66] = float("nan")
    return x.contiguous(), cent.contiguous()


def blob_case(metric, k, M=PARITY_M, seed=0, spread=0.35, uniform_share=0.1):
    """Gaussian blobs around k centres plus uniform rows, raw (euclidean) or unit-normalised (cosine), and teacher-forcing centroids:
    the blob centres, perturbed.  -> (x [M, 96] fp32, centroids [k, 96] fp32)"""
    g = torch.Generator().manual_seed(7000 + 10 * k + (1 if metric == "cosine" else 0) + seed)
    centres = torch.randn(k, D, generator=g)
    which = torch.randint(0, k, (M,), generator=g)
    x = centres[which] + spread * torch.randn(M, D, generator=g)
    nu = int(uniform_share * M)
    x[:nu] = 4.0 * torch.rand(nu, D, generator=g) - 2.0
    cent = centres + 0.1 * torch.randn(k, D, generator=g)
    if metric == "cosine":
        x, cent = unit(x.double()).float(), unit(cent.double()).float()
    return x.contiguous(), cent.contiguous()


def traj_case(metric, k, M, seed=0):
    """well separated: 4 k TIGHT blobs of unequal sizes and an init of k of their centres, so that Lloyd's iteration moves whole blobs for several
    iterations and a row's margin is set by the geometry of the blob centres, not by the noise inside a blob -> (x, init [k, 96])"""
    g = torch.Generator().manual_seed(9000 + k + TRAJ_SEED.get((metric, k), 0) + seed)
    nb = 4 * k
    centres = torch.randn(nb, D, generator=g)
    which = torch.randint(0, nb, (M,), generator=g) % torch.randint(1, nb + 1, (M,), generator=g)     # low blobs are the large ones
    x = centres[which] + 0.002 * torch.randn(M, D, generator=g)
    if metric == "cosine":
        x = unit(x.double()).float()
    init = centres[torch.randperm(nb, generator=g)[:k]].clone()          # k DISTINCT blobs: no two centroids share one
    return x.contiguous(), init.contiguous()


def group_case(seed=0):
    """three tight point groups A (180 rows), B (70), C (50) at known mutual distances, shuffled -> (x [300, 96], group [300])"""
    g = torch.Generator().manual_seed(4242 + seed)
    centres = torch.zeros(3, D)
    centres[1, 0] = 3.0                 # |A - B| = 3
    centres[2, 1] = 4.0                 # |A - C| = 4, |B - C| = 5
    group = torch.cat([torch.zeros(180), torch.ones(70), torch.full((50,), 2.0)]).long()
    group = group[torch.randperm(300, generator=g)]
    x = centres[group] + 0.01 * torch.randn(300, D, generator=g)
    return x.contiguous(), group


# ------------------------------------------------------------------------------------------------------------------ comparison
def relmax(got, ref):
    """max abs error over max abs value of the float64 tensor; NaN positions must coincide and are left out"""
    got = (got.double() if torch.is_tensor(got) else torch.tensor(got, dtype=torch.float64)).cpu().reshape(-1)     # (a Python float is a double)
    ref = (ref.double() if torch.is_tensor(ref) else torch.tensor(ref, dtype=torch.float64)).cpu().reshape(-1)
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), "NaN positions differ"
    if bool(nan.all()):
        return 0.0
    return float((got[~nan] - ref[~nan]).abs().max() / ref[~nan].abs().max().clamp_min(1e-300))


def step_errors(dist, inertia, centroids, shift, ref):
    """one assign + update against step64 -> {dist, inertia, centroids, shift: largest error over largest value, score: the largest
    ABSOLUTE error of a row's best score, recovered from its distance (dist = const - 2 score)}"""
    d = torch.as_tensor(dist).double().cpu()
    ok = ~torch.isnan(ref["dist"]) & (ref["dist"] > 0) & (d > 0)
    return dict(dist=relmax(d, ref["dist"]), inertia=relmax(inertia, ref["inertia"]), centroids=relmax(centroids, ref["centroids"]),
                shift=relmax(shift, ref["shift"]), score=float((d[ok] - ref["dist"][ok]).abs().max() / 2.0) if bool(ok.any()) else 0.0)


def case_name(metric, k):
    return f"{metric}_k{k}"


# --------------------------------------------------------------------------------------------------------------- committed bars
@functools.lru_cache(maxsize=None)
def measured():
    """{case: {quantity: the largest error measured on the MI355X}} from the committed file; {} without it"""
    out = {}
    if os.path.exists(PARITY_FILE):
        for line in open(PARITY_FILE):
            if line.strip():
                row = json.loads(line)
                out[row["case"]] = row["measured"]
    return out


def bars(case):
    """4 x the committed measurement per quantity (the project's convention); `score` is absolute and is the case's gap"""
    m = measured().get(case)
    assert m, f"no committed measurement for {case} in {PARITY_FILE}"
    return {k: 4.0 * val for k, val in m.items()}


def gap(case):
    return bars(case)["score"]


def note(case, err):
    """MSST_RECORD_DIR=<directory>: append a case's measured errors to kmeans_parity_dev.jsonl there, BEFORE the bars are asserted (the
    committed file is made from these rows); ordinary test runs write nothing"""
    d = os.environ.get("MSST_RECORD_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "kmeans_parity_dev.jsonl"), "a") as f:
            f.write(json.dumps(dict(case=case, measured=err)) + "\n")


def within(err, bar):
    """[(quantity, error, bar)] of the errors above their bar"""
    return [(k, e, bar[k]) for k, e in err.items() if not e <= bar[k]]
