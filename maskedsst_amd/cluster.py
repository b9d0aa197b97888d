"""k-means clustering of frozen per-pixel features: the label-free use of the encoder -- the ``encode_scene`` map of an unlabelled scene
clustered into a land-cover segmentation -- and, where some labels exist, the clustering score (Hungarian-matched accuracy, purity,
NMI), the fourth standard protocol beside nearest class mean (finetune.py --val-embed), weighted kNN (maskedsst_amd.knn) and the
linear probe (maskedsst_amd.probe).

    km = fit_kmeans(features, k=16, iters=50, metric="cosine", init="kmeans++", seed=0)   # KMeans; km.history [iters, 4] (CPU)
    labels, dist = km.assign(features)                                  # [Q] int64 (-1 for a NaN row), [Q] float32
    res = model.cluster_scene(scene, km)                                # ClusterScene(classes, distance, cover)
    m = match_clusters(contingency(labels, truth, k, n_classes))        # ClusterMatch(mapping, accuracy, purity, nmi)

Three calls of ``libmsst.so`` (``maskedsst_amd/csrc/msst_kmeans.hip``, ``include/msst.h``).  A Lloyd iteration is two launches:
``msst_kmeans_assign`` streams the rows once -- one score per centroid on the fp32 matrix cores, the argmax under ONE total order
(score descending, then cluster index ascending), and the per-cluster sums of every workgroup as one more matrix product -- and
``msst_kmeans_update`` sums the partials in a fixed order and writes the new centroids.  A fit enqueues its ``2 * iters`` launches
and synchronises once, to read the history.  The k-means++ seeding is ``msst_kmeans_assign`` against the centres chosen so far and
one ``msst_kmeans_pick`` per new centre, its random numbers a stateless counter hash of (seed, centre).  No atomics: two fits from
the same inputs give the same bits, and an iteration that moves no row reproduces itself bit for bit.  There is no CPU or eager
fallback.
"""
import ctypes
import math
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .features import DIM, KnnBank, _is_int, _p, _stream, _require_cuda, check_rows, on_scene_map

MAX_K = 128        # include/msst.h: msst_kmeans_assign
METRICS = {"cosine": 0, "euclidean": 1}     # include/msst.h: MSST_KMEANS_COSINE, MSST_KMEANS_EUCLIDEAN
HISTORY = ("inertia", "moved", "empty", "shift")   # the columns of KMeans.history

# classes [Bs, Hs, Ws] int64 (-1 where no window covers the pixel), distance [Bs, Hs, Ws] fp32 (NaN there), cover [Bs, Hs, Ws] int32
ClusterScene = namedtuple("ClusterScene", ["classes", "distance", "cover"])
# mapping [k] (the class matched to every cluster, -1 for a cluster left without one), accuracy, purity, nmi
ClusterMatch = namedtuple("ClusterMatch", ["mapping", "accuracy", "purity", "nmi"])


def _bias(centroids, metric):
    if metric == "cosine":
        return torch.zeros(centroids.shape[0], dtype=torch.float32, device=centroids.device)
    return (-0.5 * (centroids * centroids).sum(dim=1)).contiguous()


class KMeans:
    """A fitted (or given) clustering: centroids [k, 96] fp32 on the device (unit length for metric "cosine"), bias [k] (0, or
    -0.5 |c|^2 for "euclidean"), counts [k] int64 (the cluster sizes of the last iteration; None before a fit), history [iters, 4] on
    the CPU -- per iteration the inertia (the sum of the rows' distances to their clusters, against the centroids the iteration
    started from), the number of rows whose assignment changed, the number of empty clusters and the largest centroid displacement
    (L2) -- and seed_rows [k] int64 (the rows the initial centres were copied from; None for a tensor init)."""

    def __init__(self, centroids, metric="cosine", bias=None, counts=None, history=None, seed_rows=None, seed=None, counts_history=None):
        if metric not in METRICS:
            raise ValueError(f"metric must be one of {sorted(METRICS)}, got {metric!r}")
        if not torch.is_tensor(centroids) or centroids.dim() != 2 or centroids.shape[1] != DIM or centroids.dtype != torch.float32 \
                or not centroids.is_contiguous() or not 1 <= centroids.shape[0] <= MAX_K:
            raise ValueError(f"centroids must be a contiguous float32 tensor [k, {DIM}] with 1 <= k <= {MAX_K}, "
                             f"got {getattr(centroids, 'shape', type(centroids))}")
        self.centroids = centroids
        self.metric = metric
        self.bias = _bias(centroids, metric) if bias is None else bias
        self.counts = counts
        self.history = history
        self.seed_rows = seed_rows
        self.seed = seed
        self.counts_history = counts_history      # [iters, k] int64 on the CPU: the cluster sizes of every iteration

    @property
    def k(self):
        return self.centroids.shape[0]

    @property
    def inertia(self):
        """the last iteration's inertia (NaN before a fit)"""
        return float(self.history[-1, 0]) if self.history is not None and len(self.history) else float("nan")

    def assign(self, features):
        """(labels [Q] int64, distance [Q] fp32) of rows [Q, 96] (fp32, contiguous, on the device): the cluster of the largest score,
        ties to the lowest index, and max(0, 2 (1 - s)) (cosine) or max(0, |x|^2 - 2 s) (euclidean); a row with a NaN channel gets
        -1 and NaN.  A row has the same bits whatever batch it sits in."""
        check_rows(features, "features", 1, few="features needs at least one row")
        _require_cuda(features, "features")
        _require_cuda(self.centroids, "the centroids")
        Q = features.shape[0]
        labels = torch.empty(Q, dtype=torch.int64, device=features.device)
        dist = torch.empty(Q, dtype=torch.float32, device=features.device)
        kmeans_assign(self, features, 0, Q, 1, labels, dist)
        return labels, dist


def kmeans_assign(km, x, x_layout, rows, plane, classes, dist, assign=None):
    """msst_kmeans_assign (no slab: assignment only) on the current stream: x is rows [rows, 96] (x_layout 0) or a map
    [Bs, 96, plane] (x_layout 1) read in place; classes (int64) and dist are written in flat row order.  Returns assign (int32)."""
    lib = _lib.load()
    assign = torch.empty(rows, dtype=torch.int32, device=x.device) if assign is None else assign
    _lib.check(lib.msst_kmeans_assign(_p(x), x_layout, rows, plane, DIM, _p(km.centroids), _p(km.bias), km.k, METRICS[km.metric],
                                      _p(assign), _p(dist), _p(classes), None, 0, _stream()), "msst_kmeans_assign")
    return assign


def _check_fit(features, k, iters, metric, init, seed, n_init, check_every):
    x = features.features if isinstance(features, KnnBank) else features
    check_rows(x, "features", 1, few="features needs at least one row")
    if not _is_int(k) or not 1 <= k <= MAX_K:
        raise ValueError(f"k must be an integer in [1, {MAX_K}], got {k!r}")
    if not _is_int(iters) or iters < 1:
        raise ValueError(f"iters must be an integer >= 1, got {iters!r}")
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {sorted(METRICS)}, got {metric!r}")
    if x.shape[0] < k:
        raise ValueError(f"k = {k} clusters need at least {k} rows, got {x.shape[0]}")
    if not _is_int(seed) or not 0 <= seed < 2 ** 32:
        raise ValueError(f"seed must be an integer in [0, 2^32), got {seed!r}")
    if not _is_int(n_init) or n_init < 1 or seed + n_init > 2 ** 32:
        raise ValueError(f"n_init must be an integer >= 1 (seed + n_init <= 2^32), got {n_init!r}")
    if check_every is not None and (not _is_int(check_every) or check_every < 1):
        raise ValueError(f"check_every must be None or an integer >= 1, got {check_every!r}")
    if torch.is_tensor(init):
        if init.shape != (k, DIM) or init.dtype != torch.float32:
            raise ValueError(f"init must be 'kmeans++', 'sample' or a float32 tensor [{k}, {DIM}], got {tuple(init.shape)} of {init.dtype}")
        c = init.detach().cpu().double()
        if not bool(torch.isfinite(c).all()):
            raise ValueError("init must be finite")
        if metric == "cosine" and bool((c.norm(dim=1) == 0).any()):
            raise ValueError("init has a zero row: it cannot be normalised for metric 'cosine'")
    elif init not in ("kmeans++", "sample"):
        raise ValueError(f"init must be 'kmeans++', 'sample' or a float32 tensor [{k}, {DIM}], got {init!r}")
    return x


def _unit_rows(c):
    n = c.norm(dim=1, keepdim=True)
    return torch.where(n > 0, c / n, c).contiguous()


def _fit_once(x, k, iters, metric, init, seed, check_every):
    lib = _lib.load()
    dev = x.device
    M = x.shape[0]
    mid = METRICS[metric]
    st = _stream()
    nslab = int(lib.msst_kmeans_scratch_floats(M, k))
    slab = torch.empty(nslab, dtype=torch.float32, device=dev)
    assign = torch.full((M,), -1, dtype=torch.int32, device=dev)
    dist = torch.empty(M, dtype=torch.float32, device=dev)
    seed_rows = None
    if torch.is_tensor(init):
        cent = init.detach().to(dev).clone().contiguous()
        cent = _unit_rows(cent) if metric == "cosine" else cent
        bias = _bias(cent, metric)
    elif init == "sample":
        rows = torch.randperm(M, generator=torch.Generator().manual_seed(seed))[:k]
        seed_rows = rows.clone()
        cent = x[rows.to(dev)].contiguous()
        cent = _unit_rows(cent) if metric == "cosine" else cent
        bias = _bias(cent, metric)
    else:
        cent = torch.empty(k, DIM, dtype=torch.float32, device=dev)
        bias = torch.empty(k, dtype=torch.float32, device=dev)
        table = torch.full((k,), -1, dtype=torch.int32, device=dev)
        for j in range(k):
            if j > 0:
                _lib.check(lib.msst_kmeans_assign(_p(x), 0, M, 1, DIM, _p(cent), _p(bias), j, mid, _p(assign), _p(dist), None, _p(slab), nslab,
                                                  st), "msst_kmeans_assign")
            _lib.check(lib.msst_kmeans_pick(_p(x), M, DIM, _p(dist), _p(slab), nslab, j, k, mid, seed, _p(cent), _p(bias), _p(table), st),
                       "msst_kmeans_pick")
        assign.fill_(-1)      # the first iteration counts every row as moved, whatever the init
        seed_rows = table
    rec = torch.full((iters, record_width(k)), float("nan"), dtype=torch.float32, device=dev)
    done = iters
    for t in range(iters):
        lloyd_iteration(x, cent, bias, metric, assign, dist, slab, rec[t])
        if check_every is not None and (t + 1) % check_every == 0 and t + 1 < iters and float(rec[t, 1]) == 0.0:
            done = t + 1      # a fixed point: every later iteration would repeat this one bit for bit
            break
    rec = rec.cpu()           # the fit's one synchronisation (check_every: one more per check)
    if done < iters:
        rec[done:] = rec[done - 1]
    history, counts = read_records(rec, k)
    if seed_rows is not None:
        seed_rows = seed_rows.cpu().long()
    return KMeans(cent, metric, bias, counts[-1].to(dev), history, seed_rows, seed, counts)


def record_width(k):
    """floats of one iteration's record: inertia, moved | counts k (int32 bits) | shift k"""
    return 2 + 2 * k


def lloyd_iteration(x, centroids, bias, metric, assign, dist, slab, record):
    """One Lloyd iteration on the current stream, two launches and no synchronisation: msst_kmeans_assign in fit mode (x [M, 96];
    assign [M] int32 holds the previous assignment and takes the new one, dist [M] the distances, slab the workgroups' partials:
    msst_kmeans_scratch_floats(M, k) floats) and msst_kmeans_update (centroids [k, 96] and bias [k] are updated in place; record, a
    contiguous fp32 row of record_width(k), takes what read_records unpacks)."""
    lib = _lib.load()
    M, k, mid, st = x.shape[0], centroids.shape[0], METRICS[metric], _stream()
    row = record.data_ptr()
    _lib.check(lib.msst_kmeans_assign(_p(x), 0, M, 1, DIM, _p(centroids), _p(bias), k, mid, _p(assign), _p(dist), None, _p(slab), slab.numel(),
                                      st), "msst_kmeans_assign")
    _lib.check(lib.msst_kmeans_update(_p(slab), slab.numel(), M, DIM, k, mid, _p(centroids), _p(bias), ctypes.c_void_p(row + 8),
                                      ctypes.c_void_p(row + 8 + 4 * k), ctypes.c_void_p(row), st), "msst_kmeans_update")


def read_records(rec, k):
    """records [iters, record_width(k)] on the CPU -> (history [iters, 4]: inertia, moved, empty clusters, the largest centroid
    displacement; counts [iters, k] int64)"""
    counts = rec[:, 2:2 + k].contiguous().view(torch.int32).long()
    history = torch.stack([rec[:, 0], rec[:, 1], (counts == 0).sum(dim=1).float(), rec[:, 2 + k:].max(dim=1).values], dim=1)
    return history, counts


def fit_kmeans(features, k=16, iters=50, metric="cosine", init="kmeans++", seed=0, n_init=1, check_every=None):
    """Lloyd's k-means on frozen features.  Returns a KMeans.
      features     a contiguous fp32 tensor [M, 96] on the device, checked finite once (one read-back), or a KnnBank (checked when
                   it was built).  For metric "cosine" the rows should be unit length (encode_scene(normalize=True), feature_bank).
      metric       "cosine": unit centroids, update sum / |sum|, distance 2 (1 - x . c).  "euclidean": update sum / count, distance
                   |x - c|^2.  A cluster without rows (or a cosine sum of norm 0) keeps its centroid.
      init         "kmeans++": D^2 sampling on the device, the random numbers a stateless hash of (seed, centre): the same on every
                   machine.  "sample": k distinct rows drawn with a CPU torch.Generator seeded with `seed`.  A tensor [k, 96]:
                   normalised for cosine; a zero row raises ValueError.
      iters        every fit runs exactly this many iterations: 2 * iters launches and ONE synchronisation, the read-back of the
                   history.  An iteration that moves no row is a fixed point that the later ones reproduce bit for bit.
      check_every  n: the last history row is read every n iterations and the fit stops at moved == 0; the result (history
                   included) has the bits of the full run.
      n_init       > 1: the fit is repeated with seeds seed, seed + 1, ... and the lowest final inertia is kept (on equal inertia
                   the lowest seed).
    ValueError, before any device work, for a wrong rank, width, dtype, k, metric, init, iters, seed, or M < k; RuntimeError for CPU
    tensors.  No CPU or eager fallback."""
    x = _check_fit(features, k, iters, metric, init, seed, n_init, check_every)
    _require_cuda(x, "features")
    if not isinstance(features, KnnBank) and not bool(torch.isfinite(x).all()):
        raise ValueError("features must be finite (drop the uncovered pixels of encode_scene: cover == 0)")
    best = None
    for s in range(seed, seed + n_init):
        km = _fit_once(x, k, iters, metric, init, s, check_every)
        if best is None or km.inertia < best.inertia:
            best = km
    return best


def cluster_scene(model, scene, km, stride=None, max_windows=None):
    """See ViTSpatialSpectral.cluster_scene."""
    if not isinstance(km, KMeans):
        raise ValueError(f"km must be a KMeans, got {type(km).__name__}")

    def launch(emb, Bs, Hs, Ws):
        _require_cuda(km.centroids, "the centroids")
        dev = emb.features.device
        classes = torch.empty(Bs, Hs, Ws, dtype=torch.int64, device=dev)
        dist = torch.empty(Bs, Hs, Ws, dtype=torch.float32, device=dev)
        kmeans_assign(km, emb.features, 1, Bs * Hs * Ws, Hs * Ws, classes, dist)
        return ClusterScene(classes, dist, emb.cover)

    return on_scene_map(model, scene, stride, km.metric == "cosine", max_windows, launch)


def contingency(labels, truth, k, n_classes, ignored_label=-1):
    """table [k, n_classes] int64 (on the device of `labels`): table[c, y] = the number of elements with cluster c and true class y.
    labels and truth are integer tensors of one shape; an element counts when its cluster lies in [0, k) (-1: a NaN row, an uncovered
    pixel) and its truth is not ignored_label and lies in [0, n_classes)."""
    if not torch.is_tensor(labels) or not torch.is_tensor(truth) or labels.shape != truth.shape:
        raise ValueError("labels and truth must be tensors of one shape")
    if labels.dtype.is_floating_point or truth.dtype.is_floating_point or labels.dtype == torch.bool or truth.dtype == torch.bool:
        raise ValueError(f"labels and truth must be integers, got {labels.dtype} and {truth.dtype}")
    if not _is_int(k) or k < 1 or not _is_int(n_classes) or n_classes < 1:
        raise ValueError(f"k and n_classes must be integers >= 1, got {k!r} and {n_classes!r}")
    lab = labels.reshape(-1).long()
    tru = truth.reshape(-1).long().to(lab.device)
    ok = (lab >= 0) & (lab < k) & (tru != ignored_label) & (tru >= 0) & (tru < n_classes)
    return torch.bincount(lab[ok] * n_classes + tru[ok], minlength=k * n_classes).view(k, n_classes)


def _hungarian_min(cost):
    """row -> column of the minimum-cost perfect matching of a square matrix (the O(n^3) potentials form of the Hungarian method);
    whole-number costs stay exact in float64"""
    n = cost.shape[0]
    u, v = np.zeros(n + 1), np.zeros(n + 1)
    p, way = np.zeros(n + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
    for i in range(1, n + 1):
        p[0] = i
        j0 = 0
        minv = np.full(n + 1, np.inf)
        used = np.zeros(n + 1, dtype=bool)
        while True:
            used[j0] = True
            i0 = p[j0]
            cur = cost[i0 - 1] - u[i0] - v[1:]
            better = ~used[1:] & (cur < minv[1:])
            minv[1:][better] = cur[better]
            way[1:][better] = j0
            cand = np.where(used[1:], np.inf, minv[1:])
            j1 = int(np.argmin(cand)) + 1
            delta = cand[j1 - 1]
            u[p[used]] += delta
            v[used] -= delta
            minv[~used] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    out = np.zeros(n, dtype=np.int64)
    out[p[1:] - 1] = np.arange(n)
    return out


def match_clusters(table):
    """Score a clustering against true classes from its contingency table [k, n_classes] (a tensor, an array or nested lists of counts
    >= 0), on the host: ClusterMatch(mapping, accuracy, purity, nmi).
      mapping   [k] int64: the ONE-TO-ONE assignment of clusters to classes that maximises the matched count (the Hungarian method on
                the table padded square with zeros); -1 for a cluster matched to padding (k > n_classes).
      accuracy  the matched count over the table's total: the clustering accuracy.
      purity    every cluster mapped to its largest class (many-to-one) over the total.
      nmi       the mutual information of the two labelings over the arithmetic mean of their entropies; 1 when both entropies are 0.
    All three are NaN for an empty table."""
    t = np.asarray(table.detach().cpu().numpy() if torch.is_tensor(table) else table)
    if t.ndim != 2 or t.shape[0] < 1 or t.shape[1] < 1 or not np.issubdtype(t.dtype, np.number) or t.dtype == bool:
        raise ValueError(f"table must be a 2-D array [k, n_classes] of counts, got shape {t.shape} of {t.dtype}")
    t = t.astype(np.float64)
    if not np.isfinite(t).all() or (t < 0).any():
        raise ValueError("table must hold finite counts >= 0")
    k, nc = t.shape
    n = max(k, nc)
    sq = np.zeros((n, n))
    sq[:k, :nc] = t
    col = _hungarian_min(sq.max() - sq)[:k]
    mapping = np.where(col < nc, col, -1)
    total = t.sum()
    if total == 0:
        nan = float("nan")
        return ClusterMatch(torch.from_numpy(mapping), nan, nan, nan)
    matched = sum(t[c, mapping[c]] for c in range(k) if mapping[c] >= 0)
    pu, pv = t.sum(axis=1) / total, t.sum(axis=0) / total
    hu = -sum(x * math.log(x) for x in pu if x > 0)
    hv = -sum(x * math.log(x) for x in pv if x > 0)
    mi = 0.0
    for c in range(k):
        for y in range(nc):
            if t[c, y] > 0:
                pxy = t[c, y] / total
                mi += pxy * math.log(pxy / (pu[c] * pv[y]))
    nmi = 1.0 if hu + hv == 0 else max(0.0, 2.0 * mi / (hu + hv))
    return ClusterMatch(torch.from_numpy(mapping), float(matched / total), float(t.max(axis=1).sum() / total), float(nmi))
