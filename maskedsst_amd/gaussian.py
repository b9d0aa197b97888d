"""Class-conditional Gaussians on frozen per-pixel features: maximum-likelihood classification, the classic supervised classifier of
hyperspectral remote sensing.  Full covariances give QDA, a tied covariance Fisher LDA, a shrinkage in between Friedman's regularised
discriminant analysis; the distance of a pixel to its predicted class is the open-set score (Lee et al. 2018) that lets a land-cover
map say "none of my classes".

    clf = fit_gaussian(bank, covariance="full", shrinkage=0.0, priors="empirical", ddof=1, rcond=1e-6)   # bank: a KnnBank of RAW features
    clf.means; clf.counts; clf.priors; clf.logdet; clf.covariances; clf.pooled_covariance
    res = clf.classify(features, scores=True, max_distance=None)     # GaussianResult(classes [Q], scores [Q, nc] | None, distance [Q])
    t = clf.threshold(bank, quantile=0.99)                           # a max_distance
    res = model.gaussian_predict_scene(scene, clf)                   # GaussianScene(classes, scores, distance, cover)

The contract:
    d2_c(x)    = |A_c (x - mu_c)|^2, A_c = V_c / sqrt(lambda_c) from Sigma_c = V_c^T diag(lambda_c) V_c with the eigenvalues FLOORED at
                 rcond x the largest (not dropped: every class lives in all 96 dimensions, so the scores of classes are comparable);
    score_c(x) = log prior_c - 0.5 (d2_c(x) + logdet_c) - 48 log(2 pi), logdet_c = sum log lambda_c: the log joint density;
    classes    = the argmax of the score under the project's one total order: score descending, then class index ascending;
    distance   = d2 of the predicted class.
A row with a channel that is not finite (a pixel no window covers) gets class -1, NaN scores and a NaN distance.  With max_distance
given, a row whose distance exceeds it gets class -2; its scores and distance are still written.  A class with no row has a prior of 0,
a score of -inf and is never predicted.

The fit adds no kernel: the bank's rows are sorted by class (a stable sort and one gather), ``feature_moments`` (the centred two-pass
pair of maskedsst_amd.pca) runs on each class's contiguous slice into one stacked buffer, and that buffer is read back once.  (The
class counts, which size those launches, are read first: nc integers.)  Everything after runs in float64 on the host:
pooled = sum_c (n_c - ddof) cov_c / sum_c (n_c - ddof) over the classes with n_c > ddof; Sigma_c = (1 - shrinkage) cov_c + shrinkage
pooled ("tied": pooled for every class); ``eigen_rules`` of maskedsst_amd.pca; A_c and the per-class constant log prior_c - 0.5
logdet_c - 48 log(2 pi) are rounded to fp32 once.

One launch scores rows or a map (``msst_gauss_score``, ``maskedsst_amd/csrc/msst_gauss.hip``) in a table form that serves both
covariance kinds: full -- one table (mu_c, A_c) per present class and a zero offset; tied -- one table (the pooled mean, A) and per
class the offset m_c = A (mu_c - centre), computed here in float64.  A table id outside the range is refused by the C entry point, on
the host copy it is given.  No atomics: a row has the same bits whatever batch or layout it sits in, with or without the scores.
There is no CPU or eager fallback.
"""
import ctypes
import math
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .features import DIM, MAX_CLASSES, KnnBank, _is_int, _p, _stream, _require_cuda, on_scene_map
from .pca import _source, eigen_rules, feature_moments

# classes [Q] int64 (-1: a channel not finite, -2: farther than max_distance), scores [Q, nc] fp32 or None, distance [Q] fp32
GaussianResult = namedtuple("GaussianResult", ["classes", "scores", "distance"])
# classes [Bs, Hs, Ws] int64, scores [Bs, nc, Hs, Ws] fp32 (the layout of predict_scene's logits), distance [Bs, Hs, Ws] fp32, cover
GaussianScene = namedtuple("GaussianScene", ["classes", "scores", "distance", "cover"])

LOG_2PI_HALF_DIM = 0.5 * DIM * math.log(2.0 * math.pi)      # 48 log(2 pi)
_MOMENTS = 2 + DIM + DIM * DIM                              # floats of one feature_moments out= buffer


def gauss_score(features, centres, tables, class_table, offsets, consts, max_d2=float("inf"), scores=True, out_layout=0):
    """msst_gauss_score on the current stream: (classes int32, distance, scores or None) of `features` (rows, a KnnBank or a map) under
    the table form -- centres [T, 96], tables [T, 96, 96], offsets [nc, 96], consts [nc] (fp32, contiguous, on the device) and
    class_table, a HOST sequence of nc table ids.  Outputs are flat over the rows but for scores with out_layout 1: [Bs, nc, Hs, Ws]."""
    x, layout, rows, plane = _source(features)
    for t, what in ((x, "features"), (centres, "the centres"), (tables, "the tables"), (offsets, "the offsets"), (consts, "the constants")):
        _require_cuda(t, what)
    nc, T = offsets.shape[0], centres.shape[0]
    ids = (ctypes.c_int32 * nc)(*[int(v) for v in class_table])
    if out_layout == 1 and layout != 1:
        raise ValueError("a map output needs a map input")
    classes = torch.empty(rows, dtype=torch.int32, device=x.device)
    distance = torch.empty(rows, dtype=torch.float32, device=x.device)
    s = None
    if scores:
        s = torch.empty((x.shape[0], nc) + tuple(x.shape[2:]) if out_layout == 1 else (rows, nc), dtype=torch.float32, device=x.device)
    lib = _lib.load()
    _lib.check(lib.msst_gauss_score(_p(x), layout, rows, plane, DIM, _p(centres), _p(tables), T, ctypes.cast(ids, ctypes.c_void_p), _p(offsets),
                                    _p(consts), nc, float(max_d2), _p(classes), _p(distance), _p(s), out_layout, _stream()), "msst_gauss_score")
    return classes, distance, s


def _check_rcond(rcond):
    if isinstance(rcond, bool) or not isinstance(rcond, (int, float)) or not 0 <= rcond < 1:
        raise ValueError(f"rcond must lie in [0, 1), got {rcond!r}")


def _check_max_distance(max_distance):
    if max_distance is None:
        return float("inf")
    if isinstance(max_distance, bool) or not isinstance(max_distance, (int, float)) or not max_distance >= 0:
        raise ValueError(f"max_distance must be None or a number >= 0, got {max_distance!r}")
    return float(max_distance)


def whitening_rules(sigma, rcond):
    """(A [96, 96], logdet) of a covariance, float64: eigen_rules, the eigenvalues floored at rcond x the largest, A = V / sqrt(lambda)
    (rows), logdet = sum log lambda.  ValueError for a largest eigenvalue of 0, or a smallest of 0 with rcond = 0."""
    lam, comp = eigen_rules(sigma)
    if not np.isfinite(lam).all() or not lam[0] > 0:
        raise ValueError("the largest eigenvalue of a covariance is 0 (or the covariance is not finite)")
    lam = np.maximum(lam, rcond * lam[0])
    if not lam[-1] > 0:
        raise ValueError("a covariance is singular and rcond = 0 floors nothing")
    return comp / np.sqrt(lam)[:, None], float(np.log(lam).sum())


class GaussianClassifier:
    """Class-conditional Gaussians over 96-wide features, fitted (fit_gaussian) or from the user's own arrays, checked once here.
      means              [nc, 96] fp32 tensor (float64 values are rounded once; an absent class: zeros)
      covariances        [nc, 96, 96] float64 numpy on the CPU, the per-class covariances as given (None when tied)
      pooled_covariance  [96, 96] float64 numpy: the tied covariance, or under full covariances the pooled one when the fit made it
      priors             [nc] float64 numpy, >= 0, normalised to sum 1; a class with prior 0 is never predicted
      counts             [nc] int64 numpy (None when not given)
      logdet             [nc] (tied: [1]) float64 numpy: sum log lambda of the floored eigenvalues (NaN for an absent class)
      tied               one covariance for every class
    covariances: [nc, 96, 96], or [96, 96] with tied=True.  A class is absent when its prior is 0 (and, with counts, when its count is
    0): it needs no valid covariance.  ValueError for wrong shapes or dtypes, values that are not finite, negative priors or priors
    that sum to 0, more than 128 classes, a largest eigenvalue of 0, or rcond outside [0, 1)."""

    def __init__(self, means, covariances, priors, counts=None, tied=False, rcond=1e-6, _pooled=None):
        m = means.detach().cpu().numpy() if torch.is_tensor(means) else np.asarray(means)
        if m.ndim != 2 or m.shape[1] != DIM or not 1 <= m.shape[0] <= MAX_CLASSES or m.dtype not in (np.float32, np.float64):
            raise ValueError(f"means must be float32 or float64 [nc, {DIM}] with 1 <= nc <= {MAX_CLASSES}, got {getattr(means, 'shape', type(means))}")
        nc = m.shape[0]
        cov = covariances.detach().cpu().numpy() if torch.is_tensor(covariances) else np.asarray(covariances)
        if cov.dtype not in (np.float32, np.float64) or cov.shape != ((DIM, DIM) if tied else (nc, DIM, DIM)):
            raise ValueError(f"covariances must be float [{'' if tied else 'nc, '}{DIM}, {DIM}], got {getattr(covariances, 'shape', type(covariances))}")
        pr = priors.detach().cpu().numpy() if torch.is_tensor(priors) else np.asarray(priors)
        if pr.shape != (nc,) or pr.dtype.kind not in "fiu" or not np.isfinite(pr).all() or (pr < 0).any() or not pr.sum() > 0:
            raise ValueError(f"priors must be [{nc}] finite weights >= 0 with a positive sum")
        if counts is not None:
            counts = counts.detach().cpu().numpy() if torch.is_tensor(counts) else np.asarray(counts)
            if counts.shape != (nc,) or counts.dtype.kind not in "iu" or (counts < 0).any():
                raise ValueError(f"counts must be None or [{nc}] integers >= 0")
            counts = counts.astype(np.int64)
        _check_rcond(rcond)
        pr = pr.astype(np.float64)
        if counts is not None:
            pr = np.where(counts > 0, pr, 0.0)
            if not pr.sum() > 0:
                raise ValueError("every class with a positive prior has a count of 0")
        pr = pr / pr.sum()
        present = pr > 0
        m64, cov64 = m.astype(np.float64), cov.astype(np.float64)
        if not np.isfinite(m64[present]).all() or not np.isfinite(cov64 if tied else cov64[present]).all():
            raise ValueError("the means and covariances of the present classes must be finite")
        m64 = np.where(present[:, None], m64, 0.0)
        self.tied, self.rcond, self.n_classes = bool(tied), float(rcond), nc
        self.priors, self.counts = pr, counts
        self.covariances = None if tied else cov64
        self.pooled_covariance = cov64 if tied else _pooled
        self._means64 = m64
        self.means = torch.from_numpy(m64).float()
        if torch.is_tensor(means) and means.is_cuda:
            self.means = self.means.to(means.device)
        # ---- the table form, float64 -> fp32 once
        ids = np.nonzero(present)[0]
        logdet = np.full(1 if tied else nc, np.nan)
        offsets = np.zeros((nc, DIM))
        class_table = np.zeros(nc, dtype=np.int32)
        if tied:
            a, logdet[0] = whitening_rules(cov64, rcond)
            w = counts[ids].astype(np.float64) if counts is not None else pr[ids]
            centre = ((w[:, None] * m64[ids]).sum(axis=0) / w.sum()).astype(np.float32)      # what the kernel subtracts
            centres, tables = centre[None, :], a[None, :, :]
            offsets[ids] = (m64[ids] - centre.astype(np.float64)) @ a.T
            ld = np.full(nc, logdet[0])
        else:
            tables = np.empty((len(ids), DIM, DIM))
            for t, c in enumerate(ids):
                try:
                    tables[t], logdet[c] = whitening_rules(cov64[c], rcond)
                except ValueError as e:
                    raise ValueError(f"class {c}: {e}") from None
                class_table[c] = t
            centres = m64[ids]
            ld = logdet
        with np.errstate(divide="ignore", invalid="ignore"):
            consts = np.where(present, np.log(pr) - 0.5 * np.where(present, ld, 0.0) - LOG_2PI_HALF_DIM, -np.inf)
        self.logdet = logdet
        self._host = dict(centres=np.ascontiguousarray(centres, dtype=np.float32), tables=np.ascontiguousarray(tables, dtype=np.float32),
                          offsets=offsets.astype(np.float32), consts=consts.astype(np.float32))
        self._class_table = class_table
        self._device = {}

    def _tables(self, device):
        key = str(device)
        if key not in self._device:
            self._device[key] = {k: torch.from_numpy(v).to(device).contiguous() for k, v in self._host.items()}
        return self._device[key]

    def _launch(self, features, scores, max_d2, out_layout=0, only=None):
        """the launch on all classes, or (only = c) on class c alone: its distance is then d2_c, with the bits it has among all"""
        x, _, _, _ = _source(features)
        _require_cuda(x, "features")
        t = self._tables(x.device)
        if only is None:
            return gauss_score(features, t["centres"], t["tables"], self._class_table, t["offsets"], t["consts"], max_d2, scores, out_layout)
        k = int(self._class_table[only])
        return gauss_score(features, t["centres"][k:k + 1], t["tables"][k:k + 1], [0], t["offsets"][only:only + 1], t["consts"][only:only + 1],
                           max_d2, scores, out_layout)

    def classify(self, features, scores=True, max_distance=None):
        """GaussianResult(classes [Q] int64, scores [Q, nc] fp32 or None, distance [Q] fp32) of rows [Q, 96] (fp32, contiguous, on the
        device), a KnnBank or a map [Bs, 96, Hs, Ws] (Q = Bs Hs Ws, read in place): see the module's contract.  ValueError before any
        device work for a wrong shape, dtype or max_distance; RuntimeError for CPU tensors."""
        _source(features)
        max_d2 = _check_max_distance(max_distance)
        classes, distance, s = self._launch(features, bool(scores), max_d2)
        return GaussianResult(classes.long(), s, distance)

    def own_distance(self, bank):
        """[M] fp32: the distance of every bank row to its OWN class, in the bank's row order (NaN for a row of an absent class).  Not
        one launch: the bank's rows are sorted by class as in the fit (a stable sort, one gather, and the read-back of the nc class
        counts that size the launches: one synchronisation), then every present class's slice is scored against that class alone
        -- up to nc launches of msst_gauss_score, each with the bits the class has among all."""
        _check_bank(bank)
        _require_cuda(bank.features, "the bank's features")
        order, rows, counts = _sort_by_class(bank)
        out = torch.full((len(bank),), float("nan"), dtype=torch.float32, device=bank.features.device)
        sorted_out = torch.empty_like(out)
        start = 0
        for c, n in enumerate(counts):
            if n and self.priors[c] > 0:
                sorted_out[start:start + n] = self._launch(rows[start:start + n], False, float("inf"), only=c)[1]
            elif n:
                sorted_out[start:start + n] = float("nan")
            start += n
        out[order] = sorted_out
        return out

    def threshold(self, bank, quantile=0.99):
        """The `quantile` of the bank rows' distance to their OWN class, a float: a max_distance under which that share of the bank's
        rows is kept.  It costs what own_distance costs (a sort, a gather, the read-back of the class counts, up to nc launches), a
        sort of the M distances and a second synchronisation for the returned float: call it once per bank, not per batch."""
        if isinstance(quantile, bool) or not isinstance(quantile, (int, float)) or not 0 <= quantile <= 1:
            raise ValueError(f"quantile must lie in [0, 1], got {quantile!r}")
        d = self.own_distance(bank)
        d = d[~torch.isnan(d)]
        if not len(d):
            raise ValueError("no bank row belongs to a class of the classifier")
        k = min(len(d) - 1, max(0, int(math.ceil(quantile * len(d))) - 1))      # the smallest distance that keeps the share
        return float(torch.sort(d)[0][k])


def _check_bank(bank):
    if not isinstance(bank, KnnBank):
        raise ValueError(f"bank must be a KnnBank (of raw features: probe_bank), got {type(bank).__name__}")


def _sort_by_class(bank):
    """(order, the rows gathered in class order, the class counts as a list): a stable sort, one gather, one small read-back"""
    labels = bank.labels.long()
    order = torch.argsort(labels, stable=True)
    counts = torch.bincount(labels, minlength=bank.n_classes).tolist()
    return order, bank.features[order].contiguous(), counts


def _check_fit(bank, covariance, shrinkage, priors, ddof, rcond):
    _check_bank(bank)
    if covariance not in ("full", "tied"):
        raise ValueError(f"covariance must be 'full' or 'tied', got {covariance!r}")
    if isinstance(shrinkage, bool) or not isinstance(shrinkage, (int, float)) or not 0 <= shrinkage <= 1:
        raise ValueError(f"shrinkage must lie in [0, 1], got {shrinkage!r}")
    if not _is_int(ddof) or ddof < 0:
        raise ValueError(f"ddof must be an integer >= 0, got {ddof!r}")
    _check_rcond(rcond)
    if isinstance(priors, str):
        if priors not in ("empirical", "uniform"):
            raise ValueError(f"priors must be 'empirical', 'uniform' or [{bank.n_classes}] weights, got {priors!r}")
        return None
    w = priors.detach().cpu().numpy() if torch.is_tensor(priors) else np.asarray(priors)
    if w.shape != (bank.n_classes,) or w.dtype.kind not in "fiu" or not np.isfinite(w).all() or (w < 0).any() or not w.sum() > 0:
        raise ValueError(f"priors must be 'empirical', 'uniform' or [{bank.n_classes}] finite weights >= 0 with a positive sum")
    return w.astype(np.float64)


def fit_gaussian(bank, covariance="full", shrinkage=0.0, priors="empirical", ddof=1, rcond=1e-6):
    """The class-conditional Gaussians of a bank of labelled RAW features (a KnnBank, e.g. from probe_bank).  Returns a
    GaussianClassifier.
      covariance  "full": Sigma_c = (1 - shrinkage) cov_c + shrinkage pooled (QDA; Friedman's regularised discriminant analysis);
                  "tied": the pooled covariance for every class (Fisher LDA).
      priors      "empirical" (n_c / n), "uniform" (over the classes with a row) or [nc] weights; a class with no row keeps 0.
      ddof        the covariances divide by n_c - ddof; pooled = sum_c (n_c - ddof) cov_c / sum_c (n_c - ddof) over n_c > ddof.
      rcond       the eigenvalues are floored at rcond x the largest.
    No kernel of its own: a stable sort and one gather, feature_moments (the centred two-pass pair) on every class's slice, one
    read-back of the stacked moments (after the nc class counts that size the launches).  ValueError before any device work for
    wrong arguments or, after the read-back, a bank row with a channel that is not finite; after the counts for a present class with fewer than ddof + 1 rows under "full" with shrinkage < 1 (it names
    the class) or no class with more than ddof rows; for a largest eigenvalue of 0.  RuntimeError for CPU tensors.  No CPU or eager
    fallback."""
    weights = _check_fit(bank, covariance, shrinkage, priors, ddof, rcond)
    _require_cuda(bank.features, "the bank's features")
    nc, tied = bank.n_classes, covariance == "tied"
    _, rows, counts = _sort_by_class(bank)
    n = np.asarray(counts, dtype=np.int64)
    if not tied and shrinkage < 1:
        for c in range(nc):
            if 0 < n[c] < ddof + 1:
                raise ValueError(f"class {c} has {n[c]} rows: a full covariance with ddof = {ddof} needs at least {ddof + 1}")
    dof = np.where(n > ddof, n - ddof, 0).astype(np.float64)
    if not dof.sum() > 0:
        raise ValueError(f"no class has more than ddof = {ddof} rows")
    buf = torch.zeros(nc, _MOMENTS, dtype=torch.float32, device=rows.device)
    start = 0
    for c in range(nc):
        if n[c]:
            part = rows[start:start + n[c]]
            first = feature_moments(part, None, ddof, cov=False)
            feature_moments(part, first.mean, ddof, out=buf[c])
        start += int(n[c])
    host = buf.cpu()                                   # the fit's read-back
    means = host[:, 2:2 + DIM].double().numpy()
    cov = host[:, 2 + DIM:].reshape(nc, DIM, DIM).double().numpy()
    counted = host[:, :2].contiguous().view(torch.int64).reshape(nc).numpy()
    if not np.array_equal(counted, n):
        c = int(np.nonzero(counted != n)[0][0])
        raise ValueError(f"class {c} has {n[c]} rows but {counted[c]} without a channel that is not finite: the bank's features must be finite "
                         "(drop the uncovered pixels of encode_scene: cover == 0)")
    pooled = np.zeros((DIM, DIM))
    for c in range(nc):
        if dof[c] > 0:
            pooled += dof[c] * cov[c]
    pooled /= dof.sum()
    present = n > 0
    if weights is None:
        pr = n.astype(np.float64) if priors == "empirical" else present.astype(np.float64)
    else:
        pr = np.where(present, weights, 0.0)
        if not pr.sum() > 0:
            raise ValueError("every class with a positive prior weight has no row")
    if tied:
        sigma = pooled
    else:
        sigma = np.zeros((nc, DIM, DIM))
        for c in range(nc):
            if present[c]:
                sigma[c] = pooled if shrinkage == 1 else (1.0 - shrinkage) * cov[c] + shrinkage * pooled
    return GaussianClassifier(torch.from_numpy(np.where(present[:, None], means, 0.0)).to(rows.device), sigma, pr, counts=n, tied=tied, rcond=rcond,
                              _pooled=pooled)


def gaussian_predict_scene(model, scene, clf, stride=None, max_distance=None, max_windows=None):
    """See ViTSpatialSpectral.gaussian_predict_scene."""
    if not isinstance(clf, GaussianClassifier):
        raise ValueError(f"clf must be a GaussianClassifier, got {type(clf).__name__}")
    max_d2 = _check_max_distance(max_distance)

    def launch(emb, Bs, Hs, Ws):
        classes, distance, scores = clf._launch(emb.features, True, max_d2, out_layout=1)
        return GaussianScene(classes.long().view(Bs, Hs, Ws), scores, distance.view(Bs, Hs, Ws), emb.cover)

    return on_scene_map(model, scene, stride, False, max_windows, launch)
