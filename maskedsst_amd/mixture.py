"""Gaussian mixture models of frozen per-pixel features, fitted by EM: the unsupervised second-order model beside the hard clusterer
(maskedsst_amd.cluster), the supervised class-conditional Gaussians (maskedsst_amd.gaussian) and the one-Gaussian RX score
(maskedsst_amd.pca).  Soft clusters with shape, whose responsibilities are a score map for crf_refine and superpixel_classify; a
density of the scene, whose per-pixel -log p(x) is the cluster-based RX anomaly detector; BIC over k.

    gm = fit_mixture(features, k=8, covariance="full", iters=30, reg_covar=1e-6, init="kmeans", seed=0, min_count=1.0,
                     check_every=None, tol=1e-3)      # features: contiguous fp32 [M, 96] on the device or a KnnBank of RAW features
    gm.weights; gm.means; gm.covariances; gm.tables; gm.logdet   # [K]; [K, 96]; [K, 96, 96]; [K, 96, 96] (A_c = L_c^-1); [K] -- fp32
    gm.history; gm.converged; gm.covariance; gm.reg_covar        # [iters, 4] float64 on the CPU; bool; str; float
    res = gm.predict(features, probs=False)    # MixtureResult(classes [Q] int64, log_likelihood [Q], distance [Q], probs [Q, K] | None)
    gm.bic(features); gm.aic(features)
    res = model.mixture_scene(scene, gm)       # MixtureScene(classes, log_likelihood, distance, probs [Bs, K, Hs, Ws] | None, cover)
    GaussianMixture(weights, means, covariances, covariance="full")   # from the user's arrays: float64 Cholesky on the host

The contract (once more in include/msst.h):
    score      score_c(x) = log w_c - 0.5 (d2_c(x) + logdet_c) - 48 log(2 pi), d2_c = |A_c (x - mu_c)|^2, Sigma_c = L_c L_c^T, A_c =
               L_c^-1, logdet_c = 2 sum_i log L_c[i][i]: msst_gauss_score's full-covariance table form with zero offsets, called
               through maskedsst_amd.gaussian.gauss_score, unchanged.
    posterior  lse(x) = m + log(sum_c exp(score_c - m)), m = max_c score_c, the sum over c ascending in fp32; r_c = exp(score_c - lse);
               a score of -inf contributes exactly 0.  classes: the argmax of the score under the project's one total order (score
               descending, then index ascending), as msst_gauss_score writes it; distance: d2 of that component; log_likelihood: lse.
    iteration  E-step under the current parameters; N_c = sum r_c; mu'_c = centre_c + sum r_c (x - centre_c) / N_c with centre_c the
               current mean; Sigma'_c = sum r_c (x - centre_c)(x - centre_c)^T / N_c - delta delta^T + reg_covar I, delta = mu'_c -
               centre_c ("diag": the off-diagonal entries set to 0 before the factorisation); w'_c = N_c / sum_c N_c.  The moments
               are taken about the component's current mean, not about zero: the features are far from centred and the one-pass
               form loses four digits.
    history    history[t] = (the mean log-likelihood per counted row under the parameters iteration t started from, the counted
               rows, the starved components, the failed factorisations).  The fit returns the parameters after the last M-step.
               check_every=n reads the history every n iterations and stops when the log-likelihood rose by less than tol over the
               last iteration; the stopped fit has the bits of a fit with iters equal to the iterations run, and `converged` says
               which of the two ended it.
    init       "kmeans": fit_kmeans(features, k, metric="euclidean", init="kmeans++", seed=seed); its hard assignment becomes a
               scores buffer of 0 / -inf (torch fills: plumbing) and one M-step about the centroids gives the starting parameters;
               that M-step is not in the history.  A KMeans (euclidean): the same from its centroids.  A GaussianMixture: its
               parameters.
    starved    a component with N_c < min_count keeps its mean, table, covariance and logdet; its weight still becomes N_c / sum N
               (0: its constant is -inf and it is never predicted).  A factorisation that meets a pivot that is not finite or not
               positive keeps them the same way and is counted.  Neither is an error.
    NaN rows   a row with a channel that is not finite (a pixel no window covers) gets class -1 and NaN log_likelihood, distance
               and probs; in a fit it is not counted and contributes to no sum, by selection.  A row whose scores are all -inf
               (every weight 0) has lse = -inf and probs 0; in the M-step it is skipped and not counted.
    same bits  no float atomics; every sum in an order that depends on (rows, K) alone, the row partition on rows alone: two fits
               give the same bits; a row's lse and probs have the same bits whatever batch it sits in, as rows or inside a map;
               covariances[c] is symmetric bit for bit.
    limits     feature width 96; fit K <= 32; a GaussianMixture from arrays and predict up to 128 components; fp32; rows up to
               2^31 - 1.

Three calls of ``libmsst.so`` (``maskedsst_amd/csrc/msst_gmm.hip``): ``msst_gmm_posterior`` (prediction), ``msst_gmm_moments`` and
``msst_gmm_update`` (the M-step).  A fit is 2 * iters + 2 launches of them plus iters launches of ``msst_gauss_score`` and ONE
synchronisation, the read-back of the history (one more per check with check_every).  There is no CPU or eager fallback.
"""
import ctypes
import math
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .cluster import KMeans, fit_kmeans
from .features import DIM, MAX_CLASSES, KnnBank, _is_int, _p, _stream, _require_cuda, check_rows, on_scene_map
from .gaussian import LOG_2PI_HALF_DIM, gauss_score
from .pca import _source

MAX_FIT_K = 32                     # include/msst.h: msst_gmm_moments, msst_gmm_update
COVARIANCES = {"full": 0, "diag": 1}       # include/msst.h: MSST_GMM_FULL, MSST_GMM_DIAG
HISTORY = ("mean_log_likelihood", "rows", "starved", "failed")   # the columns of GaussianMixture.history
SLAB_ROW = 1 + DIM + DIM * DIM     # floats of a (workgroup, component) slab row and of a `raw` row: [n | s1 | s2]

# classes [Q] int64 (-1: a channel not finite), log_likelihood [Q] fp32, distance [Q] fp32, probs [Q, K] fp32 or None
MixtureResult = namedtuple("MixtureResult", ["classes", "log_likelihood", "distance", "probs"])
# classes [Bs, Hs, Ws] int64 (-1 uncovered), log_likelihood and distance [Bs, Hs, Ws] fp32 (NaN uncovered), probs [Bs, K, Hs, Ws], cover
MixtureScene = namedtuple("MixtureScene", ["classes", "log_likelihood", "distance", "probs", "cover"])


def gmm_scratch_floats(rows, k):
    """msst_gmm_scratch_floats: the floats of the slab of msst_gmm_moments over `rows` rows and k components (0: refused)"""
    return int(_lib.load().msst_gmm_scratch_floats(rows, k))


def gmm_posterior(scores, layout, rows, plane, k, probs=True, out_layout=0):
    """msst_gmm_posterior on the current stream: (lse [rows], probs or None) of a scores buffer, rows [rows, k] (layout 0) or a map
    [Bs, k, Hs, Ws] (layout 1); probs as rows [rows, k] (out_layout 0) or as a map of the scores' shape (out_layout 1)."""
    _require_cuda(scores, "the scores")
    lse = torch.empty(rows, dtype=torch.float32, device=scores.device)
    p = None
    if probs:
        p = torch.empty(tuple(scores.shape) if out_layout == layout else (rows, k), dtype=torch.float32, device=scores.device)
    _lib.check(_lib.load().msst_gmm_posterior(_p(scores), layout, rows, plane, k, _p(lse), _p(p), out_layout, _stream()), "msst_gmm_posterior")
    return lse, p


def gmm_moments(features, scores, centres, slab=None):
    """msst_gmm_moments on the current stream: the slab of per-workgroup responsibility-weighted moments of `features` (rows, a
    KnnBank or a map) under scores [rows, k] about centres [k, 96]."""
    x, layout, rows, plane = _source(features)
    for t, what in ((x, "features"), (scores, "the scores"), (centres, "the centres")):
        _require_cuda(t, what)
    k = centres.shape[0]
    if scores.shape != (rows, k) or scores.dtype != torch.float32 or not scores.is_contiguous():
        raise ValueError(f"scores must be a contiguous float32 tensor [{rows}, {k}], got {tuple(scores.shape)} of {scores.dtype}")
    if slab is None:
        slab = torch.empty(gmm_scratch_floats(rows, k), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().msst_gmm_moments(_p(x), layout, rows, plane, DIM, _p(scores), k, _p(centres), _p(slab), slab.numel(), _stream()),
               "msst_gmm_moments")
    return slab


def gmm_update(slab, rows, state, covariance, reg_covar, min_count, record, raw=None):
    """msst_gmm_update on the current stream: the M-step from a slab, in place on `state` (a dict of contiguous fp32 device tensors:
    means [k, 96], tables and covariances [k, 96, 96], logdet, consts, weights [k]).  record: a ZEROED contiguous fp32 row of 4 (see
    read_records); raw: None or [k, 1 + 96 + 96 * 96]."""
    k = state["means"].shape[0]
    _lib.check(_lib.load().msst_gmm_update(_p(slab), slab.numel(), rows, DIM, k, COVARIANCES[covariance], float(reg_covar), float(min_count),
                                           _p(state["means"]), _p(state["tables"]), _p(state["covariances"]), _p(state["logdet"]),
                                           _p(state["consts"]), _p(state["weights"]), _p(raw), ctypes.c_void_p(record.data_ptr()), _stream()),
               "msst_gmm_update")


def new_state(k, device, means=None):
    """the parameter tensors of k components before any M-step: unit covariances, so that a component starved from the start keeps
    something valid"""
    eye = torch.eye(DIM, dtype=torch.float32, device=device).repeat(k, 1, 1).contiguous()
    return dict(means=torch.zeros(k, DIM, dtype=torch.float32, device=device) if means is None else means.detach().clone().contiguous(),
                tables=eye, covariances=eye.clone(), logdet=torch.zeros(k, dtype=torch.float32, device=device),
                consts=torch.full((k,), -math.log(k) - LOG_2PI_HALF_DIM, dtype=torch.float32, device=device),
                weights=torch.full((k,), 1.0 / k, dtype=torch.float32, device=device))


def read_records(rec):
    """records [iters, 4] fp32 on the CPU -> history [iters, 4] float64: the mean log-likelihood, and the counted rows, starved
    components and failed factorisations from their int32 bits"""
    ints = rec[:, 1:].contiguous().view(torch.int32).double()
    return torch.cat([rec[:, :1].double(), ints], dim=1)


def n_parameters(k, covariance):
    """the free parameters of a mixture: k means, k covariances (96 * 97 / 2 entries, or 96 for "diag") and k - 1 weights"""
    return k * DIM + k * (DIM * (DIM + 1) // 2 if covariance == "full" else DIM) + k - 1


def _check_covariance(covariance):
    if covariance not in COVARIANCES:
        raise ValueError(f"covariance must be 'full' or 'diag', got {covariance!r}")


def _host(a, what, shape):
    v = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    if v.dtype not in (np.float32, np.float64) or v.shape != shape:
        raise ValueError(f"{what} must be float32 or float64 {list(shape)}, got {getattr(a, 'shape', type(a))}")
    return v.astype(np.float64)


class GaussianMixture:
    """A mixture of K Gaussians over 96-wide features, fitted (fit_mixture) or from the user's own arrays, checked once here:
      weights      [K] >= 0 with a positive sum, normalised to sum 1; a component of weight 0 is never predicted
      means        [K, 96]
      covariances  [K, 96, 96] symmetric positive definite ("diag": the off-diagonal entries are set to 0)
    float32 or float64 arrays or tensors, 1 <= K <= 128.  The Cholesky factorisation runs in float64 on the host; tables (A_c =
    L_c^-1, lower triangular), logdet and the per-component constants are rounded to fp32 once.  The attributes are fp32 tensors, on the
    device of `means` when that is a tensor; predict moves them to the device of its features once.  ValueError for wrong shapes or
    dtypes, values that are not finite, negative weights or weights that sum to 0, or a covariance that is not positive definite."""

    def __init__(self, weights, means, covariances, covariance="full"):
        _check_covariance(covariance)
        means = means if torch.is_tensor(means) else np.asarray(means)
        if not hasattr(means, "shape") or len(means.shape) != 2 or means.shape[1] != DIM or not 1 <= means.shape[0] <= MAX_CLASSES:
            raise ValueError(f"means must be [K, {DIM}] with 1 <= K <= {MAX_CLASSES}, got {getattr(means, 'shape', type(means))}")
        k = means.shape[0]
        m = _host(means, "means", (k, DIM))
        cov = _host(covariances, "covariances", (k, DIM, DIM))
        w = _host(weights, "weights", (k,))
        if not np.isfinite(w).all() or (w < 0).any() or not w.sum() > 0:
            raise ValueError(f"weights must be [{k}] finite values >= 0 with a positive sum")
        if not np.isfinite(m).all() or not np.isfinite(cov).all():
            raise ValueError("means and covariances must be finite")
        w = w / w.sum()
        if covariance == "diag":
            cov = cov * np.eye(DIM)[None]
        tables, logdet = np.empty_like(cov), np.empty(k)
        for c in range(k):
            if not np.array_equal(cov[c], cov[c].T):
                raise ValueError(f"component {c}: the covariance is not symmetric")
            try:
                L = np.linalg.cholesky(cov[c])
            except np.linalg.LinAlgError:
                raise ValueError(f"component {c}: the covariance is not positive definite") from None
            tables[c] = np.tril(np.linalg.solve(L, np.eye(DIM)))
            logdet[c] = 2.0 * np.log(np.diag(L)).sum()
        with np.errstate(divide="ignore"):
            consts = np.log(w) - 0.5 * logdet - LOG_2PI_HALF_DIM
        dev = means.device if torch.is_tensor(means) else torch.device("cpu")
        put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float().contiguous().to(dev)   # noqa: E731
        self._set(dict(weights=put(w), means=put(m), covariances=put(cov), tables=put(tables), logdet=put(logdet), consts=put(consts)),
                  covariance, 0.0, None, False)

    def _set(self, state, covariance, reg_covar, history, converged):
        self.weights, self.means, self.covariances = state["weights"], state["means"], state["covariances"]
        self.tables, self.logdet, self.consts = state["tables"], state["logdet"], state["consts"]
        self.covariance, self.reg_covar, self.history, self.converged = covariance, float(reg_covar), history, bool(converged)
        self._device = {}

    @classmethod
    def _fitted(cls, state, covariance, reg_covar, history, converged):
        gm = cls.__new__(cls)
        gm._set(state, covariance, reg_covar, history, converged)
        return gm

    @property
    def k(self):
        return self.means.shape[0]

    def _on(self, device):
        key = str(device)
        if key not in self._device:
            self._device[key] = dict(means=self.means.to(device).contiguous(), tables=self.tables.to(device).contiguous(),
                                     consts=self.consts.to(device).contiguous(),
                                     offsets=torch.zeros(self.k, DIM, dtype=torch.float32, device=device))
        return self._device[key]

    def _launch(self, features, probs, out_layout):
        x, layout, rows, plane = _source(features)
        _require_cuda(x, "features")
        t = self._on(x.device)
        classes, distance, s = gauss_score(features, t["means"], t["tables"], range(self.k), t["offsets"], t["consts"], scores=True,
                                           out_layout=out_layout)
        lse, p = gmm_posterior(s, out_layout, rows, plane, self.k, bool(probs), out_layout)
        return classes.long(), lse, distance, p

    def predict(self, features, probs=False):
        """MixtureResult(classes [Q] int64, log_likelihood [Q], distance [Q], probs [Q, K] or None) of rows [Q, 96] (fp32, contiguous,
        on the device), a KnnBank or a map [Bs, 96, Hs, Ws] (Q = Bs Hs Ws, read in place): see the module's contract.  Two launches,
        msst_gauss_score and msst_gmm_posterior.  ValueError before any device work for a wrong shape or dtype; RuntimeError for CPU
        tensors."""
        return MixtureResult(*self._launch(features, probs, 0))

    def log_likelihood(self, features):
        """(the summed log-likelihood of the counted rows, the counted rows): python numbers, one synchronisation.  A row with a
        channel that is not finite is not counted."""
        ll = self.predict(features).log_likelihood
        ok = ~torch.isnan(ll)
        total, n = torch.stack([torch.where(ok, ll, torch.zeros_like(ll)).double().sum(), ok.sum().double()]).tolist()
        return total, int(n)

    def bic(self, features):
        """-2 log L + p log n from the summed log-likelihood of `features`, the counted rows n and the parameter count p"""
        total, n = self.log_likelihood(features)
        return -2.0 * total + n_parameters(self.k, self.covariance) * math.log(n) if n else float("nan")

    def aic(self, features):
        """-2 log L + 2 p"""
        total, n = self.log_likelihood(features)
        return -2.0 * total + 2.0 * n_parameters(self.k, self.covariance) if n else float("nan")


def _check_fit(features, k, covariance, iters, reg_covar, init, seed, min_count, check_every, tol):
    x = features.features if isinstance(features, KnnBank) else features
    check_rows(x, "features", 1, few="features needs at least one row")
    if not _is_int(k) or not 1 <= k <= MAX_FIT_K:
        raise ValueError(f"k must be an integer in [1, {MAX_FIT_K}], got {k!r}")
    if x.shape[0] < k:
        raise ValueError(f"k = {k} components need at least {k} rows, got {x.shape[0]}")
    _check_covariance(covariance)
    if not _is_int(iters) or iters < 1:
        raise ValueError(f"iters must be an integer >= 1, got {iters!r}")
    for v, what in ((reg_covar, "reg_covar"), (min_count, "min_count"), (tol, "tol")):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not v >= 0 or math.isinf(v):
            raise ValueError(f"{what} must be a finite number >= 0, got {v!r}")
    if not _is_int(seed) or not 0 <= seed < 2 ** 32:
        raise ValueError(f"seed must be an integer in [0, 2^32), got {seed!r}")
    if check_every is not None and (not _is_int(check_every) or check_every < 1):
        raise ValueError(f"check_every must be None or an integer >= 1, got {check_every!r}")
    if isinstance(init, KMeans):
        if init.metric != "euclidean":
            raise ValueError("a KMeans init must have metric 'euclidean': cosine centroids are directions, not means")
        if init.k != k:
            raise ValueError(f"the KMeans init has {init.k} clusters, k = {k}")
    elif isinstance(init, GaussianMixture):
        if init.k != k:
            raise ValueError(f"the GaussianMixture init has {init.k} components, k = {k}")
    elif not (isinstance(init, str) and init == "kmeans"):
        raise ValueError(f"init must be 'kmeans', a KMeans (euclidean) or a GaussianMixture, got {init!r}")
    return x


def fit_mixture(features, k=8, covariance="full", iters=30, reg_covar=1e-6, init="kmeans", seed=0, min_count=1.0, check_every=None,
                tol=1e-3):
    """EM for a mixture of k Gaussians on frozen RAW features.  Returns a GaussianMixture.
      features     a contiguous fp32 tensor [M, 96] on the device, checked finite once (one read-back), or a KnnBank (checked when it
                   was built).
      covariance   "full" or "diag".
      iters        every fit runs exactly this many iterations (check_every aside): per iteration msst_gauss_score, msst_gmm_moments
                   and msst_gmm_update, and ONE synchronisation at the end, the read-back of the history.
      reg_covar    added to the diagonal of every covariance.
      init         "kmeans" (fit_kmeans with metric "euclidean", init "kmeans++" and `seed`), a KMeans (euclidean) or a GaussianMixture.
      min_count    a component with N_c below it is starved: see the module's contract.
      check_every  n: the history is read every n iterations and the fit stops when the mean log-likelihood rose by less than `tol`
                   over the last iteration; the result has the bits of a fit with iters equal to the iterations run.
    ValueError, before any device work, for wrong shapes or dtypes, k outside [1, 32], M < k, a bad covariance, init, reg_covar,
    iters, seed, min_count, check_every or tol, or a cosine KMeans; RuntimeError for CPU tensors.  No CPU or eager fallback."""
    x = _check_fit(features, k, covariance, iters, reg_covar, init, seed, min_count, check_every, tol)
    _require_cuda(x, "features")
    dev, M = x.device, x.shape[0]
    checked = isinstance(features, KnnBank)
    if isinstance(init, str):
        init = fit_kmeans(features, k, metric="euclidean", init="kmeans++", seed=seed)      # checks the features finite
        checked = True
    if not checked and not bool(torch.isfinite(x).all()):
        raise ValueError("features must be finite (drop the uncovered pixels of encode_scene: cover == 0)")
    slab = torch.empty(gmm_scratch_floats(M, k), dtype=torch.float32, device=dev)
    if isinstance(init, KMeans):
        _require_cuda(init.centroids, "the centroids")
        labels, _ = init.assign(x)
        scores = torch.full((M, k), float("-inf"), dtype=torch.float32, device=dev)
        scores.scatter_(1, labels.clamp_(min=0)[:, None], 0.0)
        state = new_state(k, dev, init.centroids.to(dev))
        gmm_moments(x, scores, state["means"], slab)
        gmm_update(slab, M, state, covariance, reg_covar, min_count, torch.zeros(4, dtype=torch.float32, device=dev))
    else:
        state = {name: getattr(init, name).detach().to(dev).clone().contiguous()
                 for name in ("means", "tables", "covariances", "logdet", "consts", "weights")}
    offsets = torch.zeros(k, DIM, dtype=torch.float32, device=dev)
    rec = torch.zeros(iters, 4, dtype=torch.float32, device=dev)
    done, converged, host = iters, False, None
    for t in range(iters):
        _, _, scores = gauss_score(x, state["means"], state["tables"], range(k), offsets, state["consts"], scores=True)
        gmm_moments(x, scores, state["means"], slab)
        gmm_update(slab, M, state, covariance, reg_covar, min_count, rec[t])
        if check_every is not None and (t + 1) % check_every == 0 and t >= 1 and t + 1 < iters:
            host = rec[:t + 1].cpu()
            if float(host[t, 0]) - float(host[t - 1, 0]) < tol:
                done, converged = t + 1, True
                break
    if not converged:
        host = rec.cpu()          # the fit's one synchronisation (check_every: one more per check)
    return GaussianMixture._fitted(state, covariance, reg_covar, read_records(host[:done]), converged)


def mixture_scene(model, scene, gm, stride=None, probs=False, max_windows=None):
    """See ViTSpatialSpectral.mixture_scene."""
    if not isinstance(gm, GaussianMixture):
        raise ValueError(f"gm must be a GaussianMixture, got {type(gm).__name__}")

    def launch(emb, Bs, Hs, Ws):
        classes, lse, distance, p = gm._launch(emb.features, probs, 1)
        return MixtureScene(classes.view(Bs, Hs, Ws), lse.view(Bs, Hs, Ws), distance.view(Bs, Hs, Ws), p, emb.cover)

    return on_scene_map(model, scene, stride, False, max_windows, launch)
