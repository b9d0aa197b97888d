"""The second-order structure of frozen per-pixel features: the spectrum of their covariance (the label-free health check of a
self-supervised encoder: explained-variance ratios and the effective rank, RankMe), principal-component maps of whole scenes (the
false-colour picture of an embedding) and RX anomaly scores (the squared Mahalanobis distance of a pixel to a bank's or the scene's
own mean under its covariance).

    pca = fit_pca(features, n_components=None, ddof=1, rcond=1e-6)   # rows [M, 96], a KnnBank, or a map [Bs, 96, Hs, Ws] (NaN pixels skipped)
    pca.explained_variance_ratio, pca.effective_rank, pca.rank       # float64 on the CPU
    z = pca.transform(features, whiten=False)                        # [Q, r]
    d2 = pca.mahalanobis(features)                                   # [Q]
    res = model.pca_scene(scene, pca)                                # PcaScene(components [Bs, r, Hs, Ws], cover)
    res = model.anomaly_scene(scene)                                 # AnomalyScene(score [Bs, Hs, Ws], cover, pca): global RX

Three calls of ``libmsst.so`` (``maskedsst_amd/csrc/msst_pca.hip``, ``include/msst.h``).  ``msst_feat_moments`` streams the rows
once and leaves, per workgroup, the count, the sum and the matrix of second moments of ``x - centre`` (``x^T x`` on the fp32 matrix
cores); ``msst_feat_moments_finish`` adds the partials in a fixed order in double.  A fit is the centred TWO-PASS covariance -- the
features are far from centred, and the one-pass form ``(sum x x^T - n mu mu^T) / (n - 1)`` loses four digits on them in fp32 -- as
four launches and one read-back: moments about zero, the mean, moments about that mean, the covariance (corrected by the second
pass's residual sum).  The 96 x 96 eigendecomposition runs on the host in float64 (numpy.linalg.eigh: 96^3 flops).
``msst_feat_project`` is the projection onto given directions with the squared norm of the result; whitening is folded into the
directions on the host, so it costs nothing on the device.  No atomics: equal inputs give equal bits.  There is no CPU or eager
fallback.
"""
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .features import DIM, KnnBank, _is_int, _p, _stream, _require_cuda, check_rows, on_scene_map

# components [Bs, r, Hs, Ws] fp32 (NaN where no window covers the pixel), cover [Bs, Hs, Ws] int32
PcaScene = namedtuple("PcaScene", ["components", "cover"])
# score [Bs, Hs, Ws] fp32: the squared Mahalanobis distance (NaN where uncovered), cover [Bs, Hs, Ws] int32, pca: the FeaturePCA used
AnomalyScene = namedtuple("AnomalyScene", ["score", "cover", "pca"])
# what msst_feat_moments_finish writes, on the device: count [1] int64, mean [96], cov [96, 96] or None, raw [96 + 96 * 96] or None
FeatureMoments = namedtuple("FeatureMoments", ["count", "mean", "cov", "raw"])


def _source(features, what="features"):
    """(x, layout, rows, plane) of rows [M, 96], a KnnBank, a map [Bs, 96, Hs, Ws] or an object with such a map as .features (a
    SceneEmbedding); ValueError otherwise"""
    x = features.features if isinstance(features, KnnBank) or (not torch.is_tensor(features) and hasattr(features, "features")) else features
    if torch.is_tensor(x) and x.dim() == 4:
        if x.shape[1] != DIM or x.dtype != torch.float32 or not x.is_contiguous() or x.numel() == 0:
            raise ValueError(f"{what} must be a contiguous float32 map [Bs, {DIM}, Hs, Ws], got {tuple(x.shape)} of {x.dtype}")
        plane = x.shape[2] * x.shape[3]
        return x, 1, x.shape[0] * plane, plane
    check_rows(x, what, 1, shape=f"[M, {DIM}] (or a map [Bs, {DIM}, Hs, Ws])", few=f"{what} needs at least one row")
    return x, 0, x.shape[0], 1


def feature_moments(features, centre=None, ddof=1, cov=True, raw=False, out=None):
    """msst_feat_moments and msst_feat_moments_finish on the current stream, no synchronisation: the moments of `features` (rows, a
    KnnBank or a map, rows with a NaN channel skipped) about `centre` ([96] fp32 on the device; None: zeros).  Returns
    FeatureMoments(count, mean, cov, raw) on the device; `out` (a contiguous fp32 tensor of 2 + 96 + 96 * 96 floats) takes count (as
    int64 bits), mean and cov back to back."""
    x, layout, rows, plane = _source(features)
    _require_cuda(x, "features")
    if not _is_int(ddof) or ddof < 0:
        raise ValueError(f"ddof must be an integer >= 0, got {ddof!r}")
    if centre is not None and (not torch.is_tensor(centre) or centre.shape != (DIM,) or centre.dtype != torch.float32 or not centre.is_contiguous()):
        raise ValueError(f"centre must be None or a contiguous float32 tensor [{DIM}]")
    if centre is not None:
        _require_cuda(centre, "the centre")
    lib = _lib.load()
    dev, st = x.device, _stream()
    nslab = int(lib.msst_feat_moments_scratch_floats(rows))
    slab = torch.empty(max(nslab, 1), dtype=torch.float32, device=dev)
    buf = torch.empty(2 + DIM + DIM * DIM, dtype=torch.float32, device=dev) if out is None else out
    count, mean, c = buf[:2].view(torch.int64), buf[2:2 + DIM], buf[2 + DIM:].view(DIM, DIM)
    r = torch.empty(DIM + DIM * DIM, dtype=torch.float32, device=dev) if raw else None
    _lib.check(lib.msst_feat_moments(_p(x), layout, rows, plane, DIM, _p(centre), _p(slab), nslab, st), "msst_feat_moments")
    _lib.check(lib.msst_feat_moments_finish(_p(slab), nslab, rows, DIM, _p(centre), ddof, _p(count), _p(mean), _p(c) if cov else None, _p(r), st),
               "msst_feat_moments_finish")
    return FeatureMoments(count, mean, c if cov else None, r)


def feature_project(features, mean, components, out_layout=0, out=True, sumsq=False):
    """msst_feat_project on the current stream: (out, sumsq) of `features` (rows, a KnnBank or a map) against mean [96] and components
    [r, 96] (fp32, contiguous, on the device).  out is rows [Q, r] (out_layout 0) or a map [Bs, r, Hs, Ws] (out_layout 1: a map input
    only); sumsq [Q] (or [Bs, Hs, Ws]).  Either is None when not asked for."""
    x, layout, rows, plane = _source(features)
    for t, what in ((x, "features"), (mean, "the mean"), (components, "the components")):
        _require_cuda(t, what)
    r = components.shape[0]
    if out_layout == 1 and layout != 1:
        raise ValueError("a map output needs a map input")
    o = s = None
    if out:
        o = torch.empty((x.shape[0], r) + tuple(x.shape[2:]) if out_layout == 1 else (rows, r), dtype=torch.float32, device=x.device)
    if sumsq:
        s = torch.empty((x.shape[0],) + tuple(x.shape[2:]) if layout == 1 else (rows,), dtype=torch.float32, device=x.device)
    lib = _lib.load()
    _lib.check(lib.msst_feat_project(_p(x), layout, rows, plane, DIM, _p(mean), _p(components), r, _p(o), out_layout, _p(s), _stream()),
               "msst_feat_project")
    return o, s


def eigen_rules(cov):
    """(eigenvalues [96] descending and clamped at 0, components [96, 96] unit rows) of a symmetric matrix, float64 numpy: the
    eigenvectors of numpy.linalg.eigh as rows, each with its entry of largest magnitude positive (ties: the lowest index)"""
    c = np.asarray(cov, dtype=np.float64)
    w, v = np.linalg.eigh(c)
    w, v = w[::-1], v[:, ::-1].T
    big = np.argmax(np.abs(v), axis=1)
    sign = np.where(v[np.arange(len(v)), big] < 0, -1.0, 1.0)
    return np.maximum(w, 0.0), np.ascontiguousarray(v * sign[:, None])


class FeaturePCA:
    """A fitted (or given) principal-component analysis of 96-wide features.
      mean                [96] fp32 tensor
      components          [r, 96] fp32 tensor, unit rows, r <= 96: the leading directions
      explained_variance  all 96 eigenvalues of the covariance, descending and >= 0: float64 numpy on the CPU
      count               the rows the fit counted
      rank                the number of eigenvalues above rcond * the largest
      covariance          [96, 96] float64 numpy: the covariance the fit read back (None for given arrays)
    Given arrays are checked once, here: ValueError for wrong shapes or dtypes, values that are not finite, eigenvalues that are
    negative or not descending, or rcond outside [0, 1)."""

    def __init__(self, mean, components, explained_variance, count, rcond=1e-6, _components64=None, _covariance=None):
        if not torch.is_tensor(mean) or mean.shape != (DIM,) or mean.dtype != torch.float32:
            raise ValueError(f"mean must be a float32 tensor [{DIM}], got {getattr(mean, 'shape', type(mean))}")
        if not torch.is_tensor(components) or components.dim() != 2 or components.shape[1] != DIM or components.dtype != torch.float32 \
                or not 1 <= components.shape[0] <= DIM:
            raise ValueError(f"components must be a float32 tensor [r, {DIM}] with 1 <= r <= {DIM}, got {getattr(components, 'shape', type(components))}")
        lam = np.asarray(explained_variance.detach().cpu().numpy() if torch.is_tensor(explained_variance) else explained_variance, dtype=np.float64)
        if lam.shape != (DIM,) or not np.isfinite(lam).all() or (lam < 0).any() or (np.diff(lam) > 0).any():
            raise ValueError(f"explained_variance must hold the {DIM} eigenvalues, finite, >= 0 and descending")
        if not _is_int(count) or count < 0:
            raise ValueError(f"count must be an integer >= 0, got {count!r}")
        if isinstance(rcond, bool) or not isinstance(rcond, (int, float)) or not 0 <= rcond < 1:
            raise ValueError(f"rcond must lie in [0, 1), got {rcond!r}")
        if not bool(torch.isfinite(mean).all()) or not bool(torch.isfinite(components).all()):
            raise ValueError("mean and components must be finite")
        self.mean = mean.contiguous()
        self.components = components.contiguous()
        self.explained_variance = lam
        self.count = count
        self.rcond = float(rcond)
        self.rank = int((lam > rcond * lam[0]).sum()) if lam[0] > 0 else 0
        self._c64 = self.components.detach().cpu().double().numpy() if _components64 is None else _components64
        self.covariance = _covariance
        self._tables = {}

    @property
    def n_components(self):
        return self.components.shape[0]

    @property
    def explained_variance_ratio(self):
        """lambda / sum lambda, float64 [96] (NaN when the sum is 0)"""
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.explained_variance / self.explained_variance.sum()

    @property
    def effective_rank(self):
        """exp of the entropy of the normalised eigenvalues (RankMe): 1 for a collapsed representation, 96 for an isotropic one"""
        p = self.explained_variance_ratio
        p = p[p > 0]
        return float(np.exp(-(p * np.log(p)).sum())) if len(p) else float("nan")

    def _device_tables(self, device, whiten):
        """(mean, components) on the device as the kernel takes them; whiten: rows j < min(r, rank) divided by sqrt(lambda_j) in
        float64 and rounded once, the rest dropped"""
        key = (str(device), bool(whiten))
        if key not in self._tables:
            c = self._c64
            if whiten:
                m = min(self.n_components, self.rank)
                if m < 1:
                    raise ValueError("whitening needs at least one eigenvalue above rcond * the largest")
                c = c[:m] / np.sqrt(self.explained_variance[:m])[:, None]
            self._tables[key] = (self.mean.to(device).contiguous(), torch.from_numpy(np.ascontiguousarray(c)).float().to(device).contiguous())
        return self._tables[key]

    def transform(self, features, whiten=False, out_layout=0):
        """The scores of rows [Q, 96] (fp32, contiguous, on the device): [Q, r], z_j = (x - mean) . component_j; whiten=True: divided
        by sqrt(lambda_j) for j < rank and the columns from rank on dropped.  A row with a NaN channel gets NaN.  A row has the same
        bits whatever batch it sits in."""
        x, _, _, _ = _source(features)
        _require_cuda(x, "features")
        mean, comp = self._device_tables(x.device, whiten)
        return feature_project(features, mean, comp, out_layout=out_layout)[0]

    def mahalanobis(self, features):
        """[Q] fp32: the squared Mahalanobis distance of rows [Q, 96] to the mean under the covariance restricted to its `rank` leading
        directions, sum_{j < rank} ((x - mean) . component_j)^2 / lambda_j; NaN for a row with a NaN channel.  Needs the components of
        all `rank` directions (fit_pca(n_components=None))."""
        x, _, _, _ = _source(features)
        if self.n_components < self.rank:
            raise ValueError(f"mahalanobis needs the {self.rank} leading components, this FeaturePCA keeps {self.n_components}")
        _require_cuda(x, "features")
        mean, comp = self._device_tables(x.device, True)
        return feature_project(features, mean, comp, out=False, sumsq=True)[1]


def _check_fit(features, n_components, ddof, rcond):
    src = _source(features)
    if n_components is not None and (not _is_int(n_components) or not 1 <= n_components <= DIM):
        raise ValueError(f"n_components must be None or an integer in [1, {DIM}], got {n_components!r}")
    if not _is_int(ddof) or ddof < 0:
        raise ValueError(f"ddof must be an integer >= 0, got {ddof!r}")
    if isinstance(rcond, bool) or not isinstance(rcond, (int, float)) or not 0 <= rcond < 1:
        raise ValueError(f"rcond must lie in [0, 1), got {rcond!r}")
    return src


def fit_pca(features, n_components=None, ddof=1, rcond=1e-6):
    """The principal components of frozen features.  Returns a FeaturePCA.
      features      a contiguous fp32 tensor [M, 96] on the device, a KnnBank, or an encode_scene map [Bs, 96, Hs, Ws] (or the
                    SceneEmbedding itself) read in place.  Rows with a channel that is not finite -- the pixels no window covers --
                    are skipped and not counted.
      n_components  how many leading directions to keep (None: all 96); the 96 eigenvalues are kept either way.
      ddof          the covariance divides by count - ddof.
      rcond         rank = the number of eigenvalues above rcond * the largest: what whitening and mahalanobis use.
    Four launches (the centred two-pass covariance) and ONE synchronisation, the read-back of count, mean and covariance; the
    eigendecomposition runs on the host in float64.  Eigenvalues descend and are clamped at 0; every component's entry of largest
    magnitude is positive (ties: the lowest index).  ValueError, before any device work, for a wrong rank, width, dtype, n_components,
    ddof or rcond, and after the read-back for fewer counted rows than ddof + 1; RuntimeError for CPU tensors.  No CPU or eager
    fallback."""
    x, _, _, _ = _check_fit(features, n_components, ddof, rcond)
    _require_cuda(x, "features")
    first = feature_moments(features, None, ddof, cov=False)
    buf = torch.empty(2 + DIM + DIM * DIM, dtype=torch.float32, device=x.device)
    feature_moments(features, first.mean, ddof, out=buf)
    host = buf.cpu()                               # the fit's one synchronisation
    count = int(host[:2].view(torch.int64)[0])
    if count < ddof + 1:
        raise ValueError(f"ddof = {ddof} needs at least {ddof + 1} rows without a NaN channel, got {count}")
    mean = host[2:2 + DIM].clone()
    cov = host[2 + DIM:].view(DIM, DIM).double().numpy()
    lam, comp = eigen_rules(cov)
    r = DIM if n_components is None else n_components
    c64 = np.ascontiguousarray(comp[:r])
    return FeaturePCA(mean.to(x.device), torch.from_numpy(c64).float().to(x.device), lam, count, rcond, _components64=c64, _covariance=cov)


def _check_pca(pca):
    if not isinstance(pca, FeaturePCA):
        raise ValueError(f"pca must be a FeaturePCA, got {type(pca).__name__}")


def pca_scene(model, scene, pca, stride=None, whiten=False, max_windows=None):
    """See ViTSpatialSpectral.pca_scene."""
    _check_pca(pca)

    def launch(emb, Bs, Hs, Ws):
        return PcaScene(pca.transform(emb.features, whiten=whiten, out_layout=1), emb.cover)

    return on_scene_map(model, scene, stride, False, max_windows, launch)


def anomaly_scene(model, scene, pca=None, stride=None, max_windows=None):
    """See ViTSpatialSpectral.anomaly_scene."""
    if pca is not None:
        _check_pca(pca)

    def launch(emb, Bs, Hs, Ws):
        p = fit_pca(emb.features) if pca is None else pca
        return AnomalyScene(p.mahalanobis(emb.features), emb.cover, p)

    return on_scene_map(model, scene, stride, False, max_windows, launch)
