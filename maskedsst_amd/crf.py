"""Feature-guided CRF refinement of class maps: the spectral-spatial last stage of hyperspectral land-cover classification (SVM-MRF;
Kraehenbuehl and Koltun's dense CRF in its local form, ConvCRF, Teichmann and Cipolla 2018).  Every scene classifier of this package
labels a pixel alone; this stage lets neighbouring pixels that look alike to the encoder agree, which removes the salt-and-pepper
errors inside homogeneous fields.  It consumes what the other calls write: score maps [Bs, nc, Hs, Ws] (predict_scene's logits, the
probe's logits, the Gaussian log densities, the kNN votes) and the encode_scene feature map [Bs, 96, Hs, Ws].

    aff = crf_affinity(features, cover=None, radius=2, w_appearance=3.0, theta_feature=0.5, theta_position=2.0,
                       w_smooth=1.0, theta_smooth=1.0)       # features: a map [Bs, 96, Hs, Ws] or a SceneEmbedding
    aff.weights; aff.live; aff.radius                         # [Bs, K, Hs, Ws] fp32; [Bs, Hs, Ws] bool; int
    res = crf_refine(scores, aff, iters=5, unary="logits", unary_scale=1.0)
    res.classes; res.probs; res.history                       # [Bs, Hs, Ws] int64 (-1 dead); [Bs, nc, Hs, Ws] (NaN dead); [iters] CPU
    res = model.refine_scene(scene, scores, embedding=None, iters=5)     # RefinedScene(classes, probs, history, cover)

The contract (p a pixel, R the radius in 1 .. 3, the K = (2R+1)^2 - 1 offsets o = (dy, dx) numbered j = 0 .. K-1 with dy ascending,
then dx ascending, (0, 0) skipped; q = p + o):
    live       for the affinity: the 96 features are finite, their norm (formed in fp32) is greater than 0, cover is None or > 0;
               for the refinement also: no score is NaN and at least one is greater than -inf.  A dead pixel sends no message and
               receives none; its probabilities are NaN and its class is -1.
    affinity   k[p, j] = a[j] exp(-d2(p, q) g) + s[j] for p and q live and q inside p's scene, else exactly 0;
               d2 = max(0, 2 (1 - cos(f_p, f_q))), cos = dot(f_p, f_q) (rn_p rn_q), rn = 1 / |f| formed by the kernel -- a raw map and
               a normalize=True map both work; dot is the fp32 fmaf chain over d = 0 .. 95; g = 1 / (2 theta_feature^2);
               a[j] = w_appearance exp(-|o_j|^2 / (2 theta_position^2)), s[j] = w_smooth exp(-|o_j|^2 / (2 theta_smooth^2)), computed
               here in float64 and rounded to fp32 once.  The cosine form is chosen because |f_p|^2 + |f_q|^2 - 2 f_p . f_q cancels
               in fp32 exactly at like neighbours.  k[p, j] and k[q, opposite j] have the same bits.
    refinement U[c, p] = unary_scale scores[c, p] ("logits") or unary_scale log(max(v, 1e-30)) ("votes"); Q_0 = softmax_c(U);
               Q_{t+1}[c, p] = softmax_c(U[c, p] + sum_j k[p, j] Q_t[c, q_j]) (Potts compatibility), the sum one fp32 fmaf chain in j
               order, the softmax with the maximum subtracted.  A class whose score is -inf has probability 0 throughout.  The
               message is NOT normalised by sum_j k: a border pixel has fewer neighbours and is smoothed less.
    classes    the argmax of the last Q under the project's one total order: value descending, then class index ascending.
    history    history[t] = the live pixels whose class after step t + 1 differs from the one after step t.

The defaults are API defaults like kNN's temperature, not tuned on any data.  A refinement enqueues iters + 1 launches of
msst_crf_step between two buffers and synchronises once, to read the history.  The affinity is computed once per scene batch
(msst_crf_affinity) and serves every classifier's scores.  Limits: feature width 96, radius <= 3, at most 128 classes, fp32; scores of
+inf are outside the contract.  There is no CPU or eager fallback.
"""
import ctypes
import math
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .features import DIM, MAX_CLASSES, _is_int, _p, _stream, _require_cuda
from .scene import SceneEmbedding

MAX_RADIUS = 3
UNARY = {"logits": 0, "votes": 1}

# weights [Bs, K, Hs, Ws] fp32, live [Bs, Hs, Ws] bool, radius
CrfAffinity = namedtuple("CrfAffinity", ["weights", "live", "radius"])
# classes [Bs, Hs, Ws] int64 (-1: dead), probs [Bs, nc, Hs, Ws] fp32 (NaN: dead), history [iters] int64 on the CPU
CrfResult = namedtuple("CrfResult", ["classes", "probs", "history"])
RefinedScene = namedtuple("RefinedScene", ["classes", "probs", "history", "cover"])


def crf_offsets(radius):
    """The K neighbour offsets (dy, dx) in the kernels' order"""
    r = range(-radius, radius + 1)
    return [(dy, dx) for dy in r for dx in r if (dy, dx) != (0, 0)]


def _positive(v, what, zero=False):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0 or (v == 0 and not zero):
        raise ValueError(f"{what} must be a finite number {'>= 0' if zero else '> 0'}, got {v!r}")
    return float(v)


def crf_tables(radius, w_appearance=3.0, theta_position=2.0, w_smooth=1.0, theta_smooth=1.0):
    """(a [K], s [K]) fp32 numpy: the position tables of the affinity, computed in float64 and rounded once"""
    if not _is_int(radius) or not 1 <= radius <= MAX_RADIUS:
        raise ValueError(f"radius must be an integer in [1, {MAX_RADIUS}], got {radius!r}")
    wa, ws = _positive(w_appearance, "w_appearance", True), _positive(w_smooth, "w_smooth", True)
    tp, ts = _positive(theta_position, "theta_position"), _positive(theta_smooth, "theta_smooth")
    o2 = np.array([dy * dy + dx * dx for dy, dx in crf_offsets(radius)], dtype=np.float64)
    return (wa * np.exp(-o2 / (2.0 * tp * tp))).astype(np.float32), (ws * np.exp(-o2 / (2.0 * ts * ts))).astype(np.float32)


def _check_map(t, what, channels=None, max_channels=None):
    if not torch.is_tensor(t) or t.dim() != 4 or (channels is not None and t.shape[1] != channels) or min(t.shape) < 1 or \
            (max_channels is not None and t.shape[1] > max_channels):
        want = channels if channels is not None else f"nc <= {max_channels}"
        raise ValueError(f"{what} must be a 4-D tensor [Bs, {want}, Hs, Ws], got {getattr(t, 'shape', type(t))}")
    if t.dtype != torch.float32:
        raise ValueError(f"{what} must be float32, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous")


def affinity_launch(features, cover, radius, a, s, g):
    """msst_crf_affinity on the current stream with the tables as given (a, s: [K] float sequences, taken as they are): CrfAffinity"""
    K = (2 * radius + 1) ** 2 - 1
    Bs, _, Hs, Ws = features.shape
    at = (ctypes.c_float * K)(*[float(v) for v in a])
    st = (ctypes.c_float * K)(*[float(v) for v in s])
    weights = torch.empty(Bs, K, Hs, Ws, dtype=torch.float32, device=features.device)
    live = torch.empty(Bs, Hs, Ws, dtype=torch.bool, device=features.device)
    _lib.check(_lib.load().msst_crf_affinity(_p(features), _p(cover), Bs, DIM, Hs, Ws, radius, ctypes.cast(at, ctypes.c_void_p),
                                             ctypes.cast(st, ctypes.c_void_p), float(g), _p(weights), _p(live), _stream()), "msst_crf_affinity")
    return CrfAffinity(weights, live, radius)


def crf_affinity(features, cover=None, radius=2, w_appearance=3.0, theta_feature=0.5, theta_position=2.0, w_smooth=1.0, theta_smooth=1.0):
    """The pairwise weights of the CRF from an encode_scene map: CrfAffinity(weights [Bs, K, Hs, Ws], live [Bs, Hs, Ws], radius); see
    the module's contract.  features: a map [Bs, 96, Hs, Ws] (fp32, contiguous, on the device; raw or normalised) or a SceneEmbedding,
    whose cover is then used unless cover is given.  cover: None or [Bs, Hs, Ws] int32, a pixel with cover <= 0 is dead.  One launch;
    computed once, it serves every classifier's scores.  The defaults are API defaults, not tuned on data.  ValueError before any
    device work for wrong shapes, dtypes or ranges; RuntimeError for CPU tensors.  No CPU or eager fallback."""
    if isinstance(features, SceneEmbedding):
        features, cover = features.features, (features.cover if cover is None else cover)
    _check_map(features, "features", DIM)
    if cover is not None:
        if not torch.is_tensor(cover) or cover.dtype != torch.int32 or tuple(cover.shape) != (features.shape[0],) + tuple(features.shape[2:]) \
                or not cover.is_contiguous():
            raise ValueError(f"cover must be None or a contiguous int32 tensor [Bs, Hs, Ws] matching the features, got "
                             f"{getattr(cover, 'shape', type(cover))}")
    a, s = crf_tables(radius, w_appearance, theta_position, w_smooth, theta_smooth)
    tf = _positive(theta_feature, "theta_feature")
    g = 1.0 / (2.0 * tf * tf)
    if g > 3.4028234e38:
        raise ValueError(f"theta_feature = {theta_feature!r} is too small for fp32")
    _require_cuda(features, "features")
    if cover is not None:
        _require_cuda(cover, "cover")
    return affinity_launch(features, cover, radius, a, s, g)


def crf_step(scores, aff, q_in=None, unary="logits", unary_scale=1.0, classes=False, prev_classes=None):
    """One msst_crf_step launch on the current stream: (q_out [Bs, nc, Hs, Ws], classes int32 [Bs, Hs, Ws] or None, changed int32 [1]
    on the device or None).  q_in None gives step 0, softmax(U).  With prev_classes (int32 [Bs, Hs, Ws]) the live pixels whose class
    differs from it are counted."""
    _check_refine(scores, aff, 0, unary, unary_scale)
    if q_in is not None:
        _check_map(q_in, "q_in")
        if q_in.shape != scores.shape:
            raise ValueError(f"q_in must have the shape of the scores {tuple(scores.shape)}, got {tuple(q_in.shape)}")
    Bs, nc, Hs, Ws = scores.shape
    if prev_classes is not None and (not torch.is_tensor(prev_classes) or prev_classes.dtype != torch.int32 or
                                     tuple(prev_classes.shape) != (Bs, Hs, Ws) or not prev_classes.is_contiguous()):
        raise ValueError("prev_classes must be None or a contiguous int32 tensor [Bs, Hs, Ws]")
    for t, what in ((scores, "scores"), (aff.weights, "the affinity"), (q_in, "q_in"), (prev_classes, "prev_classes")):
        if t is not None:
            _require_cuda(t, what)
    q_out = torch.empty_like(scores)
    cls = torch.empty(Bs, Hs, Ws, dtype=torch.int32, device=scores.device) if classes or prev_classes is not None else None
    changed = torch.zeros(1, dtype=torch.int32, device=scores.device) if prev_classes is not None else None
    _lib.check(_lib.load().msst_crf_step(_p(scores), UNARY[unary], float(unary_scale), _p(q_in), _p(aff.weights), _p(aff.live), Bs, nc, Hs, Ws,
                                         aff.radius, _p(q_out), _p(cls), _p(prev_classes), _p(changed), _stream()), "msst_crf_step")
    return q_out, cls, changed


def _check_refine(scores, aff, iters, unary, unary_scale):
    if not isinstance(aff, CrfAffinity):
        raise ValueError(f"affinity must be a CrfAffinity (from crf_affinity), got {type(aff).__name__}")
    _check_map(scores, "scores", max_channels=MAX_CLASSES)
    if not _is_int(aff.radius) or not 1 <= aff.radius <= MAX_RADIUS:
        raise ValueError(f"the affinity's radius must be an integer in [1, {MAX_RADIUS}], got {aff.radius!r}")
    K = (2 * aff.radius + 1) ** 2 - 1
    Bs, _, Hs, Ws = scores.shape
    _check_map(aff.weights, "the affinity's weights", K)
    if not torch.is_tensor(aff.live) or aff.live.dtype != torch.bool or not aff.live.is_contiguous():
        raise ValueError("the affinity's live map must be a contiguous bool tensor")
    if tuple(aff.weights.shape) != (Bs, K, Hs, Ws) or tuple(aff.live.shape) != (Bs, Hs, Ws):
        raise ValueError(f"the scores {tuple(scores.shape)} do not match the affinity's Bs, Hs, Ws {tuple(aff.live.shape)}")
    if not _is_int(iters) or iters < 0:
        raise ValueError(f"iters must be an integer >= 0, got {iters!r}")
    if unary not in UNARY:
        raise ValueError(f"unary must be 'logits' or 'votes', got {unary!r}")
    _positive(unary_scale, "unary_scale")


def crf_refine(scores, affinity, iters=5, unary="logits", unary_scale=1.0):
    """`iters` mean-field steps on score maps [Bs, nc, Hs, Ws] (fp32, contiguous, on the device) under a CrfAffinity of the same Bs, Hs,
    Ws: CrfResult(classes [Bs, Hs, Ws] int64, -1 dead; probs [Bs, nc, Hs, Ws], NaN dead; history [iters] int64 on the CPU); see the
    module's contract.  unary: "logits" (logits, probe logits, Gaussian log densities) or "votes" (the kNN vote map).  iters = 0
    returns softmax(U) and its argmax.  The message is not normalised by sum_j k: border pixels are smoothed less.  iters + 1 launches
    between two buffers and one synchronisation, to read the history.  The defaults are API defaults, not tuned on data.  ValueError
    before any device work for wrong shapes, dtypes, ranges or scores that do not match the affinity; RuntimeError for CPU tensors.
    No CPU or eager fallback."""
    _check_refine(scores, affinity, iters, unary, unary_scale)
    _require_cuda(scores, "scores")
    _require_cuda(affinity.weights, "the affinity")
    _require_cuda(affinity.live, "the affinity")
    Bs, nc, Hs, Ws = scores.shape
    dev = scores.device
    bufs = [torch.empty_like(scores), torch.empty_like(scores) if iters else None]
    classes = torch.empty(Bs, Hs, Ws, dtype=torch.int32, device=dev)
    changed = torch.zeros(max(iters, 1), dtype=torch.int32, device=dev)
    lib, st = _lib.load(), _stream()
    for t in range(iters + 1):
        q_in, q_out = (bufs[(t - 1) & 1] if t else None), bufs[t & 1]
        cnt = ctypes.c_void_p(changed.data_ptr() + 4 * (t - 1)) if t else ctypes.c_void_p(0)
        _lib.check(lib.msst_crf_step(_p(scores), UNARY[unary], float(unary_scale), _p(q_in), _p(affinity.weights), _p(affinity.live), Bs, nc,
                                     Hs, Ws, affinity.radius, _p(q_out), _p(classes), _p(classes) if t else ctypes.c_void_p(0), cnt, st),
                   "msst_crf_step")
    history = changed[:iters].cpu().long()            # the one synchronisation
    return CrfResult(classes.long(), bufs[iters & 1], history)


def refine_scene(model, scene, scores, embedding=None, stride=None, iters=5, unary="logits", unary_scale=1.0, **affinity_kwargs):
    """See ViTSpatialSpectral.refine_scene."""
    if embedding is not None and not isinstance(embedding, SceneEmbedding):
        raise ValueError(f"embedding must be None or a SceneEmbedding (from encode_scene), got {type(embedding).__name__}")
    _check_map(scores, "scores", max_channels=MAX_CLASSES)
    if not _is_int(iters) or iters < 0:
        raise ValueError(f"iters must be an integer >= 0, got {iters!r}")
    if unary not in UNARY:
        raise ValueError(f"unary must be 'logits' or 'votes', got {unary!r}")
    _positive(unary_scale, "unary_scale")
    if embedding is None:
        embedding = model.encode_scene(scene, stride=stride, normalize=True)
    aff = crf_affinity(embedding, **affinity_kwargs)
    res = crf_refine(scores, aff, iters, unary, unary_scale)
    return RefinedScene(res.classes, res.probs, res.history, embedding.cover)
