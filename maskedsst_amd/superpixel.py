"""SLIC superpixels of feature maps and object-based class maps: the other classic spectral-spatial stage of hyperspectral land-cover
work.  The scene is segmented into superpixels (SLIC, Achanta et al. 2012, in its grid form, gSLICr), the per-pixel evidence of any
scene classifier is pooled per segment, and every pixel takes its segment's class.  It consumes what the other calls write: the
encode_scene map [Bs, 96, Hs, Ws] and the score maps [Bs, nc, Hs, Ws] of predict_scene, knn_predict_scene, probe_predict_scene and
gaussian_predict_scene.  A superpixel's mean feature is a row [96], so sp.centroids.reshape(-1, 96) feeds knn_classify,
LinearProbe.classify, GaussianClassifier.classify and KMeans.assign: 4096 rows instead of 262144 for a 512 x 512 scene at step 8.

    sp = fit_superpixels(features, cover=None, step=8, compactness=0.2, iters=10)   # a map [Bs, 96, Hs, Ws] or a SceneEmbedding
    sp.labels; sp.centroids; sp.positions; sp.counts; sp.history; sp.step; sp.grid
          # [Bs, Hs, Ws] int64 (-1 dead); [Bs, n_sp, 96]; [Bs, n_sp, 2] absolute (y, x) fp32; [Bs, n_sp] int32; [iters, 2] CPU; int; (gy, gx)
    table = superpixel_pool(sp, maps)                                                 # [Bs, n_sp, C], NaN for an empty superpixel
    res = superpixel_classify(sp, scores)      # ObjectResult(classes [Bs, Hs, Ws] int64, region_scores [Bs, n_sp, nc], region_classes [Bs, n_sp])
    res = model.superpixel_scene(scene, scores=None, embedding=None, stride=None, step=8, compactness=0.2, iters=10)
          # SuperpixelScene(superpixels, classes | None, region_scores | None, cover)

The contract:
    grid        step S in {4, 8, 16}; a scene has gy = ceil(Hs / S) by gx = ceil(Ws / S) cells; cell (i, j) owns rows [i S, min((i + 1) S,
                Hs)) and columns [j S, min((j + 1) S, Ws)); superpixel id = i gx + j, per scene; n_sp = gy gx.
    live        a pixel is live when its 96 features are finite and cover is None or > 0 there.  A dead pixel gets label -1 and
                contributes to no sum.  Nothing crosses the scene border; nothing passes between the scenes of a batch.
    candidates  a live pixel in cell (i, j) competes among the centres of cells (i + di, j + dj), di, dj in {-1, 0, 1}, that lie inside
                the grid and have count > 0.  So a centre's pixels always lie in its own 3 x 3 cells.
    score       s_c(p) = f_p . c_f + bias_c - hl |p - pos_c|^2: the dot is the fp32 fmaf chain over d = 0 .. 95 on the MFMA, bias_c =
                -0.5 x (the fp32 fmaf chain of c_f[d]^2 from zero), hl = 0.5 (compactness / S)^2 computed in float64 here and rounded
                once; argmax s = argmin |f_p - c_f|^2 + (compactness / S)^2 |p - pos_c|^2.  A centre's position is stored as an fp32
                offset from its own cell's origin, in [-S, 2 S); the pixel's displacement is formed from the integer cell difference plus
                that offset, so precision does not depend on where in a scene a cell lies.  ONE total order: score descending, then
                superpixel id ascending.  No candidate with rows: label -1 -- which happens to a dead pixel only.
    update      per centre the count, the feature sum / count and the offset sum / count (one IEEE division each) and the bias.  A centre
                without a pixel keeps centroid, offset and bias, gets count 0 and is never a candidate again (a cell that is dead from the
                start keeps the zeros it was created with).  Sums run in a fixed order that depends on (Hs, Ws, S) alone; no float
                atomics.
    fit         iteration 0 labels every live pixel with its home cell and updates; then `iters` times: assign, update.  history[t] =
                (moved, empty): the pixels whose label differs from the iteration before, the centres with count 0.  One
                synchronisation, to read the history.  After an iteration with moved == 0 the next reproduces every output bit for bit.
    pooling     for a map [Bs, C, Hs, Ws], C <= 128: table[b, k, c] = the mean over the pixels of superpixel k, a fixed-order sum and one
                division; NaN for a superpixel without pixels.  region_classes[b, k] = the argmax over c under the total order, -1 where
                the row is NaN.  A -inf score (a Gaussian class without rows) pools to -inf and is never chosen.
                classes[p] = region_classes[label[p]], -1 for a dead pixel.

The defaults (step 8, compactness 0.2, 10 iterations) are API defaults like kNN's temperature, not tuned on any data; compactness is in
feature units per step, 0.2 suits unit-length (normalize=True) maps.  The fit does not enforce connectivity: a superpixel may
consist of several pieces inside its 3 x 3 cells; maskedsst_amd.regions.enforce_connectivity is SLIC's relabelling pass, run afterwards.  Limits: feature width 96, step in {4, 8, 16}, at most
128 pooled channels, Hs, Ws <= 32768, fp32.  There is no CPU or eager fallback.
"""
import ctypes
import math
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .crf import _check_map
from .features import DIM, MAX_CLASSES, _is_int, _p, _stream, _require_cuda
from .scene import SceneEmbedding

STEPS = (4, 8, 16)
FIT_CHANNELS = 98         # include/msst.h: MSST_SLIC_FIT_CHANNELS
MAX_SIDE = 32768

Superpixels = namedtuple("Superpixels", ["labels", "centroids", "positions", "counts", "history", "step", "grid"])
ObjectResult = namedtuple("ObjectResult", ["classes", "region_scores", "region_classes"])
SuperpixelScene = namedtuple("SuperpixelScene", ["superpixels", "classes", "region_scores", "cover"])
# the centres as the kernels keep them: centroids [Bs, n_sp, 96], offsets [Bs, n_sp, 2] (from the cell's origin), bias [Bs, n_sp], counts int32
SlicCentres = namedtuple("SlicCentres", ["centroids", "offsets", "bias", "counts"])


def superpixel_grid(Hs, Ws, step):
    """(gy, gx): the cells of a scene"""
    return (Hs + step - 1) // step, (Ws + step - 1) // step


def slic_hl(compactness, step):
    """hl = 0.5 (compactness / S)^2 in float64, rounded to fp32 once"""
    with np.errstate(over="ignore"):
        return float(np.float32(0.5 * (float(compactness) / step) ** 2))


def _check_step(step):
    if not _is_int(step) or step not in STEPS:
        raise ValueError(f"step must be one of {STEPS}, got {step!r}")


def _check_compactness(c, step):
    if isinstance(c, bool) or not isinstance(c, (int, float)) or not math.isfinite(c) or c < 0 or not math.isfinite(slic_hl(c, step)):
        raise ValueError(f"compactness must be a finite number >= 0 (and 0.5 (compactness / step)^2 finite in fp32), got {c!r}")


def _check_features(features, cover):
    if isinstance(features, SceneEmbedding):
        features, cover = features.features, (features.cover if cover is None else cover)
    _check_map(features, "features", DIM)
    if features.shape[2] > MAX_SIDE or features.shape[3] > MAX_SIDE:
        raise ValueError(f"Hs and Ws must be at most {MAX_SIDE}, got {tuple(features.shape)}")
    if cover is not None:
        if not torch.is_tensor(cover) or cover.dtype != torch.int32 or tuple(cover.shape) != (features.shape[0],) + tuple(features.shape[2:]) \
                or not cover.is_contiguous():
            raise ValueError(f"cover must be None or a contiguous int32 tensor [Bs, Hs, Ws] matching the features, got "
                             f"{getattr(cover, 'shape', type(cover))}")
    return features, cover


def _check_labels(labels, shape, what="labels"):
    if not torch.is_tensor(labels) or labels.dtype != torch.int64 or tuple(labels.shape) != tuple(shape) or not labels.is_contiguous():
        raise ValueError(f"{what} must be a contiguous int64 tensor {list(shape)}, got {getattr(labels, 'shape', type(labels))}")


def _check_centres(centres, Bs, n_sp):
    if not isinstance(centres, SlicCentres):
        raise ValueError(f"centres must be a SlicCentres, got {type(centres).__name__}")
    want = dict(centroids=((Bs, n_sp, DIM), torch.float32), offsets=((Bs, n_sp, 2), torch.float32), bias=((Bs, n_sp), torch.float32),
                counts=((Bs, n_sp), torch.int32))
    for name, (shape, dtype) in want.items():
        t = getattr(centres, name)
        if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous():
            raise ValueError(f"centres.{name} must be a contiguous {dtype} tensor {list(shape)}, got {getattr(t, 'shape', type(t))}")


def _slab(Bs, Hs, Ws, step, C, device):
    n = _lib.load().msst_slic_scratch_floats(Bs, Hs, Ws, step, C)
    if n <= 0:
        raise ValueError(f"a map [{Bs}, {C}, {Hs}, {Ws}] at step {step} is outside what the SLIC kernels take")
    return torch.empty(n, dtype=torch.float32, device=device)


def new_centres(Bs, n_sp, device):
    """The centres before iteration 0: zeros, count 0"""
    return SlicCentres(torch.zeros(Bs, n_sp, DIM, dtype=torch.float32, device=device), torch.zeros(Bs, n_sp, 2, dtype=torch.float32, device=device),
                       torch.zeros(Bs, n_sp, dtype=torch.float32, device=device), torch.zeros(Bs, n_sp, dtype=torch.int32, device=device))


def superpixel_assign(features, cover, step, centres=None, hl=0.0, prev_labels=None, sums=True):
    """One msst_slic_assign launch on the current stream: (labels int64 [Bs, Hs, Ws], moved int32 [1] on the device or None, slab or
    None, best [Bs, Hs, Ws] fp32: the winning score, NaN for label -1 and in the home mode).  centres None is the home mode (iteration 0: every live pixel takes its own cell); otherwise a SlicCentres, and hl the fp32
    spatial weight (slic_hl).  With prev_labels (int64 [Bs, Hs, Ws]) the pixels whose label differs from it are counted.  sums: also
    write the per-block partial sums msst_slic_update reads."""
    features, cover = _check_features(features, cover)
    _check_step(step)
    Bs, _, Hs, Ws = features.shape
    gy, gx = superpixel_grid(Hs, Ws, step)
    if centres is not None:
        _check_centres(centres, Bs, gy * gx)
    if isinstance(hl, bool) or not isinstance(hl, (int, float)) or not math.isfinite(hl) or hl < 0:
        raise ValueError(f"hl must be a finite number >= 0, got {hl!r}")
    if prev_labels is not None:
        _check_labels(prev_labels, (Bs, Hs, Ws), "prev_labels")
    for t, what in ((features, "features"), (cover, "cover"), (prev_labels, "prev_labels")) + \
            (tuple(zip(centres, ("centroids", "offsets", "bias", "counts"))) if centres is not None else ()):
        if t is not None:
            _require_cuda(t, what)
    dev = features.device
    labels = torch.empty(Bs, Hs, Ws, dtype=torch.int64, device=dev)
    moved = torch.zeros(1, dtype=torch.int32, device=dev) if prev_labels is not None else None
    slab = _slab(Bs, Hs, Ws, step, FIT_CHANNELS, dev) if sums else None
    best = torch.empty(Bs, Hs, Ws, dtype=torch.float32, device=dev)
    c = centres if centres is not None else (None, None, None, None)
    _lib.check(_lib.load().msst_slic_assign(_p(features), _p(cover), Bs, DIM, Hs, Ws, step, float(hl), _p(c[0]), _p(c[1]), _p(c[2]), _p(c[3]),
                                            _p(labels), _p(prev_labels), _p(moved), _p(best), _p(slab), slab.numel() if sums else 0, _stream()),
               "msst_slic_assign")
    return labels, moved, slab, best


def superpixel_update(slab, shape, step, centres):
    """One msst_slic_update launch on the current stream: the centres (a SlicCentres, updated IN PLACE) from the slab of a
    superpixel_assign over a map of `shape` = (Bs, Hs, Ws); returns the number of empty centres, int32 [1] on the device."""
    _check_step(step)
    if len(shape) != 3 or not all(_is_int(v) and v >= 1 for v in shape):
        raise ValueError(f"shape must be (Bs, Hs, Ws), got {shape!r}")
    Bs, Hs, Ws = shape
    gy, gx = superpixel_grid(Hs, Ws, step)
    _check_centres(centres, Bs, gy * gx)
    if not torch.is_tensor(slab) or slab.dtype != torch.float32 or slab.dim() != 1 or not slab.is_contiguous():
        raise ValueError("slab must be the 1-D float32 slab of superpixel_assign")
    _require_cuda(slab, "slab")
    for t, what in zip(centres, ("centroids", "offsets", "bias", "counts")):
        _require_cuda(t, what)
    empty = torch.zeros(1, dtype=torch.int32, device=slab.device)
    _lib.check(_lib.load().msst_slic_update(_p(slab), slab.numel(), Bs, DIM, Hs, Ws, step, _p(centres.centroids), _p(centres.offsets),
                                            _p(centres.bias), _p(centres.counts), _p(empty), _stream()), "msst_slic_update")
    return empty


def _origins(gy, gx, step, device):
    iy = torch.arange(gy, dtype=torch.float32, device=device) * step
    ix = torch.arange(gx, dtype=torch.float32, device=device) * step
    return torch.stack(torch.meshgrid(iy, ix, indexing="ij"), dim=-1).reshape(1, gy * gx, 2)


def fit_superpixels(features, cover=None, step=8, compactness=0.2, iters=10):
    """SLIC superpixels of an encode_scene map: Superpixels(labels [Bs, Hs, Ws] int64, -1 dead; centroids [Bs, n_sp, 96]; positions
    [Bs, n_sp, 2] absolute (y, x) fp32; counts [Bs, n_sp] int32; history [iters, 2] int64 on the CPU, (moved, empty) per iteration;
    step; grid (gy, gx)); see the module's contract.  features: a map [Bs, 96, Hs, Ws] (fp32, contiguous, on the device) or a
    SceneEmbedding, whose cover is then used unless cover is given.  iters = 0 gives the home labels and the cell means.  2 (iters + 1)
    launches and one synchronisation, to read the history.  The defaults are API defaults, not tuned on data.  ValueError before any
    device work for wrong shapes, dtypes or ranges or a step outside {4, 8, 16}; RuntimeError for CPU tensors.  No CPU or eager
    fallback; connectivity is enforced afterwards, by enforce_connectivity."""
    features, cover = _check_features(features, cover)
    _check_step(step)
    _check_compactness(compactness, step)
    if not _is_int(iters) or iters < 0:
        raise ValueError(f"iters must be an integer >= 0, got {iters!r}")
    _require_cuda(features, "features")
    if cover is not None:
        _require_cuda(cover, "cover")
    Bs, _, Hs, Ws = features.shape
    gy, gx = superpixel_grid(Hs, Ws, step)
    dev = features.device
    hl = slic_hl(compactness, step)
    cen = new_centres(Bs, gy * gx, dev)
    labels = torch.empty(Bs, Hs, Ws, dtype=torch.int64, device=dev)
    slab = _slab(Bs, Hs, Ws, step, FIT_CHANNELS, dev)
    hist = torch.zeros(max(iters, 1), 2, dtype=torch.int32, device=dev)
    lib, st, null = _lib.load(), _stream(), ctypes.c_void_p(0)
    for t in range(iters + 1):
        c = (null,) * 4 if t == 0 else tuple(_p(v) for v in cen)
        moved = ctypes.c_void_p(hist.data_ptr() + 8 * (t - 1)) if t else null
        empty = ctypes.c_void_p(hist.data_ptr() + 8 * (t - 1) + 4) if t else null
        _lib.check(lib.msst_slic_assign(_p(features), _p(cover), Bs, DIM, Hs, Ws, step, hl, *c, _p(labels), _p(labels) if t else null, moved,
                                        null, _p(slab), slab.numel(), st), "msst_slic_assign")
        _lib.check(lib.msst_slic_update(_p(slab), slab.numel(), Bs, DIM, Hs, Ws, step, _p(cen.centroids), _p(cen.offsets), _p(cen.bias),
                                        _p(cen.counts), empty, st), "msst_slic_update")
    history = hist[:iters].cpu().long()               # the one synchronisation
    positions = cen.offsets + _origins(gy, gx, step, dev)
    return Superpixels(labels, cen.centroids, positions, cen.counts, history, step, (gy, gx))


def _check_sp(sp, maps, what):
    if not isinstance(sp, Superpixels):
        raise ValueError(f"superpixels must be a Superpixels (from fit_superpixels), got {type(sp).__name__}")
    _check_step(sp.step)
    _check_map(maps, what, max_channels=MAX_CLASSES)
    Bs, _, Hs, Ws = maps.shape
    if not torch.is_tensor(sp.labels) or tuple(sp.labels.shape) != (Bs, Hs, Ws):
        raise ValueError(f"{what} {tuple(maps.shape)} do not match the superpixels' Bs, Hs, Ws {tuple(getattr(sp.labels, 'shape', ()))}")
    _check_labels(sp.labels, (Bs, Hs, Ws), "the superpixels' labels")
    if tuple(sp.grid) != superpixel_grid(Hs, Ws, sp.step):
        raise ValueError(f"the superpixels' grid {sp.grid!r} is not that of a {Hs} x {Ws} scene at step {sp.step}")
    _require_cuda(maps, what)
    _require_cuda(sp.labels, "the superpixels' labels")


def _pool(sp, maps, classes):
    Bs, C, Hs, Ws = maps.shape
    n_sp = sp.grid[0] * sp.grid[1]
    dev = maps.device
    slab = _slab(Bs, Hs, Ws, sp.step, C, dev)
    table = torch.empty(Bs, n_sp, C, dtype=torch.float32, device=dev)
    region = torch.empty(Bs, n_sp, dtype=torch.int64, device=dev) if classes else None
    lib, st = _lib.load(), _stream()
    _lib.check(lib.msst_slic_pool(_p(maps), _p(sp.labels), Bs, C, Hs, Ws, sp.step, _p(slab), slab.numel(), st), "msst_slic_pool")
    _lib.check(lib.msst_slic_pool_finish(_p(slab), slab.numel(), Bs, C, Hs, Ws, sp.step, _p(table), _p(region), st), "msst_slic_pool_finish")
    if not classes:
        return table, None, None
    out = torch.empty(Bs, Hs, Ws, dtype=torch.int64, device=dev)
    _lib.check(lib.msst_slic_broadcast(_p(sp.labels), _p(region), Bs, Hs, Ws, sp.step, _p(out), st), "msst_slic_broadcast")
    return table, region, out


def superpixel_pool(superpixels, maps):
    """The per-superpixel means of a map [Bs, C, Hs, Ws] (fp32, contiguous, on the device, C <= 128): [Bs, n_sp, C], NaN for a
    superpixel without pixels; a fixed-order sum and one division, the same bits in every call.  Two launches, no synchronisation.
    ValueError before any device work for a map that does not match the superpixels' Bs, Hs, Ws; RuntimeError for CPU tensors."""
    _check_sp(superpixels, maps, "maps")
    return _pool(superpixels, maps, False)[0]


def superpixel_classify(superpixels, scores):
    """Object-based classification: the score maps [Bs, nc, Hs, Ws] of any scene classifier pooled per superpixel, and every pixel given
    its superpixel's class: ObjectResult(classes [Bs, Hs, Ws] int64, -1 dead; region_scores [Bs, n_sp, nc], NaN for an empty
    superpixel; region_classes [Bs, n_sp] int64, -1 for an empty one); see the module's contract.  Three launches, no synchronisation.
    ValueError before any device work for scores that do not match the superpixels' Bs, Hs, Ws; RuntimeError for CPU tensors."""
    _check_sp(superpixels, scores, "scores")
    table, region, classes = _pool(superpixels, scores, True)
    return ObjectResult(classes, table, region)


def superpixel_scene(model, scene, scores=None, embedding=None, stride=None, step=8, compactness=0.2, iters=10):
    """See ViTSpatialSpectral.superpixel_scene."""
    if embedding is not None and not isinstance(embedding, SceneEmbedding):
        raise ValueError(f"embedding must be None or a SceneEmbedding (from encode_scene), got {type(embedding).__name__}")
    if scores is not None:
        _check_map(scores, "scores", max_channels=MAX_CLASSES)
        if torch.is_tensor(scene) and scene.dim() == 4 and (scores.shape[0],) + tuple(scores.shape[2:]) != (scene.shape[0],) + tuple(scene.shape[2:]):
            raise ValueError(f"scores {tuple(scores.shape)} do not match the scene's Bs, Hs, Ws {tuple(scene.shape)}")
    _check_step(step)
    _check_compactness(compactness, step)
    if not _is_int(iters) or iters < 0:
        raise ValueError(f"iters must be an integer >= 0, got {iters!r}")
    if embedding is None:
        embedding = model.encode_scene(scene, stride=stride, normalize=True)
    sp = fit_superpixels(embedding, step=step, compactness=compactness, iters=iters)
    if scores is None:
        return SuperpixelScene(sp, None, None, embedding.cover)
    res = superpixel_classify(sp, scores)
    return SuperpixelScene(sp, res.classes, res.region_scores, embedding.cover)
