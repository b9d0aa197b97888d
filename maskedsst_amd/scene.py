"""Scene inference: apply a (finetuned) classifier to whole scenes with sliding windows.

Replaces the window loop of the reference's ``inference_example.ipynb`` and of ``validate_downstream``
(reference ``src/utils.py:497-541``): there every ``image_size`` window is a ``.narrow()`` copy and a ``model(window)``
call of its own.  Here ``ViTSpatialSpectral.predict_scene`` reads the windows of many scenes straight out of the scene
tensor in one tokenizer launch, runs them as one batch through the block kernels and assembles the per-window logits
into scene-shaped maps on the device (``include/msst.h``: ``msst_tokenize_scene_fwd``, ``msst_scene_assemble``).

Where this differs from the notebook: overlapping windows (``stride < image_size``) are averaged (mean of the logits of
every window covering a pixel), and pixels no window covers get class ``-1`` (the configs' ``ignored_label``) and logit 0.

A pixelwise model (``pixelwise=True``) predicts one class per window, for its centre pixel: its map is the dense per-pixel
map of DeepHyperX's ``test()`` (default stride 1, one window per pixel; ``msst_scene_centre_assemble``).  The border of
width ``image_size // 2``, and with a stride above 1 every pixel that is no window's centre, gets class ``-1`` and logit 0.

``ViTSpatialSpectral.encode_scene`` runs the same windows through the same encoder and stops before the head: per-pixel embedding
maps ``[Bs, 96, Hs, Ws]`` (``msst_pool_spectral_fwd``, ``msst_scene_embed_assemble``), NaN where no window covers a pixel.
"""
from collections import namedtuple

import torch
import torch.nn.functional as F

# windows per chunk of predict_scene: two token buffers of 2048 windows at the EnMAP shape (200 bands: 1280 tokens x 96 fp32
# per window) are 2 GB of HBM
SCENE_MAX_WINDOWS = 2048

SceneMetrics = namedtuple("SceneMetrics", ["loss", "acc", "macro_acc"])
SceneReport = namedtuple("SceneReport", ["loss", "acc", "macro_acc", "report"])
# what ViTSpatialSpectral.encode_scene returns: features [Bs, 96, Hs, Ws] fp32 (NaN where cover == 0), cover [Bs, Hs, Ws] int32
SceneEmbedding = namedtuple("SceneEmbedding", ["features", "cover"])


def scene_windows(Hs, Ws, window, stride):
    """Window origins (y0, x0) in the order the kernels number them: rows outer, columns inner, origins 0, stride, 2 stride, ...
    keeping only windows that fit (origin + window <= size) -- the notebook's loop."""
    return [(y0, x0) for y0 in range(0, Hs - window + 1, stride) for x0 in range(0, Ws - window + 1, stride)]


def _check_scene(model, scene, stride, max_windows):
    if not torch.is_tensor(scene) or scene.dim() != 4:
        raise ValueError(f"scene must be a 4-D tensor [scenes, bands, H, W], got {getattr(scene, 'shape', type(scene))}")
    bands = model.num_spectral_patches * model.patch_depth
    if scene.shape[1] != bands:
        raise ValueError(f"scene has {scene.shape[1]} bands, the model expects {bands}")
    w = model.num_spatial_patches_sqrt
    if scene.shape[0] < 1 or scene.shape[2] < w or scene.shape[3] < w:
        raise ValueError(f"scene {tuple(scene.shape)} is smaller than one {w} x {w} window")
    if stride is None:
        stride = 1 if getattr(model, "pixelwise", False) else w
    if isinstance(stride, bool) or int(stride) != stride or not 1 <= int(stride) <= w:
        raise ValueError(f"stride must be an integer in [1, {w}] (the window size), got {stride!r}")
    if isinstance(max_windows, bool) or int(max_windows) != max_windows or int(max_windows) < 1:
        raise ValueError(f"max_windows must be a positive integer, got {max_windows!r}")
    return int(stride), int(max_windows)


def predict_scene(model, scene, stride=None, return_logits=False, max_windows=SCENE_MAX_WINDOWS):
    """See ViTSpatialSpectral.predict_scene."""
    stride, max_windows = _check_scene(model, scene, stride, max_windows)
    with torch.no_grad():
        logits, classes = model.engine().scene_forward(scene, stride, max_windows)
    return (classes, logits) if return_logits else classes


def encode_scene(model, scene, stride=None, normalize=False, max_windows=SCENE_MAX_WINDOWS):
    """See ViTSpatialSpectral.encode_scene."""
    if stride is None:   # features are per position whatever the head: a pixelwise model's windows tile the scene too
        stride = model.num_spatial_patches_sqrt
    stride, max_windows = _check_scene(model, scene, stride, max_windows)
    features, cover = model.engine().encode_scene(scene, stride, bool(normalize), max_windows)
    return SceneEmbedding(features, cover)


def scene_metrics(logits, classes, labels, ignore_index=-1, fused=False):
    """Validation numbers of a predicted scene batch (what validate_downstream logs, src/utils.py:531-541, over whole scenes).

    logits [Bs, nc, Hs, Ws], classes [Bs, Hs, Ws] (-1: no window covers the pixel), labels [Bs, Hs, Ws].  Pixels count when
    they are covered and their label is not ignore_index.  Returns SceneMetrics(loss, acc, macro_acc):
      loss      cross entropy of the logits over those pixels (mean),
      acc       pixel accuracy over those pixels,
      macro_acc mean per-class recall over the classes present among those pixels' labels (torchmetrics' macro accuracy).
    All three are nan when no pixel counts.
    fused=True: one pass of ``maskedsst_amd.ops.cross_entropy_stats`` over the logit map as it lies, with ``skip=classes``, and one
    read-back of its record (the same integer counts; the loss summed in the kernels' fixed order) instead of the boolean
    indexing and the per-class loop below."""
    if fused:
        from .ops import cross_entropy_stats
        with torch.no_grad():
            _, stats = cross_entropy_stats(logits, labels, ignore_index, skip=classes)
        h = stats.host()
        return SceneMetrics(h.loss, h.acc, h.macro_acc)
    labels = labels.to(classes.device).long()
    valid = (classes != -1) & (labels != ignore_index)
    n = int(valid.sum())
    if n == 0:
        nan = float("nan")
        return SceneMetrics(nan, nan, nan)
    lab = labels[valid]
    pred = classes[valid].long()
    loss = F.cross_entropy(logits.float().permute(0, 2, 3, 1)[valid], lab)
    hit = pred == lab
    acc = hit.double().mean()
    present = torch.unique(lab)
    recall = torch.stack([hit[lab == c].double().mean() for c in present])
    return SceneMetrics(float(loss), float(acc), float(recall.mean()))


def scene_report(logits, classes, labels, ignore_index=-1):
    """``scene_metrics(..., fused=True)`` and the evaluation protocol of DeepHyperX (confusion matrix, overall and average accuracy,
    per-class precision / recall / F1 / IoU, Cohen's kappa) from ONE pass of ``maskedsst_amd.ops.cross_entropy_stats`` over the logit
    map as it lies, with ``skip=classes`` and ``confusion=True``: no boolean indexing, no ``bincount``, two read-backs (the record,
    the matrix).  The same pixels count as in ``scene_metrics``.  Returns SceneReport(loss, acc, macro_acc, report): the three
    numbers of ``scene_metrics`` (the same bits as its fused path) and ``report``, the ``maskedsst_amd.ops.ConfusionReport`` of the
    matrix (``report.total`` pixels; every rate nan when none counts).  The matrix itself: ``cross_entropy_stats(...,
    confusion=True)[1].confusion``.  At most 128 classes."""
    from .ops import confusion_report, cross_entropy_stats
    with torch.no_grad():
        _, stats = cross_entropy_stats(logits, labels, ignore_index, skip=classes, confusion=True)
    h = stats.host()
    return SceneReport(h.loss, h.acc, h.macro_acc, confusion_report(h.confusion))
