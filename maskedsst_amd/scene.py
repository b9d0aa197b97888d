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

Windows at listed positions (``ViTSpatialSpectral.forward_at`` / ``predict_at``, ``msst_tokenize_at_fwd`` / ``_bwd``): the sampling
protocol of the reference's ``Houston2018Dataset`` (``src/data_houston2018.py``) on a sparsely labelled scene -- one window centred at
every labelled pixel, or windows at random positions -- with the windows read in place.  ``centre_origins``, ``random_origins`` and
``window_labels`` build the origin tables and the labels that go with them.  ``forward_at(..., scene_grad=True)`` also gives the scene its
gradient: listed windows overlap, so the per-window input gradients (``msst_tokenize_at_bwd_input``) are summed per pixel in a fixed order
(``msst_scene_fold_at``) through the inverse index ``origins_csr`` builds.

D4 augmentation (``forward_at(..., orient=)``, ``predict_at(..., tta="d4")``): every listed window may be read in one of its eight
orientations, code ``o = k + 4 f`` -- ``torch.rot90(torch.flip(w, (-1,)) if f else w, k, (-2, -1))`` -- where the kernels form the
window's address (``msst_tokenize_at_fwd_orient`` / ``_bwd_orient``): no oriented copy exists.  ``orient_windows`` is that expression
over a batch of windows (and its inverse, which maps patch-head logits back), ``random_orients`` draws codes, ``window_labels(...,
orient=)`` gives the label patches in the oriented frame.
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


def _check_labels(labels, window):
    if not torch.is_tensor(labels) or labels.dim() != 3:
        raise ValueError(f"labels must be a 3-D tensor [scenes, H, W], got {getattr(labels, 'shape', type(labels))}")
    if isinstance(window, bool) or int(window) != window or int(window) < 1:
        raise ValueError(f"window must be a positive integer, got {window!r}")
    return int(window)


def centre_origins(labels, window, ignore_index=-1):
    """The windows centred at the labelled pixels of label maps [Bs, Hs, Ws] (the reference's Houston2018Dataset(pixelwise=True),
    src/data_houston2018.py:248-255 and :303-317): every pixel (y, x) whose label is not ignore_index and whose window fits --
    y >= window // 2, y + window // 2 < Hs, likewise x -- gives the window with origin (y - window // 2, x - window // 2); for an
    even window the centre sits at index window // 2 of the window.  Returns (origins [n, 3] int32 = (scene, y0, x0), centre_labels
    [n] int64), on the labels' device, rows in the order of nonzero()."""
    window = _check_labels(labels, window)
    h = window // 2
    Hs, Ws = labels.shape[1:]
    idx = (labels != ignore_index).nonzero()
    ok = (idx[:, 1] >= h) & (idx[:, 1] + h < Hs) & (idx[:, 2] >= h) & (idx[:, 2] + h < Ws)
    idx = idx[ok]
    centre_labels = labels[idx[:, 0], idx[:, 1], idx[:, 2]].long()
    origins = torch.stack((idx[:, 0], idx[:, 1] - h, idx[:, 2] - h), dim=1).to(torch.int32)
    return origins, centre_labels


def window_labels(labels, origins, window, orient=None):
    """The label patches [n, window, window] (int64) of the windows listed in origins [n, 3] = (scene, y0, x0) out of label maps
    [Bs, Hs, Ws]: what a patch head trains against (:324).  A gather of labels only, on the labels' device.  orient [n] (codes 0 .. 7,
    any device): the patches in the oriented frame, ``orient_windows`` of them -- what ``forward_at(..., orient=orient)`` predicts."""
    window = _check_labels(labels, window)
    o = origins.to(labels.device).long()
    r = torch.arange(window, device=labels.device)
    ys = (o[:, 1, None] + r)[:, :, None]
    xs = (o[:, 2, None] + r)[:, None, :]
    patches = labels[o[:, 0, None, None], ys, xs].long()
    return patches if orient is None else orient_windows(patches, orient)


ORIENT_CODES = 8   # the dihedral group D4: code o = k + 4 f, k quarter turns counter-clockwise after f left-right flips


def _orient_index(s, device):
    """[8, s s] int64: row o holds, for every pixel of the oriented s x s window in row-major order, the row-major index of the pixel
    of the window as it lies that lands there -- the normative torch expression applied to the indices themselves"""
    w = torch.arange(s * s, device=device).view(s, s)
    return torch.stack([torch.rot90(torch.flip(w, (-1,)) if o >> 2 else w, o & 3, (-2, -1)).reshape(-1) for o in range(ORIENT_CODES)])


def orient_windows(x, orient, inverse=False):
    """The windows x [n, ..., s, s] (any dtype; the last two dimensions are the window) each in its orientation orient [n] (integer
    codes 0 .. 7 on any device): row i becomes ``torch.rot90(torch.flip(x[i], (-1,)) if f else x[i], k, (-2, -1))`` for
    ``orient[i] = k + 4 f``; code 0 is the identity.  inverse=True undoes it (oriented windows back to the frame of the scene: what
    maps the logits of a patch head under ``forward_at(..., orient=)`` back onto the window's pixels).  Eager torch -- one gather on
    x's device --, the restatement of what the kernels do in their addressing; a new tensor."""
    if not torch.is_tensor(x) or x.dim() < 3 or x.shape[-1] != x.shape[-2]:
        raise ValueError(f"x must be a tensor [n, ..., s, s] of square windows, got {getattr(x, 'shape', type(x))}")
    _check_orient(orient, x.shape[0])
    s = x.shape[-1]
    idx = _orient_index(s, x.device)
    if inverse:
        idx = torch.argsort(idx, dim=1)
    rows = idx[orient.to(x.device).long()]                                     # [n, s s]
    rows = rows.view((x.shape[0],) + (1,) * (x.dim() - 3) + (s * s,)).expand(x.shape[:-2] + (s * s,))
    return x.reshape(x.shape[:-2] + (s * s,)).gather(-1, rows).view(x.shape)


def random_orients(n, generator=None, device=None):
    """n orientation codes, uniform over 0 .. 7 -> uint8 [n], drawn with `generator` on its own device (the CPU without one) and
    moved to `device` when given"""
    if isinstance(n, bool) or int(n) != n or int(n) < 0:
        raise ValueError(f"n must be a non-negative integer, got {n!r}")
    dev = generator.device if generator is not None else torch.device("cpu")
    o = torch.randint(0, ORIENT_CODES, (int(n),), generator=generator, device=dev, dtype=torch.uint8)
    return o if device is None else o.to(device)


def random_origins(Bs, Hs, Ws, window, n, generator=None, labels=None, ignore_index=-1):
    """n windows at random positions (:319-329): scene uniform over Bs, origin uniform over [0, Hs - window] x [0, Ws - window].
    -> origins [n, 3] int32 on the labels' device (the CPU without labels), drawn with `generator` on its own device.  With labels
    [Bs, Hs, Ws] (the reference's drop_unlabeled, :326-327): a window that holds no pixel with a label other than ignore_index is
    drawn again -- only the rejected rows, in a loop, no recursion.  Raises ValueError when no window of the maps holds a labelled
    pixel (the loop would not end)."""
    if min(int(Bs), int(Hs), int(Ws), int(window)) < 1 or int(n) < 0 or window > Hs or window > Ws:
        raise ValueError(f"no {window} x {window} window in {Bs} scenes of {Hs} x {Ws}, or a negative count {n}")
    Bs, Hs, Ws, window, n = int(Bs), int(Hs), int(Ws), int(window), int(n)
    dev = generator.device if generator is not None else (labels.device if labels is not None else torch.device("cpu"))
    out_dev = labels.device if labels is not None else torch.device("cpu")

    def draw(k):
        cols = [torch.randint(0, hi, (k,), generator=generator, device=dev) for hi in (Bs, Hs - window + 1, Ws - window + 1)]
        return torch.stack(cols, dim=1).to(out_dev)

    origins = draw(n)
    if labels is not None:
        _check_labels(labels, window)
        if tuple(labels.shape) != (Bs, Hs, Ws):
            raise ValueError(f"labels {tuple(labels.shape)} are not [{Bs}, {Hs}, {Ws}]")
        if not bool((labels != ignore_index).any()):
            raise ValueError("no labelled pixel: every random window would be rejected")
        while n:
            empty = (window_labels(labels, origins, window) == ignore_index).flatten(1).all(dim=1).nonzero().flatten()
            if empty.numel() == 0:
                break
            origins[empty] = draw(empty.numel())
    return origins.to(torch.int32)


_INT_DTYPES = (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8)


def _check_orient(orient, n):
    """shape and dtype of an orientation table for n windows (no device needed, no value read)"""
    if not torch.is_tensor(orient) or orient.dim() != 1 or orient.shape[0] != n:
        raise ValueError(f"orient must be an integer tensor [{n}] of orientation codes 0 .. 7, one per window, got "
                         f"{getattr(orient, 'shape', type(orient))}")
    if orient.dtype not in _INT_DTYPES:
        raise ValueError(f"orient must be an integer tensor, got {orient.dtype}")


def _check_origins(model, scene, origins, check, orient=None):
    """forward_at / predict_at: shapes and dtypes (no device needed), then with check the value ranges -- one reduction, one read-back;
    orient (None: no table): its shape and dtype, and its range 0 .. 7 in that same read-back"""
    if not torch.is_tensor(scene) or scene.dim() != 4:
        raise ValueError(f"scene must be a 4-D tensor [scenes, bands, H, W], got {getattr(scene, 'shape', type(scene))}")
    bands = model.num_spectral_patches * model.patch_depth
    if scene.shape[1] != bands:
        raise ValueError(f"scene has {scene.shape[1]} bands, the model expects {bands}")
    w = model.num_spatial_patches_sqrt
    if scene.shape[0] < 1 or scene.shape[2] < w or scene.shape[3] < w:
        raise ValueError(f"scene {tuple(scene.shape)} is smaller than one {w} x {w} window")
    if not torch.is_tensor(origins) or origins.dim() != 2 or origins.shape[1] != 3:
        raise ValueError(f"origins must be an integer tensor [n, 3] of (scene, y0, x0), got {getattr(origins, 'shape', type(origins))}")
    if origins.dtype not in _INT_DTYPES:
        raise ValueError(f"origins must be an integer tensor, got {origins.dtype}")
    if orient is not None:
        _check_orient(orient, origins.shape[0])
    if check and origins.shape[0]:
        hi = (scene.shape[0] - 1, scene.shape[2] - w, scene.shape[3] - w)
        seen = torch.stack(torch.aminmax(origins, dim=0))
        if orient is not None:   # the codes' extremes ride along as a fourth column
            seen = torch.cat((seen.long(), torch.stack(torch.aminmax(orient.to(origins.device))).long()[:, None]), dim=1)
        lo_seen, hi_seen = (v.tolist() for v in seen.cpu())   # one reduction, the one read-back
        if orient is not None:
            lo_o, hi_o = lo_seen.pop(), hi_seen.pop()
            if lo_o < 0 or hi_o >= ORIENT_CODES:
                c = orient.cpu().long()   # the error path alone looks at the rows
                first = int(((c < 0) | (c >= ORIENT_CODES)).int().argmax())
                raise ValueError(f"orient[{first}] = {int(c[first])} is no orientation code: they are 0 .. {ORIENT_CODES - 1}")
        if min(lo_seen) < 0 or any(a > b for a, b in zip(hi_seen, hi)):
            o = origins.cpu()   # the error path alone looks at the rows
            first = int(((o < 0) | (o > torch.tensor(hi))).any(dim=1).int().argmax())
            raise ValueError(f"origins row {first} = {o[first].tolist()} is outside the scenes: (scene, y0, x0) must lie in "
                             f"[0, {hi[0]}] x [0, {hi[1]}] x [0, {hi[2]}]")


def origins_csr(origins, Bs, Hs, Ws):
    """The inverse index of an origins table [n, 3] = (scene, y0, x0) over origin cells, what ``msst_scene_fold_at`` finds the windows
    covering a pixel through: a window's cell is (scene * Hs + y0) * Ws + x0.  -> (cell_ptr int32 [Bs Hs Ws + 1], the CSR row pointers;
    cell_win int32 [n], the window numbers sorted by cell, ascending within a cell).  Torch ops on the table's device (a stable sort of
    the cell key, bincount, cumsum), no read-back; the rows must lie inside the scenes (``forward_at`` checks)."""
    o = origins.long()
    cells = int(Bs) * int(Hs) * int(Ws)
    key = (o[:, 0] * int(Hs) + o[:, 1]) * int(Ws) + o[:, 2]
    cell_win = torch.sort(key, stable=True).indices.to(torch.int32)
    cell_ptr = torch.zeros(cells + 1, dtype=torch.int32, device=o.device)
    cell_ptr[1:] = torch.cumsum(torch.bincount(key, minlength=cells)[:cells], dim=0)
    return cell_ptr, cell_win


def forward_at(model, scene, origins, check=True, scene_grad=False, orient=None):
    """See ViTSpatialSpectral.forward_at.  scene_grad may also be an ``engine.SceneGradSink`` (``saliency.scene_saliency``): the backward
    then folds into the sink's running map instead of handing autograd a gradient for the scene."""
    _check_origins(model, scene, origins, check, orient)
    wants = scene.requires_grad and torch.is_grad_enabled()
    if orient is not None and (scene_grad or wants):
        raise NotImplementedError("forward_at gives the scene no gradient through windows read with orient: the fold would need every "
                                  "window's inverse map -- detach the scene and drop scene_grad (parameter gradients are computed)")
    if wants and not scene_grad:
        raise NotImplementedError("forward_at gives no gradient for the scene unless asked: listed windows overlap, so d(loss)/d(scene) "
                                  "is an accumulating fold of the per-window input gradients -- pass scene_grad=True for it, or detach "
                                  "the scene (parameter gradients are computed)")
    eng = model.engine()
    eng._require_cuda(scene)
    from .engine import SceneGradSink, Windows
    table = origins.to(device=scene.device, dtype=torch.int32).contiguous()
    csr = sink = None
    if wants:
        Bs, _, Hs, Ws = scene.shape
        csr, sink = origins_csr(table, Bs, Hs, Ws), scene_grad if isinstance(scene_grad, SceneGradSink) else None
    if orient is not None:
        orient = orient.to(device=scene.device, dtype=torch.uint8).contiguous()
    return eng.classify_at(Windows("listed", scene, table, csr, sink, orient=orient))


def _forward_d4(model, scene, o, pix):
    """predict_at(tta="d4") on one chunk: the mean of the logits of every window of o over its eight orientations, the patch heads'
    mapped back onto the window's pixels first; summed in ascending code order"""
    total = None
    for code in range(ORIENT_CODES):
        codes = torch.full((o.shape[0],), code, dtype=torch.uint8, device=scene.device)
        out = forward_at(model, scene, o, check=False, orient=codes)
        out = out.reshape((o.shape[0], -1)) if pix else orient_windows(out, codes, inverse=True)
        total = out if total is None else total + out
    return total / ORIENT_CODES


def predict_at(model, scene, origins, return_logits=False, max_windows=SCENE_MAX_WINDOWS, orient=None, tta=None):
    """See ViTSpatialSpectral.predict_at."""
    if isinstance(max_windows, bool) or int(max_windows) != max_windows or int(max_windows) < 1:
        raise ValueError(f"max_windows must be a positive integer, got {max_windows!r}")
    if tta not in (None, "d4"):
        raise ValueError(f"tta must be None or 'd4', got {tta!r}")
    if tta is not None and orient is not None:
        raise ValueError("tta='d4' runs every window in all eight orientations: it takes no orient")
    _check_origins(model, scene, origins, True, orient)
    n, nc = origins.shape[0], model.num_classes
    w = model.num_spatial_patches_sqrt
    pix = bool(getattr(model, "pixelwise", False))
    step = int(max_windows)
    was_training = model.training
    if was_training:   # (a walk over every module each way: skipped for a model that is in eval() already)
        model.eval()
    try:
        with torch.no_grad():
            parts = []
            for i in range(0, n, step):
                o = origins[i:i + step]
                if tta is not None:
                    out = _forward_d4(model, scene, o, pix)
                else:
                    out = forward_at(model, scene, o, check=False, orient=None if orient is None else orient[i:i + step])
                parts.append(out.reshape((o.shape[0], nc) if pix else (o.shape[0], nc, w, w)))
            if parts:
                logits = torch.cat(parts) if len(parts) > 1 else parts[0]
            else:
                model.engine()._require_cuda(scene)
                logits = torch.empty((0, nc) if pix else (0, nc, w, w), dtype=torch.float32, device=scene.device)
            classes = logits.argmax(dim=1)
    finally:
        if was_training:
            model.train()
    return (classes, logits) if return_logits else classes


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
