"""The linear probe on cached features: the third standard way to judge a frozen self-supervised encoder (the protocol the SimMIM
and MAE papers report), beside nearest class mean (finetune.py --val-embed) and weighted kNN (maskedsst_amd.knn).  The labelled
pixels are encoded ONCE; the classifier head -- LayerNorm(96) -> Linear(96 -> n_classes), exactly ``mlp_head`` of the patch-head
model -- is then trained on the cached rows for as many steps as one likes, instead of running the frozen body on every step as
``linear_eval`` does.

    bank  = probe_bank(model, scenes, labels, per_class=2000)      # KnnBank of RAW features: encode_scene(normalize=False)
    probe = fit_linear_probe(bank, steps=500, lr=1e-2)             # LinearProbe; probe.history [steps, 4] (CPU), one read-back
    probe.logits(features); probe.classify(features)               # rows [Q, 96]
    res = model.probe_predict_scene(scene, probe)                  # ProbeScene(classes, logits, cover)
    probe.load_into(model); LinearProbe.from_model(model)          # <-> model.mlp_head

Three calls of ``libmsst.so`` (``maskedsst_amd/csrc/msst_probe.hip``, ``include/msst.h``).  A step is two launches:
``msst_probe_grad`` streams the bank once (LayerNorm, logits on the fp32 matrix cores, softmax, the gradient partials of every
workgroup) and ``msst_probe_update`` sums the partials in a fixed order and applies ``torch.optim.Adam`` with the step count kept on
the device.  A fit enqueues ``2 * steps`` launches and synchronises once, to read the history.  The parameters are one vector
``theta = [gamma 96 | beta 96 | W nc x 96 | b nc]``, the layout of the flat buffer's ``mlp_head`` segment, so ``inplace=model``
trains a model's head where it lies.  No atomics: two fits from the same inputs give the same bits.  There is no CPU or eager
fallback.
"""
import ctypes
import math
from collections import namedtuple

import torch

from . import _lib
from .features import DIM, MAX_CLASSES, KnnBank, _bank_from_scenes, _is_int, _p, _stream, _require_cuda, check_rows, on_scene_map

# classes [Bs, Hs, Ws] int64 (-1 where no window covers the pixel), logits [Bs, n_classes, Hs, Ws] fp32 (NaN there), cover [Bs, Hs, Ws] int32
ProbeScene = namedtuple("ProbeScene", ["classes", "logits", "cover"])
HISTORY = ("loss", "weight_sum", "correct", "rows")   # the columns of LinearProbe.history


def n_params(n_classes):
    return 2 * DIM + (DIM + 1) * n_classes


def slice_walk(M, batch, steps):
    """[(row0, rows)] of the steps of a fit over a bank of M rows: batch None (or >= M) -- every step sees the whole bank; otherwise
    step t takes the next contiguous slice of `batch` rows, the last slice of a pass is the partial remainder, and the walk then
    wraps to row 0."""
    if batch is None or batch >= M:
        return [(0, M)] * steps
    out, row0 = [], 0
    for _ in range(steps):
        rows = min(batch, M - row0)
        out.append((row0, rows))
        row0 = 0 if row0 + rows >= M else row0 + rows
    return out


def _is_num(v):
    return not isinstance(v, bool) and isinstance(v, (int, float)) and math.isfinite(v)


def _patch_head(model, n_classes, what):
    from .vit_spatial_spectral import ViTSpatialSpectral
    if not isinstance(model, ViTSpatialSpectral):
        raise ValueError(f"{what} needs a ViTSpatialSpectral, got {type(model).__name__}")
    if model.pixelwise or model.spectral_mlp_head:
        raise ValueError(f"{what} takes the patch head only (LayerNorm(96) -> Linear(96 -> n_classes)): not pixelwise, not spectral_mlp_head")
    if n_classes is not None and int(model.num_classes) != n_classes:
        raise ValueError(f"{what}: the model has {model.num_classes} classes, the probe {n_classes}")
    return [model.mlp_head[0].weight, model.mlp_head[0].bias, model.mlp_head[1].weight, model.mlp_head[1].bias]


class LinearProbe:
    """A trained (or initial) head: theta [192 + 97 n_classes] fp32 on the device = gamma | beta | W | b, Adam's moments m and v, the
    device-side step counter and, after a fit, history [steps, 4] on the CPU: per step the loss, the weight sum, the number of rows
    whose argmax equals the label and the number of rows, of the parameters as they were BEFORE that step's update (a skipped step --
    weight sum 0 -- has loss NaN)."""

    def __init__(self, theta, n_classes, m=None, v=None, step=None, history=None):
        if not _is_int(n_classes) or not 1 <= n_classes <= MAX_CLASSES:
            raise ValueError(f"n_classes must be an integer in [1, {MAX_CLASSES}], got {n_classes!r}")
        if not torch.is_tensor(theta) or theta.dtype != torch.float32 or theta.shape != (n_params(n_classes),) or not theta.is_contiguous():
            raise ValueError(f"theta must be a contiguous float32 tensor [{n_params(n_classes)}], got {getattr(theta, 'shape', type(theta))}")
        for t in (m, v):
            if t is not None and (not torch.is_tensor(t) or t.dtype != torch.float32 or t.shape != theta.shape or not t.is_contiguous()):
                raise ValueError("m and v must be contiguous float32 tensors of theta's shape")
        self.theta = theta
        self.n_classes = n_classes
        self.m = torch.zeros_like(theta) if m is None else m
        self.v = torch.zeros_like(theta) if v is None else v
        self.step = torch.zeros(_lib.PROBE_STEP_INTS, dtype=torch.int32, device=theta.device) if step is None else step
        self.history = history

    # ---- the four parameters as views of theta
    @property
    def gamma(self):
        return self.theta[:DIM]

    @property
    def beta(self):
        return self.theta[DIM:2 * DIM]

    @property
    def weight(self):
        return self.theta[2 * DIM:2 * DIM + DIM * self.n_classes].view(self.n_classes, DIM)

    @property
    def bias(self):
        return self.theta[2 * DIM + DIM * self.n_classes:]

    @property
    def steps_applied(self):
        return int(self.step[0])

    def clone(self):
        return LinearProbe(self.theta.clone(), self.n_classes, self.m.clone(), self.v.clone(), self.step.clone(), self.history)

    def _forward(self, features):
        check_rows(features, "features", 1, shape=f"[Q, {DIM}] with Q >= 1")
        _require_cuda(features, "features")
        _require_cuda(self.theta, "the probe")
        Q = features.shape[0]
        logits = torch.empty(Q, self.n_classes, dtype=torch.float32, device=features.device)
        classes = torch.empty(Q, dtype=torch.int64, device=features.device)
        probe_forward(self, features, 0, Q, 1, logits, 0, classes)
        return logits, classes

    def logits(self, features):
        """logits [Q, n_classes] of rows [Q, 96] (fp32, contiguous, on the device); a row with a NaN channel gets NaN logits"""
        return self._forward(features)[0]

    def classify(self, features):
        """classes [Q] int64, the argmax with ties to the lowest class; -1 for a row with a NaN channel"""
        return self._forward(features)[1]

    def load_into(self, model):
        """Copy the probe into model.mlp_head (the patch head with this many classes only: ValueError otherwise) in place under
        no_grad: the parameters stay the views of the flat buffer they were, so a warm engine computes with the new head at once."""
        params = _patch_head(model, self.n_classes, "load_into")
        with torch.no_grad():
            for p, src in zip(params, (self.gamma, self.beta, self.weight, self.bias)):
                p.copy_(src.to(p.device))
        return model

    @classmethod
    def from_model(cls, model):
        """The model's mlp_head (the patch head only) as a LinearProbe with zero moments: a copy, bit for bit."""
        params = _patch_head(model, None, "from_model")
        theta = torch.cat([p.detach().reshape(-1).float() for p in params]).contiguous()
        return cls(theta, int(model.num_classes))


def probe_forward(probe, x, x_layout, Q, plane, logits, out_layout, classes):
    """msst_probe_fwd on the current stream: x is rows [Q, 96] (x_layout 0) or a map [Bs, 96, plane] (x_layout 1) read in place"""
    lib = _lib.load()
    _lib.check(lib.msst_probe_fwd(_p(x), x_layout, Q, plane, _p(probe.theta), DIM, probe.n_classes, _p(logits), out_layout, _p(classes),
                                  _stream()), "msst_probe_fwd")


def _check_bank(bank):
    if not isinstance(bank, KnnBank):
        raise ValueError(f"bank must be a KnnBank (probe_bank builds one of raw features), got {type(bank).__name__}")


def _check_class_weights(class_weights, nc):
    """-> a CPU float32 tensor [nc] or None"""
    if class_weights is None:
        return None
    try:
        w = torch.as_tensor(class_weights).detach().cpu()
    except (TypeError, ValueError, RuntimeError) as e:
        raise ValueError(f"class_weights must be {nc} numbers") from e
    if w.dtype == torch.bool or w.is_complex() or w.shape != (nc,):
        raise ValueError(f"class_weights must be {nc} numbers, got shape {tuple(w.shape)} of {w.dtype}")
    w = w.to(torch.float64)
    if not bool(torch.isfinite(w).all()) or bool((w < 0).any()) or not bool((w > 0).any()):
        raise ValueError("class_weights must be finite and >= 0, with at least one above 0")
    return w.to(torch.float32)


def _check_hyper(steps, lr, betas, eps, weight_decay, batch):
    if not _is_int(steps) or steps < 1:
        raise ValueError(f"steps must be an integer >= 1, got {steps!r}")
    if _is_num(lr):
        lrs = [float(lr)] * steps
    else:
        try:
            lrs = list(lr)
        except TypeError as e:
            raise ValueError(f"lr must be a number or a sequence of {steps} numbers, got {lr!r}") from e
        if len(lrs) != steps or not all(_is_num(x) for x in lrs):
            raise ValueError(f"lr must be a number or a sequence of {steps} finite numbers")
        lrs = [float(x) for x in lrs]
    if any(x < 0 for x in lrs):
        raise ValueError("lr must be >= 0")
    if not isinstance(betas, (tuple, list)) or len(betas) != 2 or not all(_is_num(b) and 0 <= b < 1 for b in betas):
        raise ValueError(f"betas must be two numbers in [0, 1), got {betas!r}")
    if not _is_num(eps) or eps < 0:
        raise ValueError(f"eps must be a number >= 0, got {eps!r}")
    if not _is_num(weight_decay) or weight_decay < 0:
        raise ValueError(f"weight_decay must be a number >= 0, got {weight_decay!r}")
    if batch is not None and (not _is_int(batch) or batch < 1):
        raise ValueError(f"batch must be None or an integer >= 1, got {batch!r}")
    return lrs


def _head_segment(model, nc):
    """the mlp_head segment of the model's flat parameter buffer as one view [192 + 97 nc]: gamma | beta | W | b back to back"""
    eng = model.engine()
    eng.ensure()
    fp = eng.fp
    names = [f"mlp_head.{i}.{wb}" for i in (0, 1) for wb in ("weight", "bias")]
    if any(n not in fp.segments for n in names):
        raise ValueError("inplace: the model's flat buffer has no mlp_head segment")
    off = fp.segments[names[0]][0]
    at = off
    for nme in names:
        o, k, _ = fp.segments[nme]
        if o != at:
            raise ValueError("inplace: the mlp_head parameters do not lie back to back in the flat buffer")
        at += k
    if at - off != n_params(nc):
        raise ValueError("inplace: the mlp_head segment has the wrong size")
    return fp.flat[off:at]


def probe_gradient(bank, probe, row0=0, rows=None, class_weights=None):
    """One msst_probe_grad launch on rows [row0, row0 + rows) of the bank and its reduction (msst_probe_update with apply = 0: nothing is
    updated): (gradient [192 + 97 n_classes] on the device = d loss / d (gamma | beta | W | b) of the weighted-mean cross entropy, row [4]
    on the device = loss, weight sum, correct, rows)."""
    _check_bank(bank)
    if not isinstance(probe, LinearProbe) or probe.n_classes != bank.n_classes:
        raise ValueError("probe must be a LinearProbe with the bank's n_classes")
    M = len(bank)
    rows = M - row0 if rows is None else rows
    if not _is_int(row0) or not _is_int(rows) or row0 < 0 or rows < 1 or row0 + rows > M:
        raise ValueError(f"rows [{row0}, {row0} + {rows}) do not lie in the bank of {M}")
    cw = _check_class_weights(class_weights, bank.n_classes)
    _require_cuda(bank.features, "the bank's features")
    _require_cuda(probe.theta, "the probe")
    lib = _lib.load()
    dev = bank.features.device
    cw = None if cw is None else cw.to(dev)
    nslab = int(lib.msst_probe_scratch_floats(rows, bank.n_classes))
    slab = torch.full((nslab,), float("nan"), dtype=torch.float32, device=dev)
    grad = torch.full_like(probe.theta, float("nan"))
    row = torch.full((4,), float("nan"), dtype=torch.float32, device=dev)
    st = _stream()
    _lib.check(lib.msst_probe_grad(_p(bank.features), _p(bank.labels), _p(cw), _p(probe.theta), M, DIM, row0, rows, bank.n_classes,
                                   _p(slab), nslab, st), "msst_probe_grad")
    _lib.check(lib.msst_probe_update(_p(slab), nslab, rows, DIM, bank.n_classes, None, None, None, None, 0.0, 0.9, 0.999, 1e-8, 0.0,
                                     _p(row), _p(grad), 0, st), "msst_probe_update")
    return grad, row


def fit_linear_probe(bank, steps=500, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, batch=None, class_weights=None,
                     init=None, inplace=None):
    """Train LayerNorm(96) -> Linear(96 -> n_classes) on a bank of cached features (a KnnBank of RAW features, e.g. from probe_bank)
    with the weighted-mean cross entropy (torch's CrossEntropyLoss(weight=class_weights)) and torch.optim.Adam semantics (coupled L2
    weight decay, bias correction, eps outside the square root).  Returns a LinearProbe with history [steps, 4] on the CPU.
      lr            a number, or a sequence of `steps` numbers (a schedule: lr is a launch argument).
      batch         None: every step sees the whole bank.  Otherwise step t takes the next contiguous slice of `batch` rows; the last
                    slice of a pass is the partial remainder and the walk then wraps to row 0 (slice_walk).  Shuffle the bank once
                    beforehand if wanted.  A step whose slice holds only zero-weight classes is skipped whole: parameters, moments and
                    the step count stay, its history row has loss NaN.
      class_weights None or n_classes numbers >= 0, not all 0.
      init          None: gamma 1, beta 0, W 0, b 0.  A LinearProbe: continue from it, moments and step count included (it is
                    copied, not modified).  A model: start from its mlp_head (the patch head with the bank's class count).
      inplace       a model: train the mlp_head segment of its flat parameter buffer where it lies (init, if given, is copied
                    into it first); every other element of the buffer is left untouched.  The returned probe's theta is that view.
    2 * steps launches on the current stream and one synchronisation, the read-back of the history.  ValueError, before any device
    work, for a wrong type, shape, dtype or range; RuntimeError for CPU tensors.  No CPU or eager fallback."""
    _check_bank(bank)
    lrs = _check_hyper(steps, lr, betas, eps, weight_decay, batch)
    nc = bank.n_classes
    cw = _check_class_weights(class_weights, nc)
    if init is not None and not isinstance(init, LinearProbe):
        _patch_head(init, nc, "init")
    if isinstance(init, LinearProbe) and init.n_classes != nc:
        raise ValueError(f"init has {init.n_classes} classes, the bank {nc}")
    if inplace is not None:
        _patch_head(inplace, nc, "inplace")
    _require_cuda(bank.features, "the bank's features")
    _require_cuda(bank.labels, "the bank's labels")
    dev = bank.features.device
    if isinstance(init, LinearProbe):
        _require_cuda(init.theta, "init")
        probe = init.clone()
        probe.history = None
    elif init is not None:
        probe = LinearProbe.from_model(init)
        _require_cuda(probe.theta, "init")
    else:
        theta = torch.zeros(n_params(nc), dtype=torch.float32, device=dev)
        theta[:DIM] = 1.0
        probe = LinearProbe(theta, nc)
    if inplace is not None:
        seg = _head_segment(inplace, nc)
        if init is not None:
            with torch.no_grad():
                seg.copy_(probe.theta)
        probe.theta = seg
    lib = _lib.load()
    M = len(bank)
    walk = slice_walk(M, batch, steps)
    nslab = max(int(lib.msst_probe_scratch_floats(r, nc)) for r in {r for _, r in walk})
    slab = torch.empty(nslab, dtype=torch.float32, device=dev)
    hist = torch.full((steps, 4), float("nan"), dtype=torch.float32, device=dev)
    cw = None if cw is None else cw.to(dev)
    st = _stream()
    x, y, th, m, v, sc = _p(bank.features), _p(bank.labels), _p(probe.theta), _p(probe.m), _p(probe.v), _p(probe.step)
    b1, b2 = float(betas[0]), float(betas[1])
    for t, (row0, rows) in enumerate(walk):
        _lib.check(lib.msst_probe_grad(x, y, _p(cw), th, M, DIM, row0, rows, nc, _p(slab), nslab, st), "msst_probe_grad")
        _lib.check(lib.msst_probe_update(_p(slab), nslab, rows, DIM, nc, th, m, v, sc, lrs[t], b1, b2, float(eps), float(weight_decay),
                                         ctypes.c_void_p(hist.data_ptr() + 16 * t), None, 1, st), "msst_probe_update")
    probe.history = hist.cpu()   # the fit's one synchronisation
    return probe


def probe_bank(model, scenes, labels, stride=None, ignored_label=-1, per_class=None, generator=None):
    """A KnnBank of RAW features from labelled scenes: encode_scene(normalize=False) -- per pixel exactly the vector that mlp_head of
    the patch-head model consumes -- at the pixels that a window covers and whose label is not ignored_label, in scene-major pixel
    order.  Arguments and errors as maskedsst_amd.feature_bank (which keeps unit features, for kNN)."""
    return _bank_from_scenes(model, scenes, labels, stride, ignored_label, per_class, generator, False)


def probe_predict_scene(model, scene, probe, stride=None, max_windows=None):
    """See ViTSpatialSpectral.probe_predict_scene."""
    if not isinstance(probe, LinearProbe):
        raise ValueError(f"probe must be a LinearProbe, got {type(probe).__name__}")

    def launch(emb, Bs, Hs, Ws):
        _require_cuda(probe.theta, "the probe")
        dev = emb.features.device
        logits = torch.empty(Bs, probe.n_classes, Hs, Ws, dtype=torch.float32, device=dev)
        classes = torch.empty(Bs, Hs, Ws, dtype=torch.int64, device=dev)
        probe_forward(probe, emb.features, 1, Bs * Hs * Ws, Hs * Ws, logits, 1, classes)
        return ProbeScene(classes, logits, emb.cover)

    return on_scene_map(model, scene, stride, False, max_windows, launch)
