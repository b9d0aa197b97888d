"""Stand-alone ops of the hot path behind the C-ABI (``include/msst.h``), as autograd functions.

On the pre-training path every one of these runs fused into a larger kernel (``engine.py``); the functions here serve a
caller that needs the op by itself -- the reference's ``nn.LayerNorm`` of ``PreNorm`` / ``BlockwisePatchEmbedding``
(``vit_spatial_spectral.py:25,194-195``) -- and are the unit the fused kernels are checked against.  The finetune loss is an
op of its own on every path: ``cross_entropy_stats`` / ``FusedCrossEntropy`` (``msst_loss.hip``), the reference's
``CrossEntropyLoss(ignore_index)`` with the accuracy counts of its training and validation loops from the same pass; with class
weights, label smoothing and a confusion matrix (``msst_ce_ext_fwd``) it is the loss and the evaluation protocol of DeepHyperX
(``confusion_report``).
HIP only: a CPU tensor raises (no eager fallback).
"""
import ctypes
from collections import namedtuple

import numpy as np
import torch

from . import _lib


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class _LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        lib = _lib.load()
        if not x.is_cuda:
            raise RuntimeError("maskedsst_amd.ops.layer_norm runs on an MI355X only (tensor is on %s); there is no CPU fallback" % x.device)
        D = x.shape[-1]
        if weight.shape != (D,) or bias.shape != (D,):
            raise ValueError("LayerNorm over the last axis: weight / bias must be [%d]" % D)
        xc = x.contiguous().float()
        w, b = weight.contiguous().float(), bias.contiguous().float()
        y = torch.empty_like(xc)
        rows = xc.numel() // D
        _lib.check(lib.msst_layernorm_fwd(_p(xc), _p(w), _p(b), _p(y), _p(None), _p(None), rows, D, float(eps), _stream()),
                   "msst_layernorm_fwd")
        ctx.save_for_backward(xc, w)
        ctx.eps = float(eps)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        xc, w = ctx.saved_tensors
        D = xc.shape[-1]
        rows = xc.numel() // D
        dy = dy.contiguous().float()
        dx = torch.empty_like(xc)
        dg = torch.empty(D, dtype=torch.float32, device=xc.device)
        db = torch.empty(D, dtype=torch.float32, device=xc.device)
        slab = torch.empty(max(1, int(lib.msst_layernorm_bwd_slab(rows, D))), dtype=torch.float32, device=xc.device)
        _lib.check(lib.msst_layernorm_bwd(_p(xc), _p(w), _p(dy), _p(dx), _p(dg), _p(db), _p(slab), rows, D, ctx.eps, _stream()),
                   "msst_layernorm_bwd")
        return dx, dg, db, None


def layer_norm(x, weight, bias, eps=1e-5):
    """``F.layer_norm(x, (D,), weight, bias, eps)`` over the last axis (D <= 128) on the HIP kernels of msst_ln.hip."""
    return _LayerNormFn.apply(x, weight, bias, eps)


CEHost = namedtuple("CEHost", ["loss", "loss_sum", "n_valid", "n_correct", "bad_labels", "nonfinite", "support", "correct",
                               "acc", "macro_acc", "weight_sum", "confusion"], defaults=(None, None))


class CEStats:
    """The statistics record of one ``cross_entropy_stats`` call (``include/msst.h``: ``msst_ce_stats_fwd``), on the device:
    ``record`` int64 [5 + 2 nc] -- the loss sum (a double), ``n_valid``, ``n_correct``, ``bad_labels``, ``nonfinite``, then
    ``support[nc]`` and ``correct[nc]`` by label class.  The properties are device tensors (no synchronisation);
    ``host()`` brings the whole record over in one copy.
    A call with class weights, label smoothing or a confusion matrix (``msst_ce_ext_fwd``) adds ``sums`` (float64 [2]: the loss sum
    again and the weight sum the mean divides by) and ``confusion`` (int64 [nc, nc], row = label, column = argmax; None when it was
    not asked for).  Record and sums lie in one buffer, so ``host()`` still costs one copy, and a second one for a confusion matrix."""

    def __init__(self, record, n_classes, sums=None, confusion=None, buf=None):
        self.record = record
        self.n_classes = n_classes
        self.sums = sums
        self.confusion = confusion
        self._buf = buf   # record | sums as one int64 tensor (the extended call), for host()

    loss_sum = property(lambda self: self.record[_lib.CE_LOSS_SUM:_lib.CE_LOSS_SUM + 1].view(torch.float64)[0])
    n_valid = property(lambda self: self.record[_lib.CE_N_VALID])
    n_correct = property(lambda self: self.record[_lib.CE_N_CORRECT])
    bad_labels = property(lambda self: self.record[_lib.CE_BAD_LABELS])
    nonfinite = property(lambda self: self.record[_lib.CE_NONFINITE])
    support = property(lambda self: self.record[_lib.CE_SUPPORT:_lib.CE_SUPPORT + self.n_classes])
    correct = property(lambda self: self.record[_lib.CE_SUPPORT + self.n_classes:_lib.CE_SUPPORT + 2 * self.n_classes])

    @property
    def weight_sum(self):
        """what the mean loss divides by (float64): the sum of w[label] over the counting rows; n_valid without class weights"""
        return self.sums[_lib.CE_EXT_WEIGHT_SUM] if self.sums is not None else self.n_valid.double()

    @property
    def acc(self):
        """n_correct / n_valid (float64; nan when no row counts)"""
        return self.n_correct.double() / self.n_valid.double()

    @property
    def macro_acc(self):
        """mean of correct[c] / support[c] over the classes with support[c] > 0 (torchmetrics' macro accuracy; nan without any)"""
        sup, cor = self.support.double(), self.correct.double()
        present = sup > 0
        return (cor / sup.clamp_min(1.0)).sum() / present.sum().double()

    def host(self):
        """CEHost of Python numbers (support / correct: lists; confusion: an int64 numpy array or None) from ONE device-to-host copy
        of the record (the sums of an extended call travel in it), and a second one when there is a confusion matrix"""
        nc = self.n_classes
        r = (self._buf if self._buf is not None else self.record).cpu()
        loss_sum = float(r[:1].view(torch.float64)[0])
        v = r.tolist()
        n_valid, n_correct = v[_lib.CE_N_VALID], v[_lib.CE_N_CORRECT]
        support, correct = v[_lib.CE_SUPPORT:_lib.CE_SUPPORT + nc], v[_lib.CE_SUPPORT + nc:_lib.CE_SUPPORT + 2 * nc]
        recall = [c / s for c, s in zip(correct, support) if s > 0]
        nan = float("nan")
        if self._buf is not None:
            weight_sum = float(r[5 + 2 * nc + _lib.CE_EXT_WEIGHT_SUM:][:1].view(torch.float64)[0])
        else:
            weight_sum = float(n_valid)
        confusion = self.confusion.cpu().numpy() if self.confusion is not None else None
        return CEHost(loss=loss_sum / weight_sum if weight_sum > 0 else nan, loss_sum=loss_sum, n_valid=n_valid, n_correct=n_correct,
                      bad_labels=v[_lib.CE_BAD_LABELS], nonfinite=v[_lib.CE_NONFINITE], support=support, correct=correct,
                      acc=n_correct / n_valid if n_valid else nan, macro_acc=sum(recall) / len(recall) if recall else nan,
                      weight_sum=weight_sum, confusion=confusion)


class _CrossEntropyFn(torch.autograd.Function):
    """msst_ce_stats_fwd / msst_ce_bwd; with class weights, label smoothing or a confusion matrix msst_ce_ext_fwd / msst_ce_ext_bwd.
    -> (loss, buf[, confusion]); buf is int64: the record [5 + 2 nc], behind it the two double sums of an extended call"""

    @staticmethod
    def forward(ctx, logits, labels, skip, weight, ignore_index, eps, want_confusion, shape):
        lib = _lib.load()
        R0, nc, M = shape
        dev = logits.device
        ext = weight is not None or eps != 0.0 or want_confusion
        nbytes = int(lib.msst_ce_ext_scratch_bytes(R0, nc, M, int(want_confusion)) if ext else lib.msst_ce_scratch_bytes(R0, nc, M))
        if want_confusion and nc > _lib.CE_CONFUSION_MAX_CLASSES:
            raise _lib.MsstError(f"a confusion matrix needs n_classes <= {_lib.CE_CONFUSION_MAX_CLASSES}, got {nc} "
                                 "(include/msst.h: MSST_CE_CONFUSION_MAX_CLASSES)")
        loss = torch.empty((), dtype=torch.float32, device=dev)
        buf = torch.empty(5 + 2 * nc + (2 if ext else 0), dtype=torch.int64, device=dev)
        confusion = torch.empty((nc, nc), dtype=torch.int64, device=dev) if want_confusion else None
        scratch = torch.empty(max(1, nbytes // 4), dtype=torch.int32, device=dev)
        d = torch.empty_like(logits) if ctx.needs_input_grad[0] else None
        if ext:
            den = buf[5 + 2 * nc:]   # the sums
            _lib.check(lib.msst_ce_ext_fwd(_p(logits), _p(labels), _p(skip), int(ignore_index), _p(weight), float(eps), _p(d), _p(loss),
                                           _p(buf), _p(den), _p(confusion), _p(scratch), R0, nc, M, _stream()), "msst_ce_ext_fwd")
        else:
            den = buf                # the record
            _lib.check(lib.msst_ce_stats_fwd(_p(logits), _p(labels), _p(skip), int(ignore_index), _p(d), _p(loss), _p(buf), _p(scratch),
                                             R0, nc, M, _stream()), "msst_ce_stats_fwd")
        ctx.save_for_backward(d, den)
        ctx.shape, ctx.ext = shape, ext
        ctx.mark_non_differentiable(buf)
        if want_confusion:
            ctx.mark_non_differentiable(confusion)
        ctx.set_materialize_grads(False)   # no zeros_like(buf) launch in the backward
        return (loss, buf, confusion) if want_confusion else (loss, buf)

    @staticmethod
    def backward(ctx, gloss, *_):
        if gloss is None:
            return (None,) * 8
        lib = _lib.load()
        d, den = ctx.saved_tensors
        R0, nc, M = ctx.shape
        gout = gloss.contiguous().float()
        dlogits = torch.empty_like(d)
        name = "msst_ce_ext_bwd" if ctx.ext else "msst_ce_bwd"
        _lib.check(getattr(lib, name)(_p(d), _p(den), _p(gout), _p(dlogits), R0, nc, M, _stream()), name)
        return (dlogits,) + (None,) * 7


def cross_entropy_stats(logits, labels, ignore_index=-1, skip=None, weight=None, label_smoothing=0.0, confusion=False):
    """``F.cross_entropy(logits, labels, ignore_index=ignore_index)`` (mean) on the HIP kernels of msst_loss.hip, with the counts of
    the same pass: -> ``(loss, CEStats)``.  ``loss`` is a 0-d fp32 tensor attached to autograd (its backward is one launch that reads
    the incoming gradient and ``n_valid`` on the device); nothing here synchronises with the host.

    logits [B, nc, H, W], [B, nc] or [nc] (class-major, as the three classifier heads give them); labels int64 [B, H, W], [B] or 0-d.
    skip (optional, shaped like labels): rows with an entry < 0 do not count (``predict_scene``'s class map: -1 = uncovered pixel).
    A label outside [0, nc) that is not ``ignore_index`` does not count and is tallied in ``bad_labels`` (torch asserts on the device).
    No row counts: loss nan, zero gradient, zero counts.

    weight (optional, [nc]), label_smoothing in [0, 1): ``F.cross_entropy(..., weight=weight, label_smoothing=label_smoothing)`` --
    the sum of the rows' weighted losses over ``stats.weight_sum``, the sum of weight[label] over the counting rows (nan loss and
    zero gradient when that is 0).  The counts do not depend on either.  confusion=True: ``stats.confusion`` is the int64 [nc, nc]
    matrix (row = label, column = argmax) of the counting rows, from the same pass (nc <= 128); ``confusion_report`` reads it.
    Without any of the three the call, and its bits, are the ones above."""
    if not torch.is_tensor(logits) or not logits.is_cuda:
        raise RuntimeError("maskedsst_amd.ops.cross_entropy_stats runs on an MI355X only (logits are on %s); there is no CPU fallback"
                           % getattr(logits, "device", type(logits)))
    if logits.dim() == 1:
        shape, lshape = (1, logits.shape[0], 1), ()
    elif logits.dim() == 2:
        shape, lshape = (logits.shape[0], logits.shape[1], 1), (logits.shape[0],)
    elif logits.dim() == 4:
        shape, lshape = (logits.shape[0], logits.shape[1], logits.shape[2] * logits.shape[3]), (logits.shape[0],) + tuple(logits.shape[2:])
    else:
        raise ValueError(f"logits must be [B, nc, H, W], [B, nc] or [nc], got {tuple(logits.shape)}")
    for name, t in (("labels", labels), ("skip", skip)):
        if t is not None and (not torch.is_tensor(t) or tuple(t.shape) != lshape or t.dtype.is_floating_point):
            raise ValueError(f"{name} must be an integer tensor of shape {lshape} for logits {tuple(logits.shape)}, got "
                             f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    dev = logits.device
    labels = labels.to(device=dev, dtype=torch.int64).contiguous()
    skip = skip.to(device=dev, dtype=torch.int64).contiguous() if skip is not None else None
    nc = int(shape[1])
    eps = float(label_smoothing)
    if not 0.0 <= eps < 1.0:
        raise ValueError(f"label_smoothing must lie in [0, 1), got {label_smoothing!r}")
    if weight is not None:
        if not torch.is_tensor(weight) or tuple(weight.shape) != (nc,) or not weight.dtype.is_floating_point:
            raise ValueError(f"weight must be a floating-point tensor of shape ({nc},), got "
                             f"{getattr(weight, 'dtype', type(weight))} {tuple(getattr(weight, 'shape', ()))}")
        weight = weight.detach().to(device=dev, dtype=torch.float32).contiguous()
    shape = tuple(int(v) for v in shape)
    out = _CrossEntropyFn.apply(logits.contiguous().float(), labels, skip, weight, int(ignore_index), eps, bool(confusion), shape)
    loss, buf = out[0], out[1]
    if buf.numel() == 5 + 2 * nc:   # none of weight, smoothing and matrix: the record alone
        return loss, CEStats(buf, nc)
    return loss, CEStats(buf[:5 + 2 * nc], nc, sums=buf[5 + 2 * nc:].view(torch.float64), confusion=out[2] if confusion else None, buf=buf)


ConfusionReport = namedtuple("ConfusionReport", ["oa", "aa", "kappa", "mean_f1", "mean_iou", "precision", "recall", "f1", "iou",
                                                 "support", "total"])


def confusion_report(cm):
    """The evaluation protocol of DeepHyperX (reference DeepHyperX/utils.py:331-385: accuracy, F1 by class, Cohen's kappa) and the
    usual land-cover additions, from a confusion matrix ``cm`` [nc, nc] (row = label, column = prediction; a tensor on any device or
    an array), in float64 on the host.  With n = sum of cm, row_c / col_c its row / column sums and tp_c its diagonal:
      oa         sum_c tp_c / n, as a fraction (nan for an empty matrix)
      recall     tp_c / row_c;  precision  tp_c / col_c;  f1  2 tp_c / (row_c + col_c);  iou  tp_c / (row_c + col_c - tp_c)
                 -- arrays [nc], 0 where the denominator is 0
      aa, mean_f1, mean_iou   the means of recall, f1 and iou over the classes with support (row_c > 0; nan without any)
      kappa      (oa - pe) / (1 - pe), pe = sum_c row_c col_c / n^2; nan when 1 - pe is 0 (or the matrix is empty)
      support    row_c (int64), total n (int)"""
    if torch.is_tensor(cm):
        cm = cm.detach().cpu().numpy()
    cm = np.asarray(cm)
    if cm.ndim != 2 or cm.shape[0] != cm.shape[1]:
        raise ValueError(f"a confusion matrix is square, got shape {cm.shape}")
    support = cm.sum(axis=1).astype(np.int64)
    m = cm.astype(np.float64)
    tp, row, col = np.diag(m), m.sum(axis=1), m.sum(axis=0)
    n = float(m.sum())
    nan = float("nan")

    def ratio(num, den):
        return np.divide(num, den, out=np.zeros_like(num), where=den != 0)

    recall, precision = ratio(tp, row), ratio(tp, col)
    f1, iou = ratio(2.0 * tp, row + col), ratio(tp, row + col - tp)
    present = row > 0
    mean = (lambda v: float(v[present].mean())) if present.any() else (lambda v: nan)
    oa = float(tp.sum() / n) if n > 0 else nan
    pe = float((row * col).sum() / (n * n)) if n > 0 else nan
    kappa = (oa - pe) / (1.0 - pe) if n > 0 and 1.0 - pe != 0.0 else nan
    return ConfusionReport(oa=oa, aa=mean(recall), kappa=kappa, mean_f1=mean(f1), mean_iou=mean(iou), precision=precision,
                           recall=recall, f1=f1, iou=iou, support=support, total=int(cm.sum()))


class FusedCrossEntropy(torch.nn.Module):
    """``torch.nn.CrossEntropyLoss(weight=..., ignore_index=..., label_smoothing=...)`` on ``cross_entropy_stats``:
    ``criterion(logits, labels)`` is the loss; ``criterion(logits, labels, return_stats=True)`` is ``(loss, CEStats)``
    (``confusion=True``: with the confusion matrix).  ``weight`` ([nc], optional) is a buffer: it moves with ``.to()`` and is saved.  ``utils.train_step`` and ``scene.scene_metrics`` take
    their accuracy numbers and the NaN check from the record (one read-back per step) when they are given one."""
    fused_stats = True   # what utils.train_step looks for (it must not import this module for a torch criterion)

    def __init__(self, ignore_index=-1, weight=None, label_smoothing=0.0):
        super().__init__()
        self.ignore_index = int(ignore_index)
        self.label_smoothing = float(label_smoothing)
        if not 0.0 <= self.label_smoothing < 1.0:
            raise ValueError(f"label_smoothing must lie in [0, 1), got {label_smoothing!r}")
        if weight is not None:
            weight = torch.as_tensor(weight, dtype=torch.float32).detach().clone()
            if weight.dim() != 1:
                raise ValueError(f"weight must be [n_classes], got {tuple(weight.shape)}")
        self.register_buffer("weight", weight)
        self._unit = {}

    def unit_gradient(self, device):
        """a cached 0-d one on `device`: ``loss.backward(criterion.unit_gradient(loss.device))`` spares the ones_like(loss) launch
        that a bare ``loss.backward()`` makes every step"""
        if device not in self._unit:
            self._unit[device] = torch.ones((), dtype=torch.float32, device=device)
        return self._unit[device]

    def forward(self, logits, labels, skip=None, return_stats=False, confusion=False):
        loss, stats = cross_entropy_stats(logits, labels, self.ignore_index, skip, weight=self.weight,
                                          label_smoothing=self.label_smoothing, confusion=confusion)
        return (loss, stats) if return_stats else loss

    def extra_repr(self):
        weight = "None" if self.weight is None else "[%s]" % ", ".join("%.4g" % v for v in self.weight.tolist())
        return f"ignore_index={self.ignore_index}, weight={weight}, label_smoothing={self.label_smoothing:g}"
