"""Stand-alone ops of the hot path behind the C-ABI (``include/msst.h``), as autograd functions.

On the pre-training path every one of these runs fused into a larger kernel (``engine.py``); the functions here serve a
caller that needs the op by itself -- the reference's ``nn.LayerNorm`` of ``PreNorm`` / ``BlockwisePatchEmbedding``
(``vit_spatial_spectral.py:25,194-195``) -- and are the unit the fused kernels are checked against.  The finetune loss is an
op of its own on every path: ``cross_entropy_stats`` / ``FusedCrossEntropy`` (``msst_loss.hip``), the reference's
``CrossEntropyLoss(ignore_index)`` with the accuracy counts of its training and validation loops from the same pass.
HIP only: a CPU tensor raises (no eager fallback).
"""
import ctypes
from collections import namedtuple

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
                               "acc", "macro_acc"])


class CEStats:
    """The statistics record of one ``cross_entropy_stats`` call (``include/msst.h``: ``msst_ce_stats_fwd``), on the device:
    ``record`` int64 [5 + 2 nc] -- the loss sum (a double), ``n_valid``, ``n_correct``, ``bad_labels``, ``nonfinite``, then
    ``support[nc]`` and ``correct[nc]`` by label class.  The properties are device tensors (no synchronisation);
    ``host()`` brings the whole record over in one copy."""

    def __init__(self, record, n_classes):
        self.record = record
        self.n_classes = n_classes

    loss_sum = property(lambda self: self.record[_lib.CE_LOSS_SUM:_lib.CE_LOSS_SUM + 1].view(torch.float64)[0])
    n_valid = property(lambda self: self.record[_lib.CE_N_VALID])
    n_correct = property(lambda self: self.record[_lib.CE_N_CORRECT])
    bad_labels = property(lambda self: self.record[_lib.CE_BAD_LABELS])
    nonfinite = property(lambda self: self.record[_lib.CE_NONFINITE])
    support = property(lambda self: self.record[_lib.CE_SUPPORT:_lib.CE_SUPPORT + self.n_classes])
    correct = property(lambda self: self.record[_lib.CE_SUPPORT + self.n_classes:_lib.CE_SUPPORT + 2 * self.n_classes])

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
        """CEHost of Python numbers (support / correct: lists) from ONE device-to-host copy of the record"""
        r = self.record.cpu()
        nc = self.n_classes
        loss_sum = float(r[:1].view(torch.float64)[0])
        v = r.tolist()
        n_valid, n_correct = v[_lib.CE_N_VALID], v[_lib.CE_N_CORRECT]
        support, correct = v[_lib.CE_SUPPORT:_lib.CE_SUPPORT + nc], v[_lib.CE_SUPPORT + nc:_lib.CE_SUPPORT + 2 * nc]
        recall = [c / s for c, s in zip(correct, support) if s > 0]
        nan = float("nan")
        return CEHost(loss=loss_sum / n_valid if n_valid else nan, loss_sum=loss_sum, n_valid=n_valid, n_correct=n_correct,
                      bad_labels=v[_lib.CE_BAD_LABELS], nonfinite=v[_lib.CE_NONFINITE], support=support, correct=correct,
                      acc=n_correct / n_valid if n_valid else nan, macro_acc=sum(recall) / len(recall) if recall else nan)


class _CrossEntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, skip, ignore_index, shape):
        lib = _lib.load()
        R0, nc, M = shape
        dev = logits.device
        loss = torch.empty((), dtype=torch.float32, device=dev)
        record = torch.empty(5 + 2 * nc, dtype=torch.int64, device=dev)
        scratch = torch.empty(max(1, int(lib.msst_ce_scratch_bytes(R0, nc, M)) // 4), dtype=torch.int32, device=dev)
        d = torch.empty_like(logits) if ctx.needs_input_grad[0] else None
        _lib.check(lib.msst_ce_stats_fwd(_p(logits), _p(labels), _p(skip), int(ignore_index), _p(d), _p(loss), _p(record), _p(scratch),
                                         R0, nc, M, _stream()), "msst_ce_stats_fwd")
        ctx.save_for_backward(d, record)
        ctx.shape = shape
        ctx.mark_non_differentiable(record)
        ctx.set_materialize_grads(False)   # no zeros_like(record) launch in the backward
        return loss, record

    @staticmethod
    def backward(ctx, gloss, _grecord):
        if gloss is None:
            return None, None, None, None, None
        lib = _lib.load()
        d, record = ctx.saved_tensors
        R0, nc, M = ctx.shape
        gout = gloss.contiguous().float()
        dlogits = torch.empty_like(d)
        _lib.check(lib.msst_ce_bwd(_p(d), _p(record), _p(gout), _p(dlogits), R0, nc, M, _stream()), "msst_ce_bwd")
        return dlogits, None, None, None, None


def cross_entropy_stats(logits, labels, ignore_index=-1, skip=None):
    """``F.cross_entropy(logits, labels, ignore_index=ignore_index)`` (mean) on the HIP kernels of msst_loss.hip, with the counts of
    the same pass: -> ``(loss, CEStats)``.  ``loss`` is a 0-d fp32 tensor attached to autograd (its backward is one launch that reads
    the incoming gradient and ``n_valid`` on the device); nothing here synchronises with the host.

    logits [B, nc, H, W], [B, nc] or [nc] (class-major, as the three classifier heads give them); labels int64 [B, H, W], [B] or 0-d.
    skip (optional, shaped like labels): rows with an entry < 0 do not count (``predict_scene``'s class map: -1 = uncovered pixel).
    A label outside [0, nc) that is not ``ignore_index`` does not count and is tallied in ``bad_labels`` (torch asserts on the device).
    No row counts: loss nan, zero gradient, zero counts."""
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
    loss, record = _CrossEntropyFn.apply(logits.contiguous().float(), labels, skip, int(ignore_index), tuple(int(v) for v in shape))
    return loss, CEStats(record, int(shape[1]))


class FusedCrossEntropy(torch.nn.Module):
    """``torch.nn.CrossEntropyLoss(ignore_index=...)`` on ``cross_entropy_stats``: ``criterion(logits, labels)`` is the loss;
    ``criterion(logits, labels, return_stats=True)`` is ``(loss, CEStats)``.  ``utils.train_step`` and ``scene.scene_metrics`` take
    their accuracy numbers and the NaN check from the record (one read-back per step) when they are given one."""
    fused_stats = True   # what utils.train_step looks for (it must not import this module for a torch criterion)

    def __init__(self, ignore_index=-1):
        super().__init__()
        self.ignore_index = int(ignore_index)
        self._unit = {}

    def unit_gradient(self, device):
        """a cached 0-d one on `device`: ``loss.backward(criterion.unit_gradient(loss.device))`` spares the ones_like(loss) launch
        that a bare ``loss.backward()`` makes every step"""
        if device not in self._unit:
            self._unit[device] = torch.ones((), dtype=torch.float32, device=device)
        return self._unit[device]

    def forward(self, logits, labels, skip=None, return_stats=False):
        loss, stats = cross_entropy_stats(logits, labels, self.ignore_index, skip)
        return (loss, stats) if return_stats else loss

    def extra_repr(self):
        return f"ignore_index={self.ignore_index}"
