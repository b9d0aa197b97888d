"""Fused AdamW / grouped Adam + data-parallel gradient reduction for maskedsst_amd models.

``FusedAdamW`` is a ``torch.optim.Optimizer`` (so LR schedulers such as the reference's
``ReduceLROnPlateau``, ``src/utils.py:47-50``, drive it unchanged) whose ``step`` is ONE launch of
``msst_adamw`` over the flat parameter buffer instead of ~350 small tensor updates.  It reproduces
``torch.optim.AdamW`` (reference ``src/utils.py:41-44``) including the "parameters without a
gradient are skipped" rule: ``encoder.mlp_head.*`` receives no gradient in pre-training and lies
outside the updated range.  ``grad_clamp`` applies the reference's per-parameter gradient hook
``clamp(grad, -1, 1)`` (``pretrain.py:71-73``) inside the kernel, after the data-parallel mean.

``FusedAdam`` is the finetune optimizer (reference ``finetune.py:110-136``: ``torch.optim.Adam`` with coupled L2 decay, two
learning rates -- ``lr`` / ``mlp_head_lr`` -- and frozen parameters under ``linear_eval``): its ``step`` turns the parameter groups
into a table of element ranges of the flat buffer (``adam_ranges``) and updates all of them in ONE launch of ``msst_adam_groups``.

``GradAccumulator`` sums the gradients of several micro-batches in a second flat buffer between backwards and leaves their mean,
optionally clipped by its global L2 norm (``clip_grad_norm_``), in the flat gradient buffer: one or two launches
(``msst_grad_accumulate``, ``msst_grad_finalize``) over the range table ``grad_ranges`` builds.

``BucketReducer`` all-reduces slices of the flat gradient buffer as soon as the backward has
completed them (buckets are contiguous because the flat layout follows backward order), on the
process group's own stream (``torch.distributed`` NCCL backend == RCCL on ROCm), overlapping the
remaining backward kernels.  It only needs a flat tensor and a bucket list, so the gloo tests
exercise the same code on CPU tensors.
"""
import ctypes
import os
from collections import namedtuple

import torch
import torch.distributed as dist


def dp_mean(value, group=None):
    """Mean of a scalar tensor over the data-parallel ranks (identity in a single process).  Used for every number
    that steers replicated state -- e.g. the validation loss fed to ReduceLROnPlateau (reference pretrain.py:194-197):
    the all-reduce of the gradients keeps the WEIGHTS equal only while every rank applies the same learning rate."""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return value
    v = value.detach().clone().float().reshape(1)
    dist.all_reduce(v, op=dist.ReduceOp.SUM, group=group)
    return (v / dist.get_world_size(group)).reshape(())


class BucketReducer:
    def __init__(self, flat_grad, buckets, group=None, bucket_bytes=4 << 20, average_in_optimizer=True):
        """buckets: [(name, start, end)] in the order the backward completes them."""
        self.flat = flat_grad
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        # MSST_FORCE_DP=1: issue the collectives even with a single rank (exercises the RCCL path on a 1-GPU box)
        self.force = dist.is_initialized() and os.environ.get("MSST_FORCE_DP", "0") == "1"
        self.bucket_bytes = bucket_bytes
        self.average_in_optimizer = average_in_optimizer
        self.order = [b[0] for b in buckets]
        self.range = {b[0]: (b[1], b[2]) for b in buckets}
        self.reset()

    def reset(self):
        self.handles = []
        self.pending = None  # (start, end) of completed-but-unsent contiguous range
        self.done = set()

    def bucket_ready(self, name, start=None, end=None):
        """called (in backward order) when a bucket's gradients are final"""
        if self.world == 1 and not self.force:
            return
        s, e = self.range[name]
        self.done.add(name)
        if self.pending is None:
            self.pending = (s, e)
        elif self.pending[1] == s:
            self.pending = (self.pending[0], e)
        else:  # non-contiguous: flush what we have, start a new run
            self._flush()
            self.pending = (s, e)
        # the LAST bucket of the backward (the tokenizer's) goes out from its own hook: left to finish(), its all-reduce would
        # start only when the host gets there and sit fully exposed in front of the optimizer step
        if (self.pending[1] - self.pending[0]) * self.flat.element_size() >= self.bucket_bytes or name == self.order[-1]:
            self._flush()

    def _flush(self):
        if self.pending is None:
            return
        s, e = self.pending
        self.pending = None
        if e > s:
            h = dist.all_reduce(self.flat[s:e], op=dist.ReduceOp.SUM, group=self.group, async_op=True)
            self.handles.append(h)

    def finish(self):
        """flush the tail and wait for every outstanding all-reduce; returns the scale still to be
        applied to the gradients (1/world when the optimizer does the averaging)."""
        if self.world > 1 or self.force:
            self._flush()
            for h in self.handles:
                h.wait()
            if not self.average_in_optimizer:
                lo = min(self.range[n][0] for n in self.order)
                hi = max(self.range[n][1] for n in self.order)
                self.flat[lo:hi].mul_(1.0 / self.world)
        self.handles = []
        self.done = set()
        return (1.0 / self.world) if self.average_in_optimizer else 1.0


class FusedAdamW(torch.optim.Optimizer):
    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, grad_clamp=0.0):
        params = [p for p in model.parameters()]
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.model = model
        self.grad_clamp = float(grad_clamp)
        self.grad_scale = 1.0
        self._m = None
        self._v = None
        self._step = 0
        self._flat_id = None
        self._checked_flat = None

    def _state(self, eng):
        eng.ensure()
        flat = eng.fp.flat
        if self._m is None or self._flat_id != flat.data_ptr():
            # (re)allocate moments; a re-flatten (e.g. after .to()) carries the old moments over
            m = torch.zeros_like(flat)
            v = torch.zeros_like(flat)
            if self._m is not None and self._m.numel() == m.numel():
                m.copy_(self._m)
                v.copy_(self._v)
            self._m, self._v = m, v
            self._flat_id = flat.data_ptr()
        return flat, eng.fp.grad, self._m, self._v

    def zero_grad(self, set_to_none=True):
        # The backward overwrites the flat gradient buffer and hands autograd VIEWS of it, so the
        # .grad attributes must be dropped (not zeroed, not kept): a surviving .grad would make
        # autograd accumulate a view onto itself.
        return super().zero_grad(set_to_none=True)

    @torch.no_grad()
    def step(self, closure=None):
        from . import _lib
        eng = self.model.engine()
        flat, grad, m, v = self._state(eng)
        # The launch updates the whole trainable prefix of the flat buffer.  torch.optim.AdamW skips parameters
        # without a gradient; a frozen (requires_grad=False) or unused parameter inside the prefix would instead
        # receive weight decay plus whatever the gradient buffer last held -- refuse rather than diverge silently.
        # (attribute reads only on the per-step path; the pointer-range check runs on the first step and after a re-flatten)
        named = eng.trainable()
        full = self._checked_flat != grad.data_ptr()
        lo, hi = grad.data_ptr(), grad.data_ptr() + 4 * grad.numel()
        for name, p in named:
            if not p.requires_grad:
                raise RuntimeError(f"FusedAdamW updates every trainable parameter in one launch; {name!r} has "
                                   "requires_grad=False -- use torch.optim.AdamW for partially frozen models")
            if p.grad is None or (full and not (lo <= p.grad.data_ptr() < hi)):
                raise RuntimeError(f"FusedAdamW.step(): parameter {name!r} has no gradient from the HIP backward of "
                                   "this step (call loss.backward() first; gradients must be the flat-buffer views)")
        self._checked_flat = grad.data_ptr()
        # cheap per-step guard on one sentinel per end of the buffer: a later step whose .grad is not a flat-buffer view any
        # more (e.g. hooks that replace gradients) must not be applied from stale buffer contents
        for name, p in (named[0], named[-1]):
            if not (lo <= p.grad.data_ptr() < hi):
                raise RuntimeError(f"FusedAdamW.step(): the gradient of {name!r} is no view of the flat gradient buffer")
        g = self.param_groups[0]
        self._step += 1
        n = eng.fp.n_trainable
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        _lib.check(eng.lib.msst_adamw(P(flat), P(grad), P(m), P(v), n, float(g["lr"]), float(g["betas"][0]),
                                      float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]), self._step,
                                      self.grad_clamp, float(self.grad_scale), stream), "msst_adamw")
        return None

    def state_dict(self):
        d = super().state_dict()
        # clones: an in-memory snapshot must not keep changing as training continues
        d["fused"] = dict(step=self._step, m=None if self._m is None else self._m.clone(),
                          v=None if self._v is None else self._v.clone())
        return d

    def load_state_dict(self, state_dict):
        """Restores lr / betas / ... through torch and the fused moments + step count saved by ``state_dict``
        (a resumed run continues the bias correction where it stopped instead of restarting at step 0)."""
        state_dict = dict(state_dict)
        fused = state_dict.pop("fused", None)
        # validate everything BEFORE touching any state: a failed load must leave the optimizer as it was
        if fused is None:
            raise KeyError("state dict has no 'fused' entry: it was not produced by FusedAdamW.state_dict()")
        eng = self.model.engine()
        flat, _, m, v = self._state(eng)
        if fused["m"] is not None and (fused["m"].numel() != m.numel() or fused["v"] is None or fused["v"].numel() != v.numel()):
            raise ValueError(f"fused moments have {fused['m'].numel()} elements, the model needs {m.numel()}")
        super().load_state_dict(state_dict)
        self._step = int(fused["step"])
        if fused["m"] is not None:
            m.copy_(fused["m"].to(m.device))
            v.copy_(fused["v"].to(v.device))
        else:
            m.zero_()
            v.zero_()


class AdamRange(namedtuple("AdamRange", "start end group step params")):
    """one entry of the grouped-Adam table: elements [start, end) of the flat buffers, updated with the hyper-parameters of
    param_groups[group] at bias-correction step `step`; params: the tensors it covers, in flat order"""
    __slots__ = ()

    @property
    def aligned(self):
        """both ends on a 16-byte boundary (otherwise the kernel moves up to 3 + 3 single floats at the ragged ends)"""
        return self.start % 4 == 0 and self.end % 4 == 0


def _locator(fp, who, where):
    """locate(p) -> the offset of parameter p in the flat buffers of ``fp``, or None when p is skipped (``requires_grad=False`` or
    ``grad is None``: torch's rule); raises when p is no view of ``fp.flat`` or its ``.grad`` is not p's own view of ``fp.grad``.
    who / where: how the two messages name the caller."""
    base, gbase = fp.flat.data_ptr(), fp.grad.data_ptr()
    known = {off: n for off, n, _ in fp.segments.values()}

    def locate(p):
        if not p.requires_grad or p.grad is None:
            return None
        off, rem = divmod(p.data_ptr() - base, 4)
        if rem or known.get(off) != p.numel():
            raise RuntimeError(f"{who}: a parameter of the optimizer is no view of the model's flat parameter buffer "
                               "(was the model rebuilt or moved without a forward since?)")
        if p.grad.data_ptr() != gbase + 4 * off or p.grad.numel() != p.numel() or p.grad.dtype != torch.float32:
            raise RuntimeError(f"{where}: a gradient is no view of the flat gradient buffer (gradients must be "
                               "the ones the HIP backward hands to autograd)")
        return off
    return locate


def adam_ranges(fp, param_groups, step_of=None, max_ranges=64):
    """The range table of one grouped-Adam step over the flat buffers of ``fp`` (a ``FlatParams``; CPU or GPU).

    Every parameter of ``param_groups`` is located in ``fp.flat`` by its ``data_ptr``; parameters with
    ``requires_grad=False`` or ``grad is None`` are skipped (torch's rule) and leave a hole; a ``.grad`` that is not the
    parameter's view of ``fp.grad`` raises.  ``step_of(p)``: updates this tensor has received so far (default: none), its range runs
    at that plus one.  Neighbouring segments of one group whose step counters are equal merge into one range.  Returns the
    ``AdamRange`` list sorted by start; more than ``max_ranges`` (the kernel's table size, MSST_ADAM_MAX_GROUPS) raises."""
    locate = _locator(fp, "FusedAdam", "FusedAdam.step()")
    segs = []
    for gi, group in enumerate(param_groups):
        for p in group["params"]:
            off = locate(p)
            if off is not None:
                segs.append((off, off + p.numel(), gi, (step_of(p) if step_of is not None else 0) + 1, p))
    segs.sort(key=lambda t: t[0])
    out = []
    for start, end, gi, step, p in segs:
        if out and out[-1].end == start and out[-1].group == gi and out[-1].step == step:
            last = out[-1]
            out[-1] = last._replace(end=end, params=last.params + [p])
        else:
            out.append(AdamRange(start, end, gi, step, [p]))
    if len(out) > max_ranges:
        raise ValueError(f"FusedAdam: the frozen / unfrozen pattern of the parameters splits the flat buffer into {len(out)} "
                         f"ranges, the kernel's table holds {max_ranges}; use torch.optim.Adam for this pattern")
    return out


class FusedAdam(torch.optim.Optimizer):
    """``torch.optim.Adam`` (``decoupled=True``: ``AdamW``) over a maskedsst_amd model as ONE launch per step.

    ``params``: ``None`` (every parameter of ``model``), a parameter list, or a list of group dicts with their own ``lr`` /
    ``weight_decay`` -- what ``torch.optim.Adam`` takes; ``param_groups`` look like torch's, so LR schedulers and a manual
    ``group["lr"] = ...`` drive it.  Parameters that are frozen or received no gradient are skipped, as torch skips them; each tensor
    counts its own updates for the bias correction (a host integer in ``state[p]["step"]``), so a body unfrozen after some linear-eval
    steps starts at step 1 with zero moments.  betas and eps are those of the first group (one pair per launch)."""

    def __init__(self, model, params=None, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False):
        params = list(model.parameters()) if params is None else list(params)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.model = model
        self.decoupled = bool(decoupled)
        self.grad_scale = 1.0
        self._m = None
        self._v = None
        self._flat_id = None
        self._key = None      # (flat layout version, skip pattern) the cached table was built for
        self._ranges = None
        self._table = None

    _state = FusedAdamW._state   # the flat moment buffers (carried over a re-flatten)

    def zero_grad(self, set_to_none=True):
        # as FusedAdamW: the backward hands autograd views of the flat gradient buffer, a surviving .grad would accumulate onto itself
        return super().zero_grad(set_to_none=True)

    def _steps_taken(self, p):
        return int(self.state[p].get("step", 0)) if p in self.state else 0

    def ranges(self, fp):
        """this step's range table (cached on the flat layout and on which parameters are skipped: between most steps only lr changes)"""
        from . import _lib
        pattern = tuple(p.requires_grad and p.grad is not None for g in self.param_groups for p in g["params"])
        key = (fp.version, pattern)
        if key != self._key:
            self._ranges = adam_ranges(fp, self.param_groups, self._steps_taken, _lib.ADAM_MAX_GROUPS)
            self._table = (_lib.MsstAdamGroup * max(1, len(self._ranges)))()
            self._key = key
        else:
            gbase, base = fp.grad.data_ptr(), fp.flat.data_ptr()
            for r in self._ranges:
                for p in r.params:
                    if p.grad.data_ptr() - gbase != p.data_ptr() - base:
                        raise RuntimeError("FusedAdam.step(): a gradient is no view of the flat gradient buffer (gradients must "
                                           "be the ones the HIP backward hands to autograd)")
        return self._ranges

    @torch.no_grad()
    def step(self, closure=None):
        from . import _lib
        eng = self.model.engine()
        flat, grad, m, v = self._state(eng)
        ranges = self.ranges(eng.fp)
        if not ranges:
            return None
        g0 = self.param_groups[0]
        if any(tuple(g["betas"]) != tuple(g0["betas"]) or g["eps"] != g0["eps"] for g in self.param_groups):
            raise ValueError("FusedAdam: betas and eps must be the same in every parameter group (one launch, one pair)")
        flags = _lib.ADAM_DECOUPLED if self.decoupled else 0
        for t, r in zip(self._table, ranges):
            g = self.param_groups[r.group]
            t.start, t.end, t.lr, t.weight_decay, t.step, t.flags = r.start, r.end, float(g["lr"]), float(g["weight_decay"]), r.step, flags
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        _lib.check(eng.lib.msst_adam_groups(P(flat), P(grad), P(m), P(v), self._table, len(ranges), ctypes.sizeof(_lib.MsstAdamGroup),
                                            float(g0["betas"][0]), float(g0["betas"][1]), float(g0["eps"]), float(self.grad_scale),
                                            stream), "msst_adam_groups")
        for i, r in enumerate(ranges):
            for p in r.params:
                self.state[p]["step"] = r.step
            ranges[i] = r._replace(step=r.step + 1)
        return None

    def state_dict(self):
        d = super().state_dict()   # param_groups and the per-tensor step counters
        # copies and clones: an in-memory snapshot must not keep changing as training continues (torch hands out its live state)
        d["state"] = {k: dict(v) for k, v in d["state"].items()}
        d["fused"] = dict(m=None if self._m is None else self._m.clone(), v=None if self._v is None else self._v.clone())
        return d

    def load_state_dict(self, state_dict):
        """Restores lr / betas / ... and the per-tensor step counters through torch, and the flat moments saved by ``state_dict``."""
        state_dict = dict(state_dict)
        fused = state_dict.pop("fused", None)
        # validate everything BEFORE touching any state: a failed load must leave the optimizer as it was
        if fused is None:
            raise KeyError("state dict has no 'fused' entry: it was not produced by FusedAdam.state_dict()")
        eng = self.model.engine()
        _, _, m, v = self._state(eng)
        if fused["m"] is not None and (fused["m"].numel() != m.numel() or fused["v"] is None or fused["v"].numel() != v.numel()):
            raise ValueError(f"fused moments have {fused['m'].numel()} elements, the model needs {m.numel()}")
        super().load_state_dict(state_dict)
        self._key = None
        if fused["m"] is not None:
            m.copy_(fused["m"].to(m.device))
            v.copy_(fused["v"].to(v.device))
        else:
            m.zero_()
            v.zero_()


GradRange = namedtuple("GradRange", "start end params")   # elements [start, end) of the flat buffers; params: the tensors covered, in flat order


def grad_ranges(fp, params, max_ranges=64):
    """The range table of one ``GradAccumulator.add()`` over the flat buffers of ``fp`` (a ``FlatParams``; CPU or GPU): every
    parameter of ``params`` that holds its view of ``fp.grad``, located as ``adam_ranges`` locates them; frozen parameters and
    parameters without a gradient leave a hole, neighbouring segments merge.  Returns the ``GradRange`` list sorted by start; more
    than ``max_ranges`` (the kernels' table size, MSST_GRAD_MAX_RANGES) raises."""
    locate = _locator(fp, "GradAccumulator", "GradAccumulator.add()")
    segs = sorted(((off, p) for off, p in ((locate(p), p) for p in params) if off is not None), key=lambda t: t[0])
    out = []
    for off, p in segs:
        if out and out[-1].end == off:
            out[-1] = out[-1]._replace(end=off + p.numel(), params=out[-1].params + [p])
        else:
            out.append(GradRange(off, off + p.numel(), [p]))
    if len(out) > max_ranges:
        raise ValueError(f"GradAccumulator: the frozen / unfrozen pattern of the parameters splits the flat buffer into {len(out)} "
                         f"ranges, the kernels' table holds {max_ranges}")
    return out


class GradAccumulator:
    """Sums the gradients of ``steps`` micro-batches in a second flat buffer and leaves their mean in the flat gradient buffer, clipped
    by its global L2 norm when ``max_norm`` is set (``torch.nn.utils.clip_grad_norm_``): one or two launches per call instead of one
    kernel per parameter tensor.

        acc = GradAccumulator(model, steps=K, max_norm=1.0)
        for k, img in enumerate(micro_batches):
            model(img, masks=micro_masks(masks, k, K)).backward()
            ready = acc.add()            # True after the K-th call
        optimizer.step(); optimizer.zero_grad()

    Calls 1 .. K-1 add the gradients the backward has just written to ``fp.accum`` and drop the parameters' ``.grad`` so that the next
    backward is accepted.  Call K leaves ``dp_scale / K`` times the sum in ``fp.grad``, where the parameters' ``.grad`` views still
    point: ``FusedAdamW``, ``FusedAdam`` (``grad_scale`` left at 1) and any ``torch.optim`` optimizer step on it unchanged.  The
    parameters that take part are those that hold a flat-buffer gradient at the first call of a cycle (frozen ones and ones without a
    gradient leave holes nobody touches); another pattern later in the cycle raises.  ``steps=1`` is a fused ``clip_grad_norm_``.
    ``track_norm``: measure the norm without clipping.  ``error_if_nonfinite``: read the record back on the final call and raise when a
    summed gradient is NaN or infinite, as torch does."""

    def __init__(self, model, steps=1, max_norm=None, track_norm=False, error_if_nonfinite=False):
        if int(steps) < 1:
            raise ValueError(f"steps must be >= 1, got {steps}")
        if max_norm is not None and not float(max_norm) > 0.0:
            raise ValueError(f"max_norm must be > 0 (None: no clip), got {max_norm}")
        self.model = model
        self.steps = int(steps)
        self.max_norm = None if max_norm is None else float(max_norm)
        self.track_norm = bool(track_norm)
        self.error_if_nonfinite = bool(error_if_nonfinite)
        self.count = 0            # calls of add() in the running cycle
        self._key = None          # (flat layout version, which parameters hold a gradient) of the running cycle
        self._table_key = None    # ... the cached range table was built for
        self._ranges = None
        self._table = None
        self._scratch = None
        self._record = None
        self._has_record = False

    @property
    def wants_norm(self):
        return self.max_norm is not None or self.track_norm or self.error_if_nonfinite

    def reset(self):
        """abandon the running cycle (the next ``add()`` starts a new sum)"""
        self.count = 0
        self._key = None

    @torch.no_grad()
    def add(self, dp_scale=1.0):
        """Take in the gradients of the backward that has just run.  dp_scale: what ``BucketReducer.finish()`` returned (1 / world
        when the all-reduce summed), applied with the 1 / steps of the mean on the final call.  Returns True when that was the final
        call of the cycle and ``fp.grad`` holds the finished gradient."""
        from . import _lib
        eng = self.model.engine()
        fp = eng.fp
        if fp.flat is None:
            raise RuntimeError("GradAccumulator.add(): no backward has run yet (the model has no flat gradient buffer)")
        # the table is cached on the flat layout and on which parameters hold a gradient (as FusedAdam.ranges: attribute reads only
        # on the per-call path); a hit re-checks the gradients at both ends of every range against the flat buffer
        named = eng.trainable()
        key = (fp.version, tuple(p.requires_grad and p.grad is not None for _, p in named))
        if key != self._table_key:
            ranges = grad_ranges(fp, [p for _, p in named], _lib.GRAD_MAX_RANGES)
            self._ranges = ranges
            self._table = (_lib.MsstGradRange * max(1, len(ranges)))(*[_lib.MsstGradRange(r.start, r.end) for r in ranges])
            self._table_key = key
        else:
            ranges = self._ranges
            gbase, base = fp.grad.data_ptr(), fp.flat.data_ptr()
            for r in ranges:
                for p in (r.params[0], r.params[-1]):
                    if p.grad.data_ptr() - gbase != p.data_ptr() - base:
                        raise RuntimeError("GradAccumulator.add(): a gradient is no view of the flat gradient buffer (gradients must "
                                           "be the ones the HIP backward hands to autograd)")
        if not ranges:
            raise RuntimeError("GradAccumulator.add(): no parameter holds a gradient of the HIP backward (call loss.backward() first)")
        if self.count == 0:
            self._key = key
        elif key != self._key:
            raise RuntimeError("GradAccumulator.add(): the parameters that hold a gradient changed inside an accumulation cycle "
                               f"(call {self.count + 1} of {self.steps}): freeze / unfreeze or rebuild between cycles, or reset()")
        first = self.count == 0
        final = self.count + 1 == self.steps
        grad, accum = fp.grad, fp.accum_buffer()
        n, nbytes = len(ranges), ctypes.sizeof(_lib.MsstGradRange)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        if not final:
            _lib.check(eng.lib.msst_grad_accumulate(P(accum), P(grad), self._table, n, nbytes, int(first), None, 1.0, None, stream),
                       "msst_grad_accumulate")
            for r in ranges:
                for p in r.params:
                    p.grad = None
            self.count += 1
            return False
        scale = float(dp_scale) / self.steps
        if not self.wants_norm:
            _lib.check(eng.lib.msst_grad_accumulate(P(accum), P(grad), self._table, n, nbytes, int(first), P(grad), scale, None, stream),
                       "msst_grad_accumulate")
        else:
            if self._scratch is None or self._scratch.device != grad.device:
                self._scratch = torch.empty(int(eng.lib.msst_grad_accum_scratch_bytes(_lib.GRAD_MAX_RANGES)) // 8, dtype=torch.float64,
                                            device=grad.device)
                self._record = torch.zeros(4, dtype=torch.float32, device=grad.device)
            _lib.check(eng.lib.msst_grad_accumulate(P(accum), P(grad), self._table, n, nbytes, int(first), None, 1.0, P(self._scratch),
                                                    stream), "msst_grad_accumulate")
            _lib.check(eng.lib.msst_grad_finalize(P(accum), P(grad), self._table, n, nbytes, scale,
                                                  0.0 if self.max_norm is None else self.max_norm, P(self._scratch), P(self._record),
                                                  stream), "msst_grad_finalize")
            self._has_record = True
        self.count = 0
        self._key = None
        if self.error_if_nonfinite:
            norm, _, bad = self.record()
            if bad or norm != norm or norm in (float("inf"), float("-inf")):
                raise RuntimeError(f"GradAccumulator: the accumulated gradient holds {bad} non-finite values (total norm {norm}); "
                                   "the flat gradient buffer has been written all the same")
        return True

    def record(self):
        """(norm, coef, nonfinite) of the last finished cycle: the L2 norm of the mean gradient before clipping, the factor it was
        multiplied with (1.0 without ``max_norm`` or below it) and how many summed gradients were NaN or infinite.  One read-back."""
        if not self._has_record:
            raise RuntimeError("GradAccumulator.record(): no cycle with max_norm, track_norm or error_if_nonfinite has finished yet")
        norm, coef, bad, _ = self._record.tolist()
        return norm, coef, int(bad)


def attach_data_parallel(model, group=None, bucket_bytes=4 << 20):
    """Make ``model`` (a SimMIMSpatialSpectral) data parallel over ``group``: masks are drawn for
    the global batch, gradient buckets are all-reduced as the backward completes them.  Returns the
    reducer; call ``reducer.finish()`` after ``loss.backward()`` and hand its return value to
    ``optimizer.grad_scale``."""
    eng = model.engine()
    eng.ensure()
    model.dp_rank = dist.get_rank(group) if dist.is_initialized() else 0
    model.dp_world = dist.get_world_size(group) if dist.is_initialized() else 1
    red = BucketReducer(eng.fp.grad, eng.fp.buckets, group=group, bucket_bytes=bucket_bytes)
    eng.bucket_hook = red.bucket_ready
    # RCCL's channel workgroups need CUs of their own while the backward runs.  The backward's persistent grids fill every CU
    # with ONE workgroup each and are statically partitioned: a workgroup that finds no CU runs BEHIND the others and doubles
    # that launch.  Measured with bench.py --cu-thief (N probe workgroups, each holding a whole CU under the backward;
    # profiles/r03_dp_cu_contention.jsonl, two-head attention backward): step 26.46 ms undisturbed; 33.6-33.7 ms (+27 %) with
    # 8, 16 or 32 probes on the full grids; with 16 CUs left free 28.1 ms (+6 %) for 8 / 16 probes but 34.7 ms (+31 %) for 32;
    # with 32 CUs left free 27.6-27.7 ms (+4.5 %) for all three.  Hence 32 (RCCL's default channel count on this node is below
    # that); the r04 sweep (profiles/r04_dp_cu_contention.jsonl) adds the no-probe run on the reserved grids.
    # Round 4: under data parallel the attention backward and the fused LN1 + MLP launch no longer partition their tiles
    # statically but DRAW them (engine.tile_queue -> msst_block_bwd_chain's tile_queue): a workgroup whose CU is held by a
    # channel workgroup simply draws fewer tiles, so nothing has to be reserved (MSST_DP_RESERVE_CUS, default 0 now; the static
    # partition with 32 reserved CUs is MSST_DP_TILE_QUEUE=0 MSST_DP_RESERVE_CUS=32).  Cost: the gradients are no longer
    # bit-reproducible from run to run (fp32 summation order follows the draw order).
    # The queue only exists on the chained bf16 path (Engine.queue_capable): an fp32 run, an odd head count, MSST_DBG kernel
    # selections or MSST_BWD_CHAIN=0 fall back to msst_block_bwd with full static grids -- those keep round 3's reservation.
    if model.dp_world > 1 or os.environ.get("MSST_FORCE_DP", "0") == "1":
        eng.tile_queue = os.environ.get("MSST_DP_TILE_QUEUE", "1") != "0" and eng.queue_capable()
        reserve = int(os.environ.get("MSST_DP_RESERVE_CUS", "0" if eng.tile_queue else "32"))
        if reserve > 0:
            eng.reserve_cus(reserve)
    return red
