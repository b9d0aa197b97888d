#!/usr/bin/env python3
"""What gradient accumulation and the global-norm clip cost at the bench shape (200 bands, 8 x 8, depth 12: 5.19 M gradients), one run
on one box.  Three operations on the flat buffers -- a non-final micro-step (acc += g), the final one without a clip (g = mean) and
the final one with a clip (g = clipped mean) -- each four ways:

  hip_kernel_*   the msst_grad_accumulate / msst_grad_finalize launches alone, back to back (device time per call);
  hip_add_*      ``GradAccumulator.add()`` as a training loop calls it: table from the ~350 parameters, launch(es), dropping ``.grad``;
  eager_*        the eager restatement on the same flat buffers: ``accum.add_(grad)``, ``torch.linalg.vector_norm``, ``mul``;
  foreach_*      ``torch._foreach_add_`` / ``_foreach_mul_`` / ``clip_grad_norm_`` over the per-parameter views.

The variants run alternated, round after round; a figure is the median over the rounds of (time of `inner` calls) / inner.  host_us: the
host clock around the calls and a synchronise -- what a loop that waits for the result pays.  device_us: device events around the same
calls enqueued behind a workgroup that holds the device for --hold-us, so that the kernels run back to back and the events see device
time (a launch from Python takes longer than these kernels run); null where the host could not enqueue within the hold.  bytes: what the operation has to move
(12 B per element for acc += g, 16 with the scaled copy, 12 + 8 for accumulate + finalize); hbm_fraction: bytes / device time over the
5.1 TB/s the boxes stream -- the 62 MB fit the 256 MB memory-side cache, so this can exceed 1.
Prints one JSON line per variant; --out appends them to a file (profiles/grad_accum_measured.jsonl is the committed measurement).
Run on the GPU:  python tools/grad_accum_time.py --rounds 15
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STREAM_BYTES_PER_S = 5.1e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bands", type=int, default=200)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20, help="back-to-back calls per sample of the kernel / eager / foreach variants")
    ap.add_argument("--foreach-inner", type=int, default=5, help="... of the foreach variants (350 launches per call: the host is the limit)")
    ap.add_argument("--hold-us", type=int, default=6000, help="how long the device is held while the host enqueues a device-time sample")
    ap.add_argument("--max-norm", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("grad_accum_time.py measures on the GPU: no device found")
    from maskedsst_amd import ViTSpatialSpectral, SimMIMSpatialSpectral, GradAccumulator, _lib
    torch.manual_seed(5)
    enc = ViTSpatialSpectral(image_size=8, spatial_patch_size=1, spectral_patch_size=10, num_classes=8, dim=96, depth=args.depth, heads=8,
                             mlp_dim=64, channels=args.bands, spectral_pos_embed=False, spectral_pos=torch.arange(args.bands // 10),
                             precision="bf16")
    model = SimMIMSpatialSpectral(encoder=enc, masking_ratio=0.7, mask_patch_size=4, tube_masking=True,
                                  to_pixels_per_spectral_block=True).cuda().train()
    eng = model.engine()
    eng.ensure()
    fp, lib = eng.fp, _lib.load()
    n = fp.n_trainable
    named = eng.trainable()
    fp.grad.normal_(generator=torch.Generator(device="cuda").manual_seed(7))
    fp.grad.mul_(1e-3)
    accum = fp.accum_buffer()
    accum.copy_(fp.grad)

    def give_grads():   # what a backward leaves: every trainable parameter holds its view of the flat gradient buffer
        for name, p in named:
            p.grad = fp.view(name, fp.grad)

    give_grads()
    grads = [p.grad.reshape(-1) for _, p in named]
    accs = [fp.view(name, accum).reshape(-1) for name, _ in named]
    params = [p for _, p in named]
    table = (_lib.MsstGradRange * 1)(_lib.MsstGradRange(0, n))
    nbytes = ctypes.sizeof(_lib.MsstGradRange)
    scratch = torch.empty(lib.msst_grad_accum_scratch_bytes(1) // 8, dtype=torch.float64, device="cuda")
    record = torch.zeros(4, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    scale, max_norm = 0.25, args.max_norm
    g, a = fp.grad[:n], accum[:n]

    def k_nonfinal():
        _lib.check(lib.msst_grad_accumulate(P(accum), P(fp.grad), table, 1, nbytes, 0, None, 1.0, None, st()), "accumulate")

    def k_final():
        _lib.check(lib.msst_grad_accumulate(P(accum), P(fp.grad), table, 1, nbytes, 0, P(fp.grad), scale, None, st()), "accumulate")

    def k_final_clip():
        _lib.check(lib.msst_grad_accumulate(P(accum), P(fp.grad), table, 1, nbytes, 0, None, 1.0, P(scratch), st()), "accumulate")
        _lib.check(lib.msst_grad_finalize(P(accum), P(fp.grad), table, 1, nbytes, scale, max_norm, P(scratch), P(record), st()), "finalize")

    def e_nonfinal():
        a.add_(g)

    def e_final():
        a.add_(g)
        torch.mul(a, scale, out=g)

    def e_final_clip():
        a.add_(g)
        total = torch.linalg.vector_norm(a) * scale
        coef = torch.clamp(max_norm / (total + 1e-6), max=1.0)
        torch.mul(a, coef * scale, out=g)

    def f_nonfinal():
        torch._foreach_add_(accs, grads)

    def f_final():
        torch._foreach_add_(grads, accs)
        torch._foreach_mul_(grads, scale)

    def f_final_clip():
        torch._foreach_add_(grads, accs)
        torch._foreach_mul_(grads, scale)
        torch.nn.utils.clip_grad_norm_(params, max_norm)

    # GradAccumulator.add(): call 2 of 3 (non-final, first = 0) and call 2 of 2 (final); the calls before it and the gradients a
    # backward would have left are set up outside the timed window
    def add_variant(steps, **kw):
        acc = GradAccumulator(model, steps=steps, **kw)

        def prepare():
            acc.reset()
            give_grads()
            acc.add()
            give_grads()
        return acc.add, prepare

    variants = [
        ("hip_kernel_nonfinal", k_nonfinal, None, args.inner, 12), ("hip_kernel_final", k_final, None, args.inner, 16),
        ("hip_kernel_final_clip", k_final_clip, None, args.inner, 20),
        ("hip_add_nonfinal",) + add_variant(3) + (1, 12), ("hip_add_final",) + add_variant(2) + (1, 16),
        ("hip_add_final_clip",) + add_variant(2, max_norm=max_norm) + (1, 20),
        ("eager_nonfinal", e_nonfinal, None, args.inner, 12), ("eager_final", e_final, None, args.inner, 16),
        ("eager_final_clip", e_final_clip, None, args.inner, 20),
        ("foreach_nonfinal", f_nonfinal, give_grads, args.foreach_inner, 12), ("foreach_final", f_final, give_grads, args.foreach_inner, 16),
        ("foreach_final_clip", f_final_clip, give_grads, args.foreach_inner, 20),
    ]
    dev = {v[0]: [] for v in variants}
    host = {v[0]: [] for v in variants}
    sink = torch.zeros(1, dtype=torch.int32, device="cuda")

    def sample(fn, prepare, inner, hold):
        """-> (device us per call between two events, host us per call up to the synchronise).  hold: one workgroup that waits
        --hold-us is enqueued first, so that the host has enqueued all `inner` calls before the device starts on them and the events
        see device time, not the host's enqueue rate"""
        # the sums grow from call to call: start every sample from the same small values, so that nothing overflows
        accum.copy_(fp.grad.mul_(0).add_(1e-3))
        if prepare is not None:
            prepare()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if hold:
            _lib.check(lib.msst_debug_cu_thief(1, args.hold_us, P(sink), st()), "hold")
        e0.record()
        for _ in range(inner):
            fn()
        t_enq = time.perf_counter()
        e1.record()
        e1.synchronize()
        t1 = time.perf_counter()
        if hold and 1e6 * (t_enq - t0) > args.hold_us:
            return None, None   # the host was slower than the hold: the events would time the host
        return 1e3 * e0.elapsed_time(e1) / inner, 1e6 * (t1 - t0) / inner

    for r in range(args.warmup + args.rounds):
        for name, fn, prepare, inner, _ in variants:
            _, h = sample(fn, prepare, inner, hold=False)
            d, _ = sample(fn, prepare, inner, hold=True)
            if r >= args.warmup:
                host[name].append(h)
                if d is not None:
                    dev[name].append(d)
    lines = []
    for name, _, _, inner, bpe in variants:
        h = statistics.median(host[name])
        line = dict(tool="grad_accum_time", variant=name, elements=n, tensors=len(named), bands=args.bands, depth=args.depth,
                    rounds=args.rounds, inner=inner, host_us=round(h, 2), host_us_min=round(min(host[name]), 2),
                    host_us_max=round(max(host[name]), 2), bytes=bpe * n, device=torch.cuda.get_device_name(0))
        if len(dev[name]) >= max(1, args.rounds // 2):
            d = statistics.median(dev[name])
            line.update(device_us=round(d, 2), device_us_min=round(min(dev[name]), 2), device_us_max=round(max(dev[name]), 2),
                        hbm_fraction=round(bpe * n / (d * 1e-6) / STREAM_BYTES_PER_S, 3))
        else:   # not measured: the host could not enqueue the calls within the hold
            line.update(device_us=None, hbm_fraction=None)
        lines.append(line)
    for line in lines:
        print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
