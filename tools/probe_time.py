#!/usr/bin/env python3
"""Linear-probe timing (GPU box): fit_linear_probe (msst_probe_grad + msst_probe_update) against its eager restatement and against
linear_eval steps.

Per bank size M (rows [M, 96] of random features, --classes classes) one FIT of --fit-steps full-batch steps is timed two ways on the
same cached bank:
  probe   maskedsst_amd.fit_linear_probe: 2 launches per step, no host synchronisation before the history's read-back;
  eager   what a user writes in PyTorch: F.layer_norm, F.linear, F.cross_entropy, autograd and torch.optim.Adam on four leaf tensors.
Both are warmed up, then timed alternately in one process between device events (the device time of the queued launches, as in
tools/knn_time.py); the medians of --steps runs are reported.  One linear_eval step (the frozen body forward on --batch windows, the
head-only backward, FusedAdam; the encoder of --depth blocks on --bands bands) is timed the same way, and a fit is expressed in
linear_eval steps of equal time.  The two launches of a step are also timed apart (--split-launches of each between two events):
what folding the update into the next gradient launch could save at most is the step's time minus their sum.  No speed bar hangs
on this tool.  Prints ONE JSON line and appends it to --append (default profiles/probe_measured.jsonl; '' to skip).  --smoke: a tiny
shape, nothing appended.

Run:  python tools/probe_time.py [--banks 8192,262144] [--classes 16] [--fit-steps 100] [--steps 20]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from maskedsst_amd import KnnBank, LinearProbe, ViTSpatialSpectral, _lib, fit_linear_probe  # noqa: E402
from maskedsst_amd.features import _p, _stream  # noqa: E402

SEED = 5


def eager_fit(x, y, nc, steps, lr):
    g = torch.ones(96, device=x.device, requires_grad=True)
    b = torch.zeros(96, device=x.device, requires_grad=True)
    W = torch.zeros(nc, 96, device=x.device, requires_grad=True)
    c = torch.zeros(nc, device=x.device, requires_grad=True)
    opt = torch.optim.Adam([g, b, W, c], lr=lr)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss = F.cross_entropy(F.linear(F.layer_norm(x, (96,), g, b, 1e-5), W, c), y)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    return torch.stack(losses).cpu()          # one read-back, as the probe's history


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def alternate(fast, slow, steps, warmup):
    for _ in range(warmup):
        fast()
        slow()
    a, b = [], []
    for _ in range(steps):
        t, rf = event_ms(fast)
        a.append(t)
        t, rs = event_ms(slow)
        b.append(t)
    return statistics.median(a), statistics.median(b), rf, rs


def split_us(bank, n, runs):
    """median device time in microseconds of one msst_probe_grad launch, one msst_probe_update launch and one step (both), each from
    n launches queued between two events"""
    lib = _lib.load()
    M, nc = len(bank), bank.n_classes
    theta = torch.zeros(2 * 96 + 97 * nc, device=bank.features.device)
    theta[:96] = 1.0
    probe = LinearProbe(theta, nc)
    nslab = int(lib.msst_probe_scratch_floats(M, nc))
    slab = torch.empty(nslab, device=theta.device)
    hist = torch.empty(4, device=theta.device)
    st = _stream()

    def grad():
        _lib.check(lib.msst_probe_grad(_p(bank.features), _p(bank.labels), None, _p(probe.theta), M, 96, 0, M, nc, _p(slab), nslab, st),
                   "msst_probe_grad")

    def update():
        _lib.check(lib.msst_probe_update(_p(slab), nslab, M, 96, nc, _p(probe.theta), _p(probe.m), _p(probe.v), _p(probe.step), 1e-2, 0.9,
                                         0.999, 1e-8, 0.0, _p(hist), None, 1, st), "msst_probe_update")

    def both():
        grad()
        update()

    def many(fn):
        return lambda: [fn() for _ in range(n)]

    legs = [many(grad), many(update), many(both)]
    for leg in legs:
        leg()
    t = [[] for _ in legs]
    for _ in range(runs):
        for i, leg in enumerate(legs):
            t[i].append(1e3 * event_ms(leg)[0] / n)
    return [round(statistics.median(v), 2) for v in t]


def linear_eval_step_ms(args, device, gen):
    from maskedsst_amd.optim import FusedAdam
    torch.manual_seed(SEED)
    model = ViTSpatialSpectral(
        image_size=8, spatial_patch_size=1, spectral_patch_size=10, num_classes=args.classes, dim=96, depth=args.depth, heads=8, mlp_dim=64,
        dropout=0.0, emb_dropout=0.0, channels=args.bands, spectral_pos_embed=False, spectral_pos=torch.arange(args.bands // 10),
        blockwise_patch_embed=True, spectral_only=False, precision=args.precision).to(device).train()
    head = []
    for n, p in model.named_parameters():
        p.requires_grad_("mlp_head" in n)
        if "mlp_head" in n:
            head.append(p)
    opt = FusedAdam(model, head, lr=args.lr, weight_decay=0.0)
    img = torch.randn(args.batch, args.bands, 8, 8, generator=gen).to(device)
    label = torch.randint(0, args.classes, (args.batch, 8, 8), generator=gen).to(device)

    def step():
        opt.zero_grad()
        F.cross_entropy(model(img), label).backward()
        opt.step()

    for _ in range(args.warmup + 1):
        step()
    return statistics.median(event_ms(step)[0] for _ in range(args.steps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--banks", default="8192,262144", help="comma separated bank sizes M")
    ap.add_argument("--classes", type=int, default=16)
    ap.add_argument("--fit-steps", type=int, default=100)
    ap.add_argument("--lr", type=float, default=1e-2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--batch", type=int, default=256, help="windows per linear_eval step")
    ap.add_argument("--bands", type=int, default=200)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--split-launches", type=int, default=50, help="launches between two events when the two kernels are timed apart")
    ap.add_argument("--append", default=os.path.join(ROOT, "profiles", "probe_measured.jsonl"))
    ap.add_argument("--smoke", action="store_true", help="a tiny shape, two runs, nothing appended")
    args = ap.parse_args()
    if args.smoke:
        args.banks, args.classes, args.fit_steps, args.steps, args.warmup = "300", 5, 5, 2, 1
        args.batch, args.bands, args.depth, args.append, args.split_launches = 8, 50, 1, "", 3
    device = torch.device("cuda")
    gen = torch.Generator().manual_seed(SEED)
    le_ms = linear_eval_step_ms(args, device, gen)
    nc = args.classes
    rows = []
    for M in (int(v) for v in args.banks.split(",")):
        y = torch.randint(0, nc, (M,), generator=gen)
        x = (0.6 * torch.randn(nc, 96, generator=gen)[y] + torch.randn(M, 96, generator=gen) + 0.3).to(device)
        y = y.to(device)
        bank = KnnBank(x, y, nc)
        fast = lambda: fit_linear_probe(bank, steps=args.fit_steps, lr=args.lr)     # noqa: E731
        slow = lambda: eager_fit(x, y, nc, args.fit_steps, args.lr)                   # noqa: E731
        tf, ts, probe, losses = alternate(fast, slow, args.steps, args.warmup)
        grad_us, update_us, both_us = split_us(bank, args.split_launches, max(3, args.steps // 2))
        rows.append(dict(M=M, n_classes=nc, fit_steps=args.fit_steps, fit_ms=round(tf, 4), eager_fit_ms=round(ts, 4),
                         grad_launch_us=grad_us, update_launch_us=update_us, step_launches_us=both_us,
                         step_us=round(1e3 * tf / args.fit_steps, 3), eager_step_us=round(1e3 * ts / args.fit_steps, 3),
                         bank_stream_GBps=round(M * 96 * 4 * args.fit_steps / (tf * 1e-3) / 1e9, 1),
                         last_loss=float(probe.history[-1, 0]), eager_last_loss=float(losses[-1]),
                         linear_eval_step_ms=round(le_ms, 4), linear_eval_steps_per_fit=round(tf / le_ms, 3)))
    row = dict(tool="probe_time", precision=args.precision, bands=args.bands, depth=args.depth, batch=args.batch, steps=args.steps,
               lr=args.lr, results=rows)
    line = json.dumps(row)
    print(line, flush=True)
    if args.append:
        os.makedirs(os.path.dirname(os.path.abspath(args.append)), exist_ok=True)
        with open(args.append, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
