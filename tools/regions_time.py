#!/usr/bin/env python3
"""Connected regions time (GPU box): maskedsst_amd.label_regions (three launches), a 4-round sieve_classes and enforce_connectivity
against two eager routes on the same maps.

Per shape two maps: `blobs` -- a class map of 16 classes, smooth blobs (the nearest of planted points) with 2 % salt-and-pepper pixels:
what a sieve is for -- and `superpixels` -- the label map of a real fit_superpixels run (step 8, a low compactness, so that it has
fragments) on planted fields.
  label     hip: label_regions.
            scipy: scipy.ndimage.label per class on the host, the copy of the map to the host and of the labels back to the device
                   inside the timing (wall clock around a synchronised call: the route leaves the device).
            torch: the minimum index of a region propagated to a fixed point: one channel per value, -index where the pixel holds the
                   value and -inf elsewhere, max_pool2d (3 x 3 for connectivity 8; the larger of a 1 x 3 and a 3 x 1 pool for 4) masked
                   again, until nothing moves (checked every 8 sweeps: a synchronisation each).  fp32 indices: exact below 2^24 pixels.
  sieve     hip: sieve_classes(min_size 8, 4 rounds): 5 labellings and 4 merges, one synchronisation.  The eager side is the LABELLING
            alone, 5 times: a lower bound for an eager sieve, which would add the merge rounds on top.  (blobs only)
  connect   hip: enforce_connectivity(4 rounds), no features.  The eager side as for the sieve.  (superpixels only)
hip and torch are timed between device events (the device time of the queued launches, as in tools/slic_time.py), all three alternately
in one process after a warm-up; the medians of --runs runs are reported.  No speed bar hangs on this tool; every shape is reported, the
ones an eager route wins included.  Prints ONE JSON line per shape and map and appends it to --append (default
profiles/regions_measured.jsonl; '' to skip).  --quick: the smallest shape alone, two runs, nothing appended.

Run:  python tools/regions_time.py [--runs 20]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from maskedsst_amd import enforce_connectivity, fit_superpixels, label_regions, sieve_classes  # noqa: E402

SEED = 5
SHAPES = [(4, 64, 64), (1, 512, 512)]
CLASSES = 16
MIN_SIZE, ROUNDS = 8, 4
CONNECTIVITY = 4


def event_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b)


def wall_us(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t)


def alternate(routes, runs, warmup):
    """routes: {name: (fn, timer)}; the medians in microseconds"""
    for _ in range(warmup):
        for fn, _ in routes.values():
            fn()
    times = {k: [] for k in routes}
    for _ in range(runs):
        for k, (fn, timer) in routes.items():
            times[k].append(timer(fn))
    return {k: statistics.median(v) for k, v in times.items()}


def scipy_label(values, n_values, connectivity=CONNECTIVITY):
    """per value scipy.ndimage.label on the host: (component ids [Bs, Hs, Ws] int64 on the device, -1 dead; regions)"""
    from scipy import ndimage
    v = values.cpu().numpy()
    structure = np.ones((3, 3), dtype=int) if connectivity == 8 else None
    out = np.full(v.shape, -1, dtype=np.int64)
    total = 0
    for b in range(v.shape[0]):
        for c in range(n_values):
            mask = v[b] == c
            if mask.any():
                comp, k = ndimage.label(mask, structure=structure)
                out[b][mask] = comp[mask] + total - 1
                total += k
    return torch.from_numpy(out).to(values.device), total


def torch_label(values, n_values, connectivity=CONNECTIVITY):
    """the minimum index of every region by max_pool2d to a fixed point: labels [Bs, Hs, Ws] int64 in the root form, -1 dead"""
    Bs, Hs, Ws = values.shape
    dev = values.device
    idx = -torch.arange(Hs * Ws, device=dev, dtype=torch.float32).view(1, 1, Hs, Ws)
    mask = values.unsqueeze(1) == torch.arange(n_values, device=dev).view(1, n_values, 1, 1)
    ninf = torch.full((), float("-inf"), device=dev)
    x = torch.where(mask, idx, ninf)
    while True:
        before = x
        for _ in range(8):
            if connectivity == 8:
                y = F.max_pool2d(x, 3, 1, 1)
            else:
                y = torch.maximum(F.max_pool2d(x, (1, 3), 1, (0, 1)), F.max_pool2d(x, (3, 1), 1, (1, 0)))
            x = torch.where(mask, y, ninf)
        if torch.equal(x, before):
            break
    best = x.max(dim=1).values
    return torch.where(torch.isinf(best), torch.full_like(best, 1.0), -best).long() * (values >= 0) - (values < 0).long()


def blobs(shape, gen, device):
    Bs, Hs, Ws = shape
    n = max(8, Hs * Ws // 1024)
    pts = torch.rand(Bs, n, 2, generator=gen) * torch.tensor([Hs, Ws])
    cls = torch.randint(0, CLASSES, (Bs, n), generator=gen)
    yy = torch.arange(Hs).view(1, Hs, 1, 1).float()
    xx = torch.arange(Ws).view(1, 1, Ws, 1).float()
    near = ((yy - pts[:, None, None, :, 0]) ** 2 + (xx - pts[:, None, None, :, 1]) ** 2).argmin(dim=-1)
    v = cls.gather(1, near.view(Bs, -1)).view(Bs, Hs, Ws)
    salt = torch.rand(Bs, Hs, Ws, generator=gen) < 0.02
    return torch.where(salt, torch.randint(0, CLASSES, (Bs, Hs, Ws), generator=gen), v).contiguous().to(device)


def superpixels(shape, gen, device):
    """fit_superpixels (step 8, compactness 0.05) on planted fields: 16 x 16 blocks share a unit prototype, plus noise"""
    Bs, Hs, Ws = shape
    lab = torch.randint(0, 16, (Bs, (Hs + 15) // 16, (Ws + 15) // 16), generator=gen)
    lab = lab.repeat_interleave(16, 1).repeat_interleave(16, 2)[:, :Hs, :Ws]
    proto = F.normalize(torch.randn(16, 96, generator=gen), dim=1)
    feat = F.normalize(proto[lab] + 0.15 * torch.randn(Bs, Hs, Ws, 96, generator=gen), dim=-1).permute(0, 3, 1, 2)
    return fit_superpixels(feat.contiguous().to(device), step=8, compactness=0.05, iters=10)


def same_partition(labels, comp):
    """do the root labels and scipy's component ids describe the same partition?  a bijection between the two on every live pixel"""
    live = labels >= 0
    if not torch.equal(live, comp >= 0):
        return False
    Bs = labels.shape[0]
    plane = labels[0].numel()
    key = (labels + plane * torch.arange(Bs, device=labels.device).view(Bs, 1, 1))[live]
    pairs = torch.unique(torch.stack([key, comp[live]]), dim=1)
    return pairs.shape[1] == torch.unique(key).numel() == torch.unique(comp[live]).numel()


def row(shape, kind, args, gen, device):
    Bs, Hs, Ws = shape
    if kind == "blobs":
        sp, values, n_values = None, blobs(shape, gen, device), CLASSES
    else:
        sp = superpixels(shape, gen, device)
        values, n_values = sp.labels, sp.grid[0] * sp.grid[1]
    t = alternate({"hip": (lambda: label_regions(values, CONNECTIVITY), event_us),
                   "scipy": (lambda: scipy_label(values, n_values), wall_us),
                   "torch": (lambda: torch_label(values, n_values), event_us)}, args.runs, args.warmup)
    reg = label_regions(values, CONNECTIVITY)
    comp, total = scipy_label(values, n_values)
    out = dict(tool="regions_time", shape=f"{Bs}x{Hs}x{Ws}", map=kind, values=n_values, connectivity=CONNECTIVITY, runs=args.runs,
               regions=int(reg.count.sum()), error_word=int(reg.error.cpu()[0]),
               label_us=round(t["hip"], 2), scipy_label_us=round(t["scipy"], 2), torch_label_us=round(t["torch"], 2),
               label_gbs=round(8.0 * values.numel() / (t["hip"] * 1e-6) / 1e9, 2),
               scipy_agrees=bool(total == int(reg.count.sum()) and same_partition(reg.labels, comp)),
               torch_agrees=bool(torch.equal(torch_label(values, n_values), reg.labels)))
    if kind == "blobs":
        fn, name = (lambda: sieve_classes(values, MIN_SIZE, CONNECTIVITY, ROUNDS)), "sieve"
        res = fn()
        out.update(min_size=MIN_SIZE, rounds=ROUNDS, history=res.history.tolist(), regions_after=int(res.regions.count.sum()))
    else:
        fn, name = (lambda: enforce_connectivity(sp, None, CONNECTIVITY, ROUNDS)), "connect"
        res = fn()
        out.update(rounds=ROUNDS, history=res.history.tolist(),
                   fragments_after=int(res.regions.count.sum()) - int((res.superpixels.counts > 0).sum()))
    us = alternate({"hip": (fn, event_us)}, args.runs, args.warmup)["hip"]
    out[name + "_us"] = round(us, 2)
    out["eager_lower_bound_us"] = dict(scipy=round((ROUNDS + 1) * t["scipy"], 2), torch=round((ROUNDS + 1) * t["torch"], 2))
    out["eager_faster_label"] = [k for k in ("scipy", "torch") if t[k] < t["hip"]]
    out["eager_faster_" + name] = [k for k in ("scipy", "torch") if (ROUNDS + 1) * t[k] < us]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--append", default=os.path.join(ROOT, "profiles", "regions_measured.jsonl"))
    ap.add_argument("--quick", action="store_true", help="the smallest shape alone, two runs, nothing appended")
    args = ap.parse_args()
    shapes = SHAPES
    if args.quick:
        args.runs, args.warmup, args.append, shapes = 2, 1, "", SHAPES[:1]
    device = torch.device("cuda")
    gen = torch.Generator().manual_seed(SEED)
    for shape in shapes:
        for kind in ("blobs", "superpixels"):
            line = json.dumps(row(shape, kind, args, gen, device))
            print(line, flush=True)
            if args.append:
                os.makedirs(os.path.dirname(os.path.abspath(args.append)), exist_ok=True)
                with open(args.append, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
