#!/usr/bin/env python3
"""SLIC superpixel time (GPU box): maskedsst_amd.fit_superpixels (msst_slic_assign + msst_slic_update per iteration) and
superpixel_classify (msst_slic_pool, msst_slic_pool_finish, msst_slic_broadcast) against an eager restatement on the same maps.

Per shape -- a unit-length feature map [Bs, 96, Hs, Ws] of planted fields, score maps [Bs, C, Hs, Ws], grid step S:
  fit    hip: 2 (iters + 1) launches and the read of the history.  eager: the home labels; per iteration the nine shifted candidate
         products -- the candidate's centroid gathered per pixel, multiplied with the channel-last copy of the map (made once, outside
         the timing) and summed over the channels, in bands of rows that keep a gathered tensor under --gather-gib -- the spatial
         term, the mask of candidates outside the grid or without rows, `argmax`; then `index_add_` of features, places and counts and
         the division.  The eager side handles no dead pixel (the timing maps have none) and has no fixed tie rule.
  pool   hip: three launches.  eager: `index_add_` of the channel-last score map by label, the division, `argmax`, a gather.
Both sides are warmed up, then timed alternately in one process between device events (the device time of the queued launches, as
in tools/crf_time.py); the medians of --runs runs are reported.  `fit_gbs` is the feature map read once per launch pair, (iters + 1)
times, over the fit's time; `pool_gbs` the score map read once over the pooling's time: bytes over time against what the box
streams.  No speed bar hangs on this tool; every shape is reported, the ones eager wins included.  Prints ONE JSON line per shape and
appends it to --append (default profiles/slic_measured.jsonl; '' to skip).  --quick: the smallest shape alone, two runs, nothing
appended.

Run:  python tools/slic_time.py [--runs 20]
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

from maskedsst_amd import fit_superpixels, superpixel_classify  # noqa: E402
from maskedsst_amd.superpixel import slic_hl  # noqa: E402

SEED = 5
REPEAT = 2      # calls queued between two events
SHAPES = [(4, 64, 64), (1, 512, 512)]
STEPS = [4, 8, 16]
CHANNELS = [16, 128]
COMPACTNESS = 0.2


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPEAT):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / REPEAT


def alternate(fast, slow, runs, warmup):
    for _ in range(warmup):
        fast()
        slow()
    a, b = [], []
    for _ in range(runs):
        a.append(event_ms(fast))
        b.append(event_ms(slow))
    return 1e3 * statistics.median(a), 1e3 * statistics.median(b)      # microseconds


def eager_update(flast, labels, n_sp, gx, S):
    """(centroids [Bs, n_sp, 96], positions [Bs, n_sp, 2] absolute, bias, counts) by index_add_"""
    Bs, Hs, Ws, D = flast.shape
    dev = flast.device
    flat = (labels + n_sp * torch.arange(Bs, device=dev).view(Bs, 1, 1)).reshape(-1)
    sums = torch.zeros(Bs * n_sp, D, device=dev).index_add_(0, flat, flast.reshape(-1, D))
    yy = torch.arange(Hs, device=dev, dtype=torch.float32).view(1, Hs, 1).expand(Bs, Hs, Ws)
    xx = torch.arange(Ws, device=dev, dtype=torch.float32).view(1, 1, Ws).expand(Bs, Hs, Ws)
    pos = torch.zeros(Bs * n_sp, 2, device=dev).index_add_(0, flat, torch.stack([yy, xx], dim=-1).reshape(-1, 2))
    cnt = torch.zeros(Bs * n_sp, device=dev).index_add_(0, flat, torch.ones(flat.numel(), device=dev))
    den = cnt.clamp(min=1).unsqueeze(1)
    cent = sums / den
    return cent.view(Bs, n_sp, D), (pos / den).view(Bs, n_sp, 2), (-0.5 * (cent * cent).sum(1)).view(Bs, n_sp), cnt.view(Bs, n_sp)


def eager_fit(flast, S, hl, iters, gib):
    Bs, Hs, Ws, D = flast.shape
    dev = flast.device
    gy, gx = (Hs + S - 1) // S, (Ws + S - 1) // S
    n_sp = gy * gx
    pi = (torch.arange(Hs, device=dev) // S).view(Hs, 1).expand(Hs, Ws)
    pj = (torch.arange(Ws, device=dev) // S).view(1, Ws).expand(Hs, Ws)
    yy = torch.arange(Hs, device=dev, dtype=torch.float32).view(Hs, 1).expand(Hs, Ws)
    xx = torch.arange(Ws, device=dev, dtype=torch.float32).view(1, Ws).expand(Hs, Ws)
    labels = (pi * gx + pj).unsqueeze(0).expand(Bs, Hs, Ws).contiguous()
    cent, pos, bias, cnt = eager_update(flast, labels, n_sp, gx, S)
    band = max(1, int(gib * 2 ** 30 / (4.0 * Bs * Ws * D)))
    bidx = torch.arange(Bs, device=dev).view(Bs, 1, 1)
    for _ in range(iters):
        new = torch.empty_like(labels)
        for y0 in range(0, Hs, band):
            ys = slice(y0, min(Hs, y0 + band))
            scores, ids = [], []
            for di in (-1, 0, 1):
                for dj in (-1, 0, 1):
                    ci, cj = pi[ys] + di, pj[ys] + dj
                    inside = (ci >= 0) & (ci < gy) & (cj >= 0) & (cj < gx)
                    k = torch.where(inside, ci * gx + cj, torch.zeros_like(ci)).unsqueeze(0).expand(Bs, -1, -1)
                    s = (flast[:, ys] * cent[bidx, k]).sum(-1) + bias[bidx, k] \
                        - hl * ((yy[ys] - pos[bidx, k, 0]) ** 2 + (xx[ys] - pos[bidx, k, 1]) ** 2)
                    ok = inside.unsqueeze(0) & (cnt[bidx, k] > 0)
                    scores.append(torch.where(ok, s, torch.full_like(s, float("-inf"))))
                    ids.append(k)
            pick = torch.stack(scores).argmax(0, keepdim=True)
            new[:, ys] = torch.stack(ids).gather(0, pick)[0]
        labels = new
        c2, p2, b2, cnt = eager_update(flast, labels, n_sp, gx, S)
        has = (cnt > 0).unsqueeze(-1)
        cent, pos, bias = torch.where(has, c2, cent), torch.where(has, p2, pos), torch.where(has[..., 0], b2, bias)
    return labels, cent


def eager_pool(slast, labels, n_sp):
    Bs, Hs, Ws, C = slast.shape
    dev = slast.device
    flat = (labels + n_sp * torch.arange(Bs, device=dev).view(Bs, 1, 1)).reshape(-1)
    sums = torch.zeros(Bs * n_sp, C, device=dev).index_add_(0, flat, slast.reshape(-1, C))
    cnt = torch.zeros(Bs * n_sp, device=dev).index_add_(0, flat, torch.ones(flat.numel(), device=dev))
    table = sums / cnt.unsqueeze(1)
    region = table.nan_to_num(nan=float("-inf")).argmax(1)
    return table.view(Bs, n_sp, C), region[flat].view(Bs, Hs, Ws)


def make_maps(shape, C, gen, device):
    """planted fields: 16 x 16 blocks share a unit prototype, plus noise, renormalised; sharp scores at the block's class"""
    Bs, Hs, Ws = shape
    lab = torch.randint(0, 16, (Bs, (Hs + 15) // 16, (Ws + 15) // 16), generator=gen)
    lab = lab.repeat_interleave(16, 1).repeat_interleave(16, 2)[:, :Hs, :Ws]
    proto = F.normalize(torch.randn(16, 96, generator=gen), dim=1)
    feat = F.normalize(proto[lab] + 0.15 * torch.randn(Bs, Hs, Ws, 96, generator=gen), dim=-1).permute(0, 3, 1, 2)
    scores = torch.randn(Bs, C, Hs, Ws, generator=gen) + 4.0 * F.one_hot(lab % C, C).permute(0, 3, 1, 2)
    return feat.contiguous().to(device), scores.contiguous().to(device)


def shape_row(shape, S, C, args, gen, device):
    Bs, Hs, Ws = shape
    feat, scores = make_maps(shape, C, gen, device)
    flast, slast = feat.permute(0, 2, 3, 1).contiguous(), scores.permute(0, 2, 3, 1).contiguous()
    hl = slic_hl(COMPACTNESS, S)
    fit_us, eager_fit_us = alternate(lambda: fit_superpixels(feat, step=S, compactness=COMPACTNESS, iters=args.iters),
                                     lambda: eager_fit(flast, S, hl, args.iters, args.gather_gib), args.runs, args.warmup)
    sp = fit_superpixels(feat, step=S, compactness=COMPACTNESS, iters=args.iters)
    elab, _ = eager_fit(flast, S, hl, args.iters, args.gather_gib)
    n_sp = sp.grid[0] * sp.grid[1]
    pool_us, eager_pool_us = alternate(lambda: superpixel_classify(sp, scores), lambda: eager_pool(slast, sp.labels, n_sp), args.runs, args.warmup)
    res = superpixel_classify(sp, scores)
    etab, ecls = eager_pool(slast, sp.labels, n_sp)
    both = ~torch.isnan(etab) & ~torch.isnan(res.region_scores)
    map_bytes, score_bytes = 4.0 * feat.numel(), 4.0 * scores.numel()
    return dict(tool="slic_time", shape=f"{Bs}x{Hs}x{Ws}", step=S, channels=C, iters=args.iters, runs=args.runs, superpixels=Bs * n_sp,
                fit_us=round(fit_us, 2), eager_fit_us=round(eager_fit_us, 2),
                fit_gbs=round((args.iters + 1) * map_bytes / (fit_us * 1e-6) / 1e9, 1),
                labels_agree=round(float((sp.labels == elab).double().mean()), 5), moved_last=int(sp.history[-1, 0]) if args.iters else 0,
                pool_us=round(pool_us, 2), eager_pool_us=round(eager_pool_us, 2), pool_gbs=round(score_bytes / (pool_us * 1e-6) / 1e9, 1),
                pool_max_diff=float((res.region_scores - etab)[both].abs().max()),
                classes_agree=round(float((res.classes == ecls).double().mean()), 5),
                eager_faster_fit=bool(eager_fit_us < fit_us), eager_faster_pool=bool(eager_pool_us < pool_us))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10, help="iterations of a fit (the API default)")
    ap.add_argument("--gather-gib", type=float, default=1.0, help="the largest gathered tensor of the eager route, GiB")
    ap.add_argument("--append", default=os.path.join(ROOT, "profiles", "slic_measured.jsonl"))
    ap.add_argument("--quick", action="store_true", help="the smallest shape alone at step 8 and 16 channels, two runs, nothing appended")
    args = ap.parse_args()
    shapes, steps, channels = SHAPES, STEPS, CHANNELS
    if args.quick:
        args.runs, args.warmup, args.append, shapes, steps, channels = 2, 1, "", SHAPES[:1], [8], [16]
    device = torch.device("cuda")
    gen = torch.Generator().manual_seed(SEED)
    for shape in shapes:
        for S in steps:
            for C in channels:
                line = json.dumps(shape_row(shape, S, C, args, gen, device))
                print(line, flush=True)
                if args.append:
                    os.makedirs(os.path.dirname(os.path.abspath(args.append)), exist_ok=True)
                    with open(args.append, "a") as f:
                        f.write(line + "\n")


if __name__ == "__main__":
    main()
