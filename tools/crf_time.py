#!/usr/bin/env python3
"""CRF refinement time (GPU box): the launches of maskedsst_amd.crf_affinity (msst_crf_affinity) and of one mean-field step
(msst_crf_step) against the eager restatement on the same maps.

Per shape -- a feature map [Bs, 96, Hs, Ws] of planted fields around 50 per channel, score maps [Bs, nc, Hs, Ws], radius R:
  affinity  hip: one launch, k [Bs, K, Hs, Ws] and the live map.  eager: F.normalize, F.pad, F.unfold of the feature map
            ([Bs, 96 (2R+1)^2, rows Ws], in bands of rows so that the unfolded tensor stays under --unfold-gib), the product with the
            centre and the sum over the 96 channels, exp, the tables, the border mask.
  step      hip: one launch from a given Q (probabilities, classes and the changed count).  eager: F.pad and F.unfold of Q
            ([Bs, nc (2R+1)^2, rows Ws], banded the same way), the weighted sum over the neighbours, softmax, argmax.
The eager side handles no dead pixel (the timing maps have none).  Both sides are warmed up, then timed alternately in one process
between device events (the device time of the queued launches, as in tools/gauss_time.py); the medians of --runs runs are reported.
`affinity_tflops` counts the useful products (2 x 96 x K per pixel), `affinity_mfma_tflops` the ones issued (a 16 x 32 block per
tile row and dy, of which the band |dx| <= R is kept); `step_gbs` is the step's compulsory traffic (k, scores, Q in, Q out, classes)
over its time.  No speed bar hangs on this tool; every shape is reported, the ones eager wins included.  Prints ONE JSON line per
shape and appends it to --append (default profiles/crf_measured.jsonl; '' to skip).  --smoke: the smallest shape alone, two runs,
nothing appended.

Run:  python tools/crf_time.py [--runs 20]
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

from maskedsst_amd import crf_affinity  # noqa: E402
from maskedsst_amd.crf import crf_step, crf_tables  # noqa: E402

SEED = 5
REPEAT = 4      # calls queued between two events
SHAPES = [((4, 64, 64), 16), ((1, 512, 512), 16), ((1, 512, 512), 128)]


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


def band_rows(channels, R, Bs, Ws, gib):
    """rows per band so that an unfolded tensor [Bs, channels (2R+1)^2, rows Ws] fp32 stays under gib"""
    return max(1, int(gib * 2 ** 30 / (4.0 * Bs * channels * (2 * R + 1) ** 2 * Ws)))


def neighbours(x, R, y0, h):
    """[Bs, C, K, h Ws]: the K neighbours of the rows y0 .. y0 + h - 1 of x padded by R (zeros), the centre dropped"""
    Bs, C, _, Wp = x.shape
    S = 2 * R + 1
    u = F.unfold(x[:, :, y0:y0 + h + 2 * R], S).view(Bs, C, S * S, h * (Wp - 2 * R))
    cen = R * S + R
    return torch.cat([u[:, :, :cen], u[:, :, cen + 1:]], dim=2)


def eager_affinity(feat, R, a, s, g, gib):
    Bs, _, Hs, Ws = feat.shape
    K = a.numel()
    fn = F.normalize(feat, dim=1)
    pad = F.pad(fn, (R, R, R, R))
    inside = F.pad(torch.ones(1, 1, Hs, Ws, device=feat.device), (R, R, R, R))
    out = torch.empty(Bs, K, Hs, Ws, device=feat.device)
    band = band_rows(96, R, Bs, Ws, gib)
    for y0 in range(0, Hs, band):
        h = min(band, Hs - y0)
        cos = (neighbours(pad, R, y0, h) * fn[:, :, y0:y0 + h].reshape(Bs, 96, 1, h * Ws)).sum(1)
        d2 = (2.0 * (1.0 - cos)).clamp_(min=0)
        kk = (a.view(1, K, 1) * torch.exp(-d2 * g) + s.view(1, K, 1)) * neighbours(inside, R, y0, h)[:, 0]
        out[:, :, y0:y0 + h] = kk.view(Bs, K, h, Ws)
    return out


def eager_step(U, k, q, R, gib):
    Bs, nc, Hs, Ws = U.shape
    K = k.shape[1]
    pad = F.pad(q, (R, R, R, R))
    x = torch.empty_like(U)
    band = band_rows(nc, R, Bs, Ws, gib)
    for y0 in range(0, Hs, band):
        h = min(band, Hs - y0)
        msg = (neighbours(pad, R, y0, h) * k[:, :, y0:y0 + h].reshape(Bs, 1, K, h * Ws)).sum(2)
        x[:, :, y0:y0 + h] = U[:, :, y0:y0 + h] + msg.view(Bs, nc, h, Ws)
    probs = torch.softmax(x, dim=1)
    return probs, probs.argmax(1)


def make_maps(shape, nc, gen, device):
    """planted fields: 16 x 16 blocks share a prototype, plus noise; sharp logits at the block's class"""
    Bs, Hs, Ws = shape
    lab = torch.randint(0, nc, (Bs, (Hs + 15) // 16, (Ws + 15) // 16), generator=gen)
    lab = lab.repeat_interleave(16, 1).repeat_interleave(16, 2)[:, :Hs, :Ws]
    proto = torch.randn(nc, 96, generator=gen) + 50.0
    feat = proto[lab].permute(0, 3, 1, 2) + 0.5 * torch.randn(Bs, 96, Hs, Ws, generator=gen)
    scores = torch.randn(Bs, nc, Hs, Ws, generator=gen) + 4.0 * F.one_hot(lab, nc).permute(0, 3, 1, 2)
    return feat.contiguous().to(device), scores.contiguous().to(device)


def shape_row(shape, nc, R, args, gen, device):
    Bs, Hs, Ws = shape
    feat, scores = make_maps(shape, nc, gen, device)
    a, s = crf_tables(R)
    at, st, g = torch.from_numpy(a).to(device), torch.from_numpy(s).to(device), 2.0
    K, pixels = a.size, Bs * Hs * Ws
    aff_us, eager_aff_us = alternate(lambda: crf_affinity(feat, radius=R), lambda: eager_affinity(feat, R, at, st, g, args.unfold_gib),
                                     args.runs, args.warmup)
    aff = crf_affinity(feat, radius=R)
    k_err = float((aff.weights - eager_affinity(feat, R, at, st, g, args.unfold_gib)).abs().max())
    q0, cls0, _ = crf_step(scores, aff, classes=True)
    step_us, eager_step_us = alternate(lambda: crf_step(scores, aff, q_in=q0, prev_classes=cls0),
                                       lambda: eager_step(scores, aff.weights, q0, R, args.unfold_gib), args.runs, args.warmup)
    q1, cls1, _ = crf_step(scores, aff, q_in=q0, prev_classes=cls0)
    eq, ecls = eager_step(scores, aff.weights, q0, R, args.unfold_gib)
    tiles = Bs * ((Hs + 7) // 8) * ((Ws + 15) // 16)
    issued = tiles * 8 * (2 * R + 1) * 2 * 24 * (2.0 * 16 * 16 * 4)
    step_bytes = 4.0 * pixels * (K + 3 * nc + 2) + pixels
    return dict(tool="crf_time", shape=f"{Bs}x{Hs}x{Ws}", nc=nc, radius=R, runs=args.runs, affinity_us=round(aff_us, 2),
                eager_affinity_us=round(eager_aff_us, 2), affinity_tflops=round(2.0 * 96 * K * pixels / (aff_us * 1e-6) / 1e12, 3),
                affinity_mfma_tflops=round(issued / (aff_us * 1e-6) / 1e12, 3), affinity_max_diff=k_err,
                step_us=round(step_us, 2), eager_step_us=round(eager_step_us, 2), step_gbs=round(step_bytes / (step_us * 1e-6) / 1e9, 1),
                step_max_diff=float((q1 - eq).abs().max()), classes_agree=round(float((cls1.long() == ecls).double().mean()), 5),
                eager_faster_affinity=bool(eager_aff_us < aff_us), eager_faster_step=bool(eager_step_us < step_us))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--radii", default="1,3")
    ap.add_argument("--unfold-gib", type=float, default=1.0, help="the largest unfolded tensor of the eager route, GiB")
    ap.add_argument("--append", default=os.path.join(ROOT, "profiles", "crf_measured.jsonl"))
    ap.add_argument("--smoke", action="store_true", help="the smallest shape alone at radius 1, two runs, nothing appended")
    args = ap.parse_args()
    shapes = SHAPES
    if args.smoke:
        args.runs, args.warmup, args.append, args.radii, shapes = 2, 1, "", "1", SHAPES[:1]
    device = torch.device("cuda")
    gen = torch.Generator().manual_seed(SEED)
    for shape, nc in shapes:
        for R in (int(v) for v in args.radii.split(",")):
            line = json.dumps(shape_row(shape, nc, R, args, gen, device))
            print(line, flush=True)
            if args.append:
                os.makedirs(os.path.dirname(os.path.abspath(args.append)), exist_ok=True)
                with open(args.append, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
