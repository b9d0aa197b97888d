#!/usr/bin/env python3
"""Timing of D4 augmentation on windows at listed scene positions (GPU box): ``forward_at(..., orient=)`` against the same step without
the keyword, at the EnMAP finetune shape of the shipped config (200 bands, depth 4, 8 classes, the config's dropout on), for a pixelwise
model (7 x 7 windows) and the patch head (8 x 8 windows), N = 512 and 2048 windows per step out of 64 x 64 tiles.

  plain_step    optimizer.zero_grad, model.forward_at(tiles, origins), F.cross_entropy, backward, optimizer step: the step as it runs
                without this feature (the un-oriented entry points);
  orient_step   the same step with orient = random codes 0 .. 7 (drawn once, resident) and the labels of the oriented windows;
  eager_step    the augmentation as a caller without the keyword writes it: the N windows gathered out of the tiles with torch
                indexing INSIDE the timed step, ``orient_windows`` of the copy, then model(stacked); ``eager_copy_mb`` is what it
                holds (the gathered copy and the oriented one).

  tokenizer_ms  the oriented tokenizer launch alone (device events around ten back-to-back calls, eval mode): plain = the un-oriented
                entry point; code0 = every window in code 0 through the oriented one; flip = code 4 (a pure left-right flip: steps
                +Ws, -1); transpose = code 5 (steps 1, +Ws: reads Ws floats apart along j); random = the step's codes.

Tiles, labels, the origin table and the codes are resident before the clock starts.  One process, one model and one optimizer per
shape; every leg is warmed up, then the legs are timed alternately, each run between two device synchronisations (host clock).  Per leg:
median and minimum over --steps runs (at least 20).  ``slower`` flags orient_step when its median exceeds plain_step's by more than
plain_step's own spread (its median minus its minimum).  Prints one JSON line per shape and appends them to --append (default
profiles/orient_measured.jsonl; '' to skip).

Run:  python tools/orient_time.py [--steps 20] [--warmup 3] [--precision bf16] [--windows 512,2048] [--quick]
--quick: 50 bands, depth 1, 64 windows, 3 runs (a smoke run).  Give the process a time limit of its own (timeout -k 10 600 ...).
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import finetune  # noqa: E402
from forward_at_time import build, event_ms, gather, timed  # noqa: E402
from maskedsst_amd import centre_origins, orient_windows, random_orients, random_origins, window_labels  # noqa: E402
from maskedsst_amd.engine import Windows  # noqa: E402


def tokenizer_alone(model, tiles, origins, orient):
    eng = model.engine()
    model.eval()
    with torch.no_grad():
        eng.ensure()
        full = lambda code: torch.full_like(orient, code)   # noqa: E731
        legs = dict(plain=Windows("listed", tiles, origins), code0=Windows("listed", tiles, origins, orient=full(0)),
                    flip=Windows("listed", tiles, origins, orient=full(4)), transpose=Windows("listed", tiles, origins, orient=full(5)),
                    random=Windows("listed", tiles, origins, orient=orient))
        return {k: event_ms(lambda src=src: eng.tokenize(src)) for k, src in legs.items()}


def shape_row(args, dev, pixelwise, n):
    config, model = build(args, dev, pixelwise)
    s = config.image_size - config.patch_sub
    gen = torch.Generator().manual_seed(finetune.SEED)
    tiles_n = max(2, -(-n // 1024))
    tiles = torch.randn(tiles_n, config.n_bands, 64, 64, generator=gen)
    label = torch.randint(-1, config.n_classes, (tiles_n, 64, 64), generator=gen)
    if pixelwise:
        origins, labels = centre_origins(label, s, config.ignored_label)
        pick = torch.randperm(origins.shape[0], generator=gen)[:n]
        origins, labels = origins[pick], labels[pick]
        orient = random_orients(n, generator=gen)
        labels_o = labels   # the centre of an odd window is a fixed point of every orientation
    else:
        origins = random_origins(tiles_n, 64, 64, s, n, generator=gen, labels=label, ignore_index=config.ignored_label)
        labels = window_labels(label, origins, s)
        orient = random_orients(n, generator=gen)
        labels_o = window_labels(label, origins, s, orient)
    assert origins.shape[0] == n
    tiles, origins, orient = tiles.to(dev), origins.to(dev).contiguous(), orient.to(dev)
    labels, labels_o = labels.to(dev), labels_o.to(dev)
    opt = finetune.make_optimizer(model, config, "torch")
    ign = config.ignored_label

    def step(forward, lab):
        model.train()
        opt.zero_grad()
        F.cross_entropy(forward(), lab, ignore_index=ign).backward()
        opt.step()

    legs = dict(plain_step=lambda: step(lambda: model.forward_at(tiles, origins), labels),
                orient_step=lambda: step(lambda: model.forward_at(tiles, origins, orient=orient), labels_o),
                eager_step=lambda: step(lambda: model(orient_windows(gather(tiles, origins, s), orient)), labels_o))
    # the two augmented paths give the same bits (tests/test_gpu_orient.py); checked here once more at the timed size
    model.eval()
    with torch.no_grad():
        same = bool(torch.equal(model.forward_at(tiles, origins, orient=orient), model(orient_windows(gather(tiles, origins, s), orient))))
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    times = {k: [] for k in legs}
    for _ in range(args.steps):
        for k, fn in legs.items():
            times[k].append(timed(fn))
    res = {k: dict(median_ms=round(1e3 * statistics.median(v), 3), min_ms=round(1e3 * min(v), 3)) for k, v in times.items()}
    spread = res["plain_step"]["median_ms"] - res["plain_step"]["min_ms"]
    slower = bool(res["orient_step"]["median_ms"] > res["plain_step"]["median_ms"] + spread)
    return dict(tool="orient_time", head="pixelwise" if pixelwise else "patch", window=s, windows=n, tiles=tiles_n, bands=config.n_bands,
                depth=config.transformer_depth, precision=args.precision, steps=args.steps, warmup=args.warmup, same_bits=same,
                tokenizer_ms=tokenizer_alone(model, tiles, origins, orient),
                eager_copy_mb=round(2 * n * config.n_bands * s * s * 4 / 2 ** 20, 1), slower=dict(orient_step=slower), **res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--windows", default="512,2048")
    ap.add_argument("--append", default=os.path.join(ROOT, "profiles", "orient_measured.jsonl"))
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    if args.quick:
        args.steps, args.warmup, args.windows = 3, 1, "64"
    if not torch.cuda.is_available():
        raise SystemExit("orient_time.py needs an MI355X: a timing taken elsewhere says nothing")
    dev = torch.device("cuda")
    for pixelwise in (True, False):
        for n in [int(v) for v in args.windows.split(",")]:
            line = json.dumps(shape_row(args, dev, pixelwise, n))
            print(line, flush=True)
            if args.append:
                os.makedirs(os.path.dirname(os.path.abspath(args.append)), exist_ok=True)
                with open(args.append, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
