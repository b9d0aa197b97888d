#!/usr/bin/env python3
"""Timing of windows at listed scene positions (GPU box): ``ViTSpatialSpectral.forward_at`` / ``predict_at`` against the same work on the
stacked copy of the windows, at the EnMAP finetune shape of the shipped config (200 bands, depth 4, 8 classes, the config's dropout on),
for a pixelwise model (7 x 7 windows) and the patch head (8 x 8 windows), N = 512 and 2048 windows per step out of 64 x 64 tiles.

  at_step       optimizer.zero_grad, model.forward_at(tiles, origins), F.cross_entropy, backward, optimizer step;
  stacked_step  the same step as a caller without forward_at writes it: the N windows gathered out of the tiles with torch indexing
                INSIDE the timed step (one advanced-indexing gather into [N, C, s, s]), then model(stacked);
  predict_at / predict_stacked   the eval forward and argmax under no_grad: predict_at, and gather + model(stacked) + argmax.

  tokenizer_ms  the tokenizer alone (device events around ten back-to-back calls, eval mode): at = msst_tokenize_at_fwd on the table,
                gather = the advanced-indexing copy, batch = msst_tokenize_fwd on the stacked copy.

Tiles, labels and the origin table (int32, on the device) are resident before the clock starts.  Pixelwise: the table is N rows of
``centre_origins`` (a window per labelled pixel); patch head: N ``random_origins`` with ``window_labels``.  One process, one model and one
optimizer per shape; every leg is warmed up, then the legs are timed alternately, each run between two device synchronisations
(host clock).  Per leg: median and minimum over --steps runs (at least 20).  ``slower`` flags a leg whose forward_at median exceeds the
stacked median by more than the stacked leg's own spread (its median minus its minimum).
Prints one JSON line per shape and appends them to --append (default profiles/forward_at_measured.jsonl; '' to skip).

Run:  python tools/forward_at_time.py [--steps 20] [--warmup 3] [--precision bf16] [--windows 512,2048] [--quick]
--quick: 50 bands, depth 1, 64 windows, 3 runs (a smoke run).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import finetune  # noqa: E402
from maskedsst_amd import ViTSpatialSpectral, centre_origins, random_origins, window_labels  # noqa: E402
from maskedsst_amd.engine import Windows  # noqa: E402


def build(args, device, pixelwise):
    config = finetune.get_finetune_config(os.path.join(ROOT, "configs/finetune_config_enmap.yaml"),
                                          os.path.join(ROOT, "configs/config.yaml"), finetune.SEED, device,
                                          pixelwise=True if pixelwise else None)
    if args.quick:
        config.n_bands, config.transformer_depth = 50, 1
        config.spectral_pos = torch.arange(5)
    torch.manual_seed(finetune.SEED)
    model = ViTSpatialSpectral(
        image_size=config.image_size - config.patch_sub, spatial_patch_size=config.patch_size,
        spectral_patch_size=config.band_patch_size, num_classes=config.n_classes, dim=config.transformer_dim,
        depth=config.transformer_depth, heads=config.transformer_n_heads, mlp_dim=config.transformer_mlp_dim,
        dropout=config.transformer_dropout, emb_dropout=config.transformer_emb_dropout, channels=config.n_bands,
        spectral_pos=config.spectral_pos, spectral_pos_embed=config.spectral_pos_embed,
        blockwise_patch_embed=config.blockwise_patch_embed, spectral_only=config.spectral_only,
        pixelwise=config.pixelwise, pos_embed_len=config.pos_embed_len, precision=args.precision).to(device)
    return config, model


def gather(tiles, origins, s):
    """the stacked copy [n, C, s, s] of the listed windows: one advanced-indexing gather"""
    o = origins.long()
    r = torch.arange(s, device=tiles.device)
    ys = (o[:, 1, None] + r)[:, None, :, None]
    xs = (o[:, 2, None] + r)[:, None, None, :]
    ch = torch.arange(tiles.shape[1], device=tiles.device)[None, :, None, None]
    return tiles[o[:, 0, None, None, None], ch, ys, xs]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def event_ms(fn, n=10):
    """ms per call of n back-to-back calls between two device events"""
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return round(a.elapsed_time(b) / n, 4)


def tokenizer_alone(model, tiles, origins, s):
    eng = model.engine()
    model.eval()
    with torch.no_grad():
        eng.ensure()
        stacked, listed = gather(tiles, origins, s), Windows("listed", tiles, origins)
        return dict(at=event_ms(lambda: eng.tokenize(listed)), gather=event_ms(lambda: gather(tiles, origins, s)),
                    batch=event_ms(lambda: eng.tokenize(stacked)))


def shape_row(args, dev, pixelwise, n):
    config, model = build(args, dev, pixelwise)
    s = config.image_size - config.patch_sub
    gen = torch.Generator().manual_seed(finetune.SEED)
    tiles_n = max(2, -(-n // 1024))   # a 64 x 64 tile has 3364 (3249) window positions; a few tiles per step as in finetune.py
    tiles = torch.randn(tiles_n, config.n_bands, 64, 64, generator=gen)
    label = torch.randint(-1, config.n_classes, (tiles_n, 64, 64), generator=gen)
    if pixelwise:
        origins, labels = centre_origins(label, s, config.ignored_label)
        pick = torch.randperm(origins.shape[0], generator=gen)[:n]
        origins, labels = origins[pick], labels[pick]
    else:
        origins = random_origins(tiles_n, 64, 64, s, n, generator=gen, labels=label, ignore_index=config.ignored_label)
        labels = window_labels(label, origins, s)
    assert origins.shape[0] == n
    tiles, origins, labels = tiles.to(dev), origins.to(dev).contiguous(), labels.to(dev)
    opt = finetune.make_optimizer(model, config, "torch")
    ign = config.ignored_label

    def at_step():
        model.train()
        opt.zero_grad()
        F.cross_entropy(model.forward_at(tiles, origins), labels, ignore_index=ign).backward()
        opt.step()

    def stacked_step():
        model.train()
        opt.zero_grad()
        F.cross_entropy(model(gather(tiles, origins, s)), labels, ignore_index=ign).backward()
        opt.step()

    def predict_at():
        model.predict_at(tiles, origins)

    def predict_stacked():
        model.eval()
        with torch.no_grad():
            model(gather(tiles, origins, s)).argmax(dim=1)

    legs = dict(at_step=at_step, stacked_step=stacked_step, predict_at=predict_at, predict_stacked=predict_stacked)
    # the two paths give the same bits (tests/test_gpu_forward_at.py); checked here once more at the timed size
    model.eval()
    with torch.no_grad():
        same = bool(torch.equal(model.forward_at(tiles, origins), model(gather(tiles, origins, s))))
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    times = {k: [] for k in legs}
    for _ in range(args.steps):
        for k, fn in legs.items():
            times[k].append(timed(fn))
    res = {k: dict(median_ms=round(1e3 * statistics.median(v), 3), min_ms=round(1e3 * min(v), 3)) for k, v in times.items()}
    slower = {}
    for a, b in (("at_step", "stacked_step"), ("predict_at", "predict_stacked")):
        spread = res[b]["median_ms"] - res[b]["min_ms"]
        slower[a] = bool(res[a]["median_ms"] > res[b]["median_ms"] + spread)
    return dict(tool="forward_at_time", head="pixelwise" if pixelwise else "patch", window=s, windows=n, tiles=tiles_n,
                bands=config.n_bands, depth=config.transformer_depth, precision=args.precision, steps=args.steps, warmup=args.warmup,
                same_bits=same, tokenizer_ms=tokenizer_alone(model, tiles, origins, s), stacked_copy_mb=round(n * config.n_bands * s * s * 4 / 2 ** 20, 1), slower=slower, **res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--windows", default="512,2048")
    ap.add_argument("--append", default=os.path.join(ROOT, "profiles", "forward_at_measured.jsonl"))
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    if args.quick:
        args.steps, args.warmup, args.windows = 3, 1, "64"
    if not torch.cuda.is_available():
        raise SystemExit("forward_at_time.py needs an MI355X: a timing taken elsewhere says nothing")
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
