#!/usr/bin/env python3
"""Timing of SimMIM pre-training on windows read from resident tiles (GPU box): ``SimMIMSpatialSpectral.forward_at`` against the same
step on the stacked copy of the windows, at bench.py's shape (200 bands, depth 12, 8 heads, batch 256, tube masking 0.7, dropout 0.1,
fused AdamW), bf16, 8 x 8 windows out of a pool of 64 x 64 tiles resident on the device.

  at_step        optimizer.zero_grad, model.forward_at(pool, origins, masks, check=False), backward, optimizer step;
  stacked_step   the same step as a caller without forward_at writes it on resident tiles: the windows gathered out of the pool with torch
                 indexing INSIDE the timed step (one advanced-indexing gather into [B, C, 8, 8]), then model(stacked, masks);
  tokenizer_ms   the masked forward tokenizer alone (device events around ten back-to-back calls): at = msst_tokenize_at_fwd_masked on
                 the table, gather = the advanced-indexing copy, batch = msst_tokenize_fwd on the stacked copy;
  head_ms        the masked-L1 head's forward alone, likewise: at = msst_head_at_fwd, batch = msst_head_fwd on the stacked copy.

The pool, the origin table (int32, one position per window, on the device) and the masks are fixed before the clock starts; both steps
upload the same masks.  One process, one model and one optimizer; every leg is warmed up, then the legs are timed alternately, each run
between two device synchronisations (host clock).  Per leg: median and minimum over --steps runs (at least 20).  ``slower`` says whether
the forward_at median exceeds the stacked median by more than the stacked leg's own spread (its median minus its minimum).
``bytes_per_step``: what the stacked copy costs -- its device memory, and what the host loader of pretrain.py sends over PCIe for it --
against the 12 bytes per window of the table.
Prints one JSON line and appends it to --append (default profiles/pretrain_at_measured.jsonl; '' to skip).

Run:  python tools/pretrain_at_time.py [--steps 20] [--warmup 3] [--precision bf16] [--batch 256] [--quick]
--quick: 50 bands, depth 1, batch 16, 3 runs (a smoke run).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from maskedsst_amd import SimMIMSpatialSpectral, ViTSpatialSpectral  # noqa: E402
from maskedsst_amd.data import ResidentTileLoader  # noqa: E402
from maskedsst_amd.engine import Windows  # noqa: E402
from maskedsst_amd.optim import FusedAdamW  # noqa: E402
from forward_at_time import event_ms, gather, timed  # noqa: E402

SEED = 5


def build(args, dev):
    torch.manual_seed(SEED)
    np.random.seed(SEED)
    enc = ViTSpatialSpectral(
        image_size=8, spatial_patch_size=1, spectral_patch_size=10, num_classes=8, dim=96, depth=args.depth, heads=8, mlp_dim=64,
        dropout=args.dropout, emb_dropout=args.dropout, channels=args.bands, spectral_pos_embed=False,
        spectral_pos=torch.arange(args.bands // 10), blockwise_patch_embed=True, spectral_only=False, precision=args.precision)
    model = SimMIMSpatialSpectral(encoder=enc, masking_ratio=0.7, mask_patch_size=4, tube_masking=True,
                                  to_pixels_per_spectral_block=True).to(dev)
    return model.train(), FusedAdamW(model, lr=0.008, weight_decay=0.05, grad_clamp=1.0)


def launches_alone(model, pool, origins, masks, s):
    eng = model.engine()
    mask_u8 = torch.as_tensor(np.asarray(masks[0])).to(device=pool.device, dtype=torch.uint8).contiguous()
    idx32 = torch.as_tensor(np.asarray(masks[1])).to(device=pool.device, dtype=torch.int32).contiguous()
    with torch.no_grad():
        eng.prep_weights()
        stacked, listed = gather(pool, origins, s).contiguous(), Windows("listed", pool, origins)
        y = eng.tokenize(stacked, mask_u8)
        tok = dict(at=event_ms(lambda: eng.tokenize(listed, mask_u8)), gather=event_ms(lambda: gather(pool, origins, s)),
                   batch=event_ms(lambda: eng.tokenize(stacked, mask_u8)))
        head = dict(at=event_ms(lambda: eng.head_fwd(y, listed, idx32)), batch=event_ms(lambda: eng.head_fwd(y, stacked, idx32)))
    return tok, head


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--bands", type=int, default=200)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--dropout", type=float, default=0.1)
    ap.add_argument("--pool-tiles", type=int, default=64)
    ap.add_argument("--append", default=os.path.join(ROOT, "profiles", "pretrain_at_measured.jsonl"))
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    if args.quick:
        args.steps, args.warmup, args.batch, args.bands, args.depth, args.pool_tiles = 3, 1, 16, 50, 1, 4
    if not torch.cuda.is_available():
        raise SystemExit("pretrain_at_time.py needs an MI355X: a timing taken elsewhere says nothing")
    dev = torch.device("cuda")
    model, opt = build(args, dev)
    s = 8
    loader = ResidentTileLoader(args.batch, args.bands, image_size=s, pool_tiles=args.pool_tiles, seed=SEED, device=dev, crop="sample")
    pool, origins = next(loader)
    origins = origins.to(dev).contiguous()
    masks = model.draw_masks(args.batch)

    def at_step():
        opt.zero_grad()
        model.forward_at(pool, origins, masks, check=False).backward()
        opt.step()

    def stacked_step():
        opt.zero_grad()
        model(gather(pool, origins, s), masks).backward()
        opt.step()

    legs = dict(at_step=at_step, stacked_step=stacked_step)
    # the two paths give the same bits (tests/test_gpu_simmim_at.py); checked here once more at the timed size
    model.eval()
    with torch.no_grad():
        same = bool(torch.equal(model.forward_at(pool, origins, masks), model(gather(pool, origins, s), masks)))
    model.train()
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    times = {k: [] for k in legs}
    for _ in range(args.steps):
        for k, fn in legs.items():
            times[k].append(timed(fn))
    res = {k: dict(median_ms=round(1e3 * statistics.median(v), 3), min_ms=round(1e3 * min(v), 3)) for k, v in times.items()}
    spread = res["stacked_step"]["median_ms"] - res["stacked_step"]["min_ms"]
    tok, head = launches_alone(model, pool, origins, masks, s)
    copy = args.batch * args.bands * s * s * 4
    row = dict(tool="pretrain_at_time", window=s, batch=args.batch, pool_tiles=args.pool_tiles, bands=args.bands, depth=args.depth,
               dropout=args.dropout, precision=args.precision, steps=args.steps, warmup=args.warmup, same_bits=same,
               tokenizer_ms=tok, head_ms=head, slower=bool(res["at_step"]["median_ms"] > res["stacked_step"]["median_ms"] + spread),
               bytes_per_step=dict(stacked_copy=copy, origins_table=args.batch * 12), resident_pool_bytes=pool.numel() * 4, **res)
    line = json.dumps(row)
    print(line, flush=True)
    if args.append:
        os.makedirs(os.path.dirname(os.path.abspath(args.append)), exist_ok=True)
        with open(args.append, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
