#!/usr/bin/env python3
"""Reconstruction timing (GPU box): SimMIMSpatialSpectral.reconstruct against its eager restatement, on the SimMIM model of bench.py
(EnMAP shape: 8 x 8 x 200 bands, depth 12, 8 heads, batch 256; masking ratio 0.7, 4 x 4 tube masks, a to_pixels per spectral block).

Both methods run the SAME encoder (the HIP tokenizer and blocks, as Engine.reconstruct runs them); they differ in what
follows the encoder output y [B, T, 96]:
  reconstruct   one launch of msst_recon_fwd: to_pixels over every token, stored into the cube layout, blended with the input, with
                the per-band |pred - img| sums over the masked pixels;
  eager         the same in PyTorch: einsum with the per-block to_pixels weights over all tokens, rearrange to [B, C, H, W],
                torch.where with the expanded mask, masked abs-error sums and counts per band.
Both are warmed up, then timed alternately in one process (device-synchronised wall clock per repetition, median reported), the
two tails also on their own (the same y; ten back-to-back calls between two device events -- y, 126 MB at the default shape,
then comes out of the 256 MB memory-side cache, as it does right after the last block wrote it).  Prints ONE JSON line with
every time and the largest difference between the two results.

Run:  python tools/recon_time.py [--steps 20] [--warmup 3] [--precision bf16] [--batch 256] [--bands 200] [--depth 12]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from maskedsst_amd import ViTSpatialSpectral, SimMIMSpatialSpectral  # noqa: E402

SEED = 5


def build(args, device):
    torch.manual_seed(SEED)
    S = args.bands // 10
    enc = ViTSpatialSpectral(
        image_size=8, spatial_patch_size=1, spectral_patch_size=10, num_classes=8, dim=96, depth=args.depth, heads=args.heads,
        mlp_dim=64, dropout=0.0, emb_dropout=0.0, channels=args.bands, spectral_pos_embed=False, spectral_pos=torch.arange(S),
        blockwise_patch_embed=True, spectral_only=False, precision=args.precision)
    model = SimMIMSpatialSpectral(encoder=enc, masking_ratio=0.7, mask_patch_size=4, tube_masking=True,
                                  to_pixels_per_spectral_block=True)
    return model.to(device).eval()


def encoder_output(eng, img, mask_u8):
    """y [B, T, 96]: the encoder path of Engine.reconstruct"""
    eng.prep_weights()
    acts, _ = eng.blocks_fwd(eng.tokenize(img, mask_u8), save=False)
    return acts[-1]


def eager_tail(model, y, img, mask_u8):
    """to_pixels over all tokens, rearrange, blend, masked abs-error sums: (cube, band_err, band_cnt) like Reconstruction's"""
    enc = model.encoder
    B = y.shape[0]
    S, N, P, s = enc.num_spectral_patches, enc.num_spatial_patches, enc.pixels_per_patch, enc.num_spatial_patches_sqrt
    W = torch.stack([l.weight for l in model.to_pixels.layers])   # [S, P, 96]
    bias = torch.stack([l.bias for l in model.to_pixels.layers])  # [S, P]
    pred = torch.einsum("bsnd,spd->bspn", y.view(B, S, N, 96), W) + bias[None, :, :, None]
    pred = pred.reshape(B, S * P, s, s)
    mask = mask_u8.bool().view(B, S, 1, s, s).expand(B, S, P, s, s).reshape(B, S * P, s, s)
    err = ((pred - img).abs() * mask).double().sum(dim=(2, 3))
    cnt = mask.sum(dim=(2, 3), dtype=torch.int32)
    return torch.where(mask, pred, img), err, cnt


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def event_ms(fn, n=10):
    """ms per call of n back-to-back calls between two device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--bands", type=int, default=200)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--heads", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/recon_time.py needs an MI355X: maskedsst_amd has no CPU fallback")
    device = torch.device("cuda")
    model = build(args, device)
    eng = model.engine()
    gen = torch.Generator().manual_seed(SEED)
    img = torch.randn(args.batch, args.bands, 8, 8, generator=gen).to(device)
    masks = model.draw_masks(args.batch)
    mask_u8 = masks[0].to(device=device, dtype=torch.uint8).contiguous()

    def fast():
        return model.reconstruct(img, masks)

    def slow():
        with torch.no_grad():
            return eager_tail(model, encoder_output(eng, img, mask_u8), img, mask_u8)

    for _ in range(max(1, args.warmup)):
        fast()
        slow()
    tf, ts = [], []
    for _ in range(args.steps):
        t, rec = timed(fast)
        tf.append(t)
        t, (cube, err, cnt) = timed(slow)
        ts.append(t)
    with torch.no_grad():
        y = encoder_output(eng, img, mask_u8)
        tk, te = [], []
        for _ in range(max(1, args.warmup)):
            eng.recon_fwd(y, img, mask_u8, True)
            eager_tail(model, y, img, mask_u8)
        for _ in range(args.steps):
            tk.append(event_ms(lambda: eng.recon_fwd(y, img, mask_u8, True)))
            te.append(event_ms(lambda: eager_tail(model, y, img, mask_u8)))
    mf, ms = statistics.median(tf), statistics.median(ts)
    # bytes msst_recon_fwd has to move: y and img read, the cube written (the mask and the tables are noise)
    moved = 4 * (y.numel() + 2 * img.numel())
    kernel_ms = statistics.median(tk)
    print(json.dumps(dict(
        tool="recon_time", precision=args.precision, bands=args.bands, depth=args.depth, batch=args.batch, steps=args.steps,
        reconstruct_ms=round(1e3 * mf, 3), eager_ms=round(1e3 * ms, 3), reconstruct_ms_min=round(1e3 * min(tf), 3),
        eager_ms_min=round(1e3 * min(ts), 3), recon_kernel_ms=round(kernel_ms, 4), eager_tail_ms=round(statistics.median(te), 4),
        recon_kernel_ms_min=round(min(tk), 4), eager_tail_ms_min=round(min(te), 4),
        recon_kernel_gb_per_s=round(moved / (kernel_ms * 1e-3) / 1e9, 1), recon_kernel_bytes=moved,
        max_abs_cube_diff=float((rec.cube - cube).abs().max()),
        max_rel_band_err_diff=float(((rec.band_err - err).abs() / err.abs().clamp(min=1e-30)).max()),
        band_cnt_equal=bool(torch.equal(rec.band_cnt, cnt)))), flush=True)


if __name__ == "__main__":
    main()
