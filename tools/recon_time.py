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

--scene: whole-tile reconstruction instead.  SimMIMSpatialSpectral.reconstruct_scene on --tiles tiles of --tile-size x --tile-size
(default 4 of 64 x 64; non-overlapping 8 x 8 windows, one random mask per window placed in tile coordinates) against the path
there was before it: the windows stacked into a batch (a copy), reconstruct on it, the cube re-tiled and the per-window tables summed
per tile in PyTorch.  Alternated in one process, median of --steps per repetition, --reps repetitions; msst_scene_recon_assemble and
the masked scene tokenizer also on their own between device events.  ONE JSON line (tool = "recon_scene_time"); --append FILE also
appends it to FILE.
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


def scene_main(args, device):
    import ctypes
    from maskedsst_amd import window_masks_to_scene
    from maskedsst_amd.engine import _p, _stream
    model = build(args, device)
    eng = model.engine()
    enc = model.encoder
    S, P, C, B, ts, w = enc.num_spectral_patches, enc.pixels_per_patch, args.bands, args.tiles, args.tile_size, 8
    nr = nq = ts // w
    nwin = B * nr * nq
    gen = torch.Generator().manual_seed(SEED)
    tiles = torch.randn(B, C, ts, ts, generator=gen).to(device)
    bm = model.draw_masks(nwin)[0]
    scene_mask = window_masks_to_scene(bm, B, S, ts, ts, w).to(device)

    def fast():
        return model.reconstruct_scene(tiles, scene_mask)

    def slow():
        stacked = tiles[:, :, :nr * w, :nq * w].reshape(B, C, nr, w, nq, w).permute(0, 2, 4, 1, 3, 5).reshape(nwin, C, w, w).contiguous()
        rec = model.reconstruct(stacked, bm)
        cube = tiles.clone()   # trailing rows / columns no window covers keep the input
        cube[:, :, :nr * w, :nq * w] = rec.cube.view(B, nr, nq, C, w, w).permute(0, 3, 1, 4, 2, 5).reshape(B, C, nr * w, nq * w)
        return cube, rec.band_err.view(B, nr * nq, C).sum(1), rec.band_cnt.view(B, nr * nq, C).sum(1, dtype=torch.int32)

    for _ in range(max(1, args.warmup)):
        fast()
        slow()
    reps = []
    for _ in range(args.reps):
        tf, ts_ = [], []
        for _ in range(args.steps):
            t, rec = timed(fast)
            tf.append(t)
            t, (cube, err, cnt) = timed(slow)
            ts_.append(t)
        reps.append((statistics.median(tf), statistics.median(ts_), min(tf), min(ts_)))
    # the two new kernels on their own: the assembler (accumulate + finalize) on the per-window predictions, the masked tokenizer
    stacked = tiles[:, :, :nr * w, :nq * w].reshape(B, C, nr, w, nq, w).permute(0, 2, 4, 1, 3, 5).reshape(nwin, C, w, w).contiguous()
    win_recon = model.reconstruct(stacked, bm, blend=False).cube.contiguous()
    mask_u8 = scene_mask.to(torch.uint8).contiguous()
    out = torch.empty(B, C, ts, ts, device=device)
    e2, c2 = torch.empty(B, C, dtype=torch.float64, device=device), torch.empty(B, C, dtype=torch.int32, device=device)
    cov = torch.empty(B, ts, ts, dtype=torch.int32, device=device)
    tok = torch.empty(nwin, S * w * w, 96, device=device)

    def assemble():
        rc = eng.lib.msst_scene_recon_assemble(_p(win_recon), 0, nwin, _p(tiles), _p(mask_u8), _p(out), _p(e2), _p(c2), _p(cov), B, S, P,
                                               ts, ts, w, w, 1, 1, _stream())
        assert rc == 0, rc

    def tokenize():
        eng.tokenize_scene_masked(tiles, mask_u8, w, 0, nwin, out=tok)

    ta, tt = [], []
    for _ in range(max(1, args.warmup)):
        assemble()
        tokenize()
    for _ in range(args.steps):
        ta.append(event_ms(assemble))
        tt.append(event_ms(tokenize))
    torch.cuda.synchronize()
    moved = 4 * (win_recon.numel() + 3 * out.numel() + tiles.numel()) + mask_u8.numel() * P   # accumulate: read + write; finalize: cube r/w, scene, mask per band
    row = dict(
        tool="recon_scene_time", precision=args.precision, bands=args.bands, depth=args.depth, tiles=B, tile_size=ts, windows=nwin,
        steps=args.steps, reps=args.reps,
        reconstruct_scene_ms=[round(1e3 * r[0], 3) for r in reps], stacked_ms=[round(1e3 * r[1], 3) for r in reps],
        reconstruct_scene_ms_min=[round(1e3 * r[2], 3) for r in reps], stacked_ms_min=[round(1e3 * r[3], 3) for r in reps],
        assemble_kernels_ms=round(statistics.median(ta), 4), assemble_kernels_ms_min=round(min(ta), 4), assemble_bytes=moved,
        masked_tokenizer_ms=round(statistics.median(tt), 4), masked_tokenizer_ms_min=round(min(tt), 4),
        cube_equal=bool(torch.equal(rec.cube, cube)), assembled_equal=bool(torch.equal(out, cube)),
        max_rel_band_err_diff=float(((rec.band_err - err).abs() / err.abs().clamp(min=1e-30)).max()),
        band_cnt_equal=bool(torch.equal(rec.band_cnt, cnt)))
    line = json.dumps(row)
    print(line, flush=True)
    if args.append:
        os.makedirs(os.path.dirname(os.path.abspath(args.append)), exist_ok=True)
        with open(args.append, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--bands", type=int, default=200)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--scene", action="store_true", help="time reconstruct_scene on whole tiles against the stacked-window path")
    ap.add_argument("--tiles", type=int, default=4)
    ap.add_argument("--tile-size", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--append", default=None, help="--scene: also append the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/recon_time.py needs an MI355X: maskedsst_amd has no CPU fallback")
    device = torch.device("cuda")
    if args.scene:
        return scene_main(args, device)
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
