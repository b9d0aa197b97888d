#!/usr/bin/env python3
"""Timing of scene gradients through overlapping windows (GPU box): ``maskedsst_amd.scene_saliency`` against the route a caller
without it writes, at the EnMAP finetune shape of the shipped config (200 bands, depth 4, 8 classes) on 64 x 64 tiles: the patch head
(8 x 8 windows) at stride 8 and stride 4, and a pixelwise model (7 x 7 windows) at stride 1.

  scene_saliency  predict_scene for the class map, then per chunk forward_at on the windows in place, backward, msst_tokenize_at_bwd_input
                  and msst_scene_fold_at into the one map;
  stacked         the eager route on the same class map and weights: every window gathered out of the tiles with torch indexing into
                  [n, C, s, s] (the stacked copy), maskedsst_amd.input_gradient's autograd on it (eval, frozen), and index_add_ of the
                  per-window gradients back into the scene -- predict_scene included, as in scene_saliency;
  launches_ms     the two new launches alone (device events around ten back-to-back calls): at_bwd_input = msst_tokenize_at_bwd_input,
                  fold = msst_scene_fold_at, csr = scene.origins_csr (torch ops), index_add = the eager scatter of the same dwin.

Everything is resident before the clock starts.  One process and one model per shape; both legs are warmed up, then timed alternately,
each run between two device synchronisations (host clock).  Per leg: median and minimum over --steps runs (at least 20).  ``slower``
flags scene_saliency when its median exceeds the stacked median by more than the stacked leg's own spread (median minus minimum).
stacked_copy_mb is what the stacked route holds beside the scene and scene_saliency does not: the copy of the windows (its gradient of
the same size comes out of both routes, as dwin here).
Prints one JSON line per shape and appends them to --append (default profiles/scene_saliency_measured.jsonl; '' to skip).

Run:  python tools/scene_saliency_time.py [--steps 20] [--warmup 3] [--precision bf16] [--tiles 2] [--quick]
--quick: 50 bands, depth 1, 3 runs (a smoke run).
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from forward_at_time import build, event_ms, gather, timed  # noqa: E402
from maskedsst_amd import scene_saliency  # noqa: E402
from maskedsst_amd.saliency import _Frozen  # noqa: E402
from maskedsst_amd.scene import origins_csr  # noqa: E402


def grid_origins(Bs, Hs, Ws, w, stride, dev):
    nr, nq = (Hs - w) // stride + 1, (Ws - w) // stride + 1
    k = torch.arange(Bs * nr * nq, device=dev)
    return torch.stack((k // (nr * nq), k % (nr * nq) // nq * stride, k % nq * stride), dim=1).to(torch.int32).contiguous()


def scatter_back(dwin, origins, shape, s):
    """index_add_ of per-window gradients [n, C, s, s] into a scene-shaped map: the eager accumulating scatter (atomics on the device)"""
    Bs, C, Hs, Ws = shape
    o = origins.long()
    r = torch.arange(s, device=dwin.device)
    pix = (o[:, 0, None, None] * Hs + o[:, 1, None, None] + r[None, :, None]) * Ws + o[:, 2, None, None] + r[None, None, :]   # [n, s, s]
    out = torch.zeros(Bs * Hs * Ws, C, dtype=torch.float32, device=dwin.device)
    out.index_add_(0, pix.reshape(-1), dwin.permute(0, 2, 3, 1).reshape(-1, C))
    return out.view(Bs, Hs, Ws, C).permute(0, 3, 1, 2)


def stacked_saliency(model, tiles, stride, pix):
    """the eager route: the class map, then stack every window, autograd on the stack, scatter back"""
    s, nc = model.num_spatial_patches_sqrt, model.num_classes
    Bs, C, Hs, Ws = tiles.shape
    classes = model.predict_scene(tiles, stride=stride)
    origins = grid_origins(Bs, Hs, Ws, s, stride, tiles.device)
    n = origins.shape[0]
    o = origins.long()
    r = torch.arange(s, device=tiles.device)
    if pix:
        at = (o[:, 0], o[:, 1] + s // 2, o[:, 2] + s // 2)
        idx, wgt = classes[at].clamp(min=0).view(n, 1), torch.ones(n, 1, device=tiles.device)
    else:
        at = (o[:, 0, None, None], (o[:, 1, None] + r)[:, :, None], (o[:, 2, None] + r)[:, None, :])
        cover = scatter_back(torch.ones(n, 1, s, s, device=tiles.device), origins, (Bs, 1, Hs, Ws), s)[:, 0]
        idx, wgt = classes[at].clamp(min=0).view(n, 1, s, s), (1.0 / cover.clamp(min=1))[at].view(n, 1, s, s)
    was = model.training
    model.eval()
    with _Frozen(model), torch.enable_grad():
        x = gather(tiles, origins, s).requires_grad_(True)
        out = model(x).view((n, nc) if pix else (n, nc, s, s))
        (out.gather(1, idx) * wgt).sum().backward()
    model.train(was)
    return scatter_back(x.grad, origins, tiles.shape, s)


def launches_alone(model, tiles, stride):
    eng = model.engine()
    eng.ensure()
    s = model.num_spatial_patches_sqrt
    Bs, C, Hs, Ws = tiles.shape
    origins = grid_origins(Bs, Hs, Ws, s, stride, tiles.device)
    n = origins.shape[0]
    csr = origins_csr(origins, Bs, Hs, Ws)
    dx0 = torch.randn(n, eng.S * eng.N, 96, device=tiles.device)
    dwin = torch.randn(n, C, s, s, device=tiles.device)
    out = torch.empty_like(tiles)
    import ctypes
    from maskedsst_amd import _lib
    V = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)   # noqa: E731

    def at_bwd_input():
        _lib.check(eng.lib.msst_tokenize_at_bwd_input(V(tiles), V(origins), *eng._tok_params(), V(dx0), V(dwin), Bs, Hs, Ws, s, n, eng.S, eng.P,
                                                      0.0, 0, st()), "msst_tokenize_at_bwd_input")

    def fold():
        _lib.check(eng.lib.msst_scene_fold_at(V(dwin), V(csr[0]), V(csr[1]), V(out), Bs, C, Hs, Ws, s, n, eng.P, 0, st()), "msst_scene_fold_at")

    return dict(at_bwd_input=event_ms(at_bwd_input), fold=event_ms(fold), csr=event_ms(lambda: origins_csr(origins, Bs, Hs, Ws)),
                index_add=event_ms(lambda: scatter_back(dwin, origins, tiles.shape, s)))


def shape_row(args, dev, pixelwise, stride):
    config, model = build(args, dev, pixelwise)
    s = config.image_size - config.patch_sub
    gen = torch.Generator().manual_seed(7)
    tiles = torch.randn(args.tiles, config.n_bands, 64, 64, generator=gen).to(dev)
    model.eval()
    legs = dict(scene_saliency=lambda: scene_saliency(model, tiles, stride=stride),
                stacked=lambda: stacked_saliency(model, tiles, stride, pixelwise))
    a, b = legs["scene_saliency"]().grad, legs["stacked"]()
    rel = float((a - b).abs().max() / b.abs().max())   # the eager scatter adds in no fixed order: agreement, not equal bits
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    times = {k: [] for k in legs}
    for _ in range(args.steps):
        for k, fn in legs.items():
            times[k].append(timed(fn))
    res = {k: dict(median_ms=round(1e3 * statistics.median(v), 3), min_ms=round(1e3 * min(v), 3)) for k, v in times.items()}
    spread = res["stacked"]["median_ms"] - res["stacked"]["min_ms"]
    n = args.tiles * ((64 - s) // stride + 1) ** 2
    return dict(tool="scene_saliency_time", head="pixelwise" if pixelwise else "patch", window=s, stride=stride, tiles=args.tiles,
                windows=n, bands=config.n_bands, depth=config.transformer_depth, precision=args.precision, steps=args.steps,
                warmup=args.warmup, max_rel_diff=rel, launches_ms=launches_alone(model, tiles, stride),
                stacked_copy_mb=round(n * config.n_bands * s * s * 4 / 2 ** 20, 1), scene_mb=round(tiles.numel() * 4 / 2 ** 20, 1),
                slower=bool(res["scene_saliency"]["median_ms"] > res["stacked"]["median_ms"] + spread), **res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--tiles", type=int, default=2)
    ap.add_argument("--append", default=os.path.join(ROOT, "profiles", "scene_saliency_measured.jsonl"))
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    if args.quick:
        args.steps, args.warmup = 3, 1
    if not torch.cuda.is_available():
        raise SystemExit("scene_saliency_time.py needs an MI355X: a timing taken elsewhere says nothing")
    dev = torch.device("cuda")
    for pixelwise, stride in ((False, 8), (False, 4), (True, 1)):
        line = json.dumps(shape_row(args, dev, pixelwise, stride))
        print(line, flush=True)
        if args.append:
            os.makedirs(os.path.dirname(os.path.abspath(args.append)), exist_ok=True)
            with open(args.append, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
