#!/usr/bin/env python3
"""Finetune step timing (GPU box) at the EnMAP finetune shape of the shipped config (200 bands, depth 4, 8 classes, image_size 8),
B = 256, training mode (the config's dropout on):

    ms per step (forward + backward + optimizer) of {full finetune, linear_eval} x {torch.optim.Adam, FusedAdam},
    and the peak of allocated memory over one step of each leg, above what was allocated before it.

Every leg has a model and an optimizer of its own, built the way finetune.py builds them at this revision (``make_optimizer``; a
revision without it: Adam over body + head, two learning rates, as its finetune.py does).  All legs are warmed up, then timed
alternately in one process with HIP events around each step; a repetition reports the median step, the result the median of the
repetitions and their spread.  Legs whose pieces a revision lacks (no ``FusedAdam``) are left out, so the tool also runs on an
older tree: that is where a baseline comes from.

``--loss torch | fused | both``: a step is then ``maskedsst_amd.utils.train_step`` as finetune.py runs it -- the loss, the accuracy
numbers and the NaN check with their host synchronisations, not the bare ``F.cross_entropy`` of the default -- with
``torch.nn.CrossEntropyLoss`` or ``maskedsst_amd.ops.FusedCrossEntropy`` (finetune.py --loss); ``both`` gives every leg twice
(``...+loss_torch`` / ``...+loss_fused``), alternated step by step in the one process.  ``--legs`` keeps the legs whose name contains
one of the given words.

``--shifting-window``: the shifting_window step instead -- ``--tiles`` 64 x 64 tiles per step (4: 256 windows), full finetune with
torch.optim.Adam, the bare ``F.cross_entropy`` step; two legs on ONE model, alternated step by step: ``tiles`` =
``model.forward_windows(tiles)`` (the windows read out of the resident tiles), ``stacked`` = ``model(stack_windows(tiles, 8))`` -- stack_image_batch's image half --
(the stacked copy made inside the timed step, as a caller without forward_windows has to).

Prints ONE JSON line.  Run:  python tools/finetune_time.py [--steps 20] [--reps 3] [--warmup 5] [--precision bf16] [--batch 256]
                                                           [--loss both] [--legs linear_eval+fused full+torch]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import finetune  # noqa: E402
from maskedsst_amd import ViTSpatialSpectral  # noqa: E402
from maskedsst_amd.utils import train_step  # noqa: E402


def build(precision, device, linear_eval):
    config = finetune.get_finetune_config(os.path.join(ROOT, "configs/finetune_config_enmap.yaml"),
                                          os.path.join(ROOT, "configs/config.yaml"), finetune.SEED, device)
    config.linear_eval = linear_eval
    torch.manual_seed(finetune.SEED)
    model = ViTSpatialSpectral(
        image_size=config.image_size - config.patch_sub, spatial_patch_size=config.patch_size,
        spectral_patch_size=config.band_patch_size, num_classes=config.n_classes, dim=config.transformer_dim,
        depth=config.transformer_depth, heads=config.transformer_n_heads, mlp_dim=config.transformer_mlp_dim,
        dropout=config.transformer_dropout, emb_dropout=config.transformer_emb_dropout, channels=config.n_bands,
        spectral_pos=config.spectral_pos, spectral_pos_embed=config.spectral_pos_embed,
        blockwise_patch_embed=config.blockwise_patch_embed, spectral_only=config.spectral_only,
        pixelwise=config.pixelwise, pos_embed_len=config.pos_embed_len, precision=precision).to(device)
    if linear_eval:
        for n, p in model.named_parameters():
            p.requires_grad_("mlp_head" in n)
    return config, model.train()


def optimizer(model, config, kind):
    """finetune.py's optimizer at this revision; None when the revision has no such leg"""
    if hasattr(finetune, "make_optimizer"):
        return finetune.make_optimizer(model, config, kind)
    if kind != "torch":
        return None
    head = [p for n, p in model.named_parameters() if "mlp_head" in n]
    body = [p for n, p in model.named_parameters() if "mlp_head" not in n]
    return torch.optim.Adam([{"params": body}, {"params": head, "lr": config.mlp_head_lr}], lr=config.lr, weight_decay=config.weight_decay)


def criterion(loss, config):
    """finetune.py's criterion for --loss; None: the bare F.cross_entropy step.  ImportError: the revision has no fused loss"""
    if loss is None:
        return None
    if loss == "fused":
        from maskedsst_amd.ops import FusedCrossEntropy
        return FusedCrossEntropy(ignore_index=config.ignored_label)
    return torch.nn.CrossEntropyLoss(ignore_index=config.ignored_label)


def box_probe(model):
    """shader clock (MHz) and MFMA rate this box holds right now (msst_debug_box_probe); {} when the library has no probe"""
    lib = model.engine().lib
    if not hasattr(lib, "msst_debug_box_probe"):
        return {}
    out = (ctypes.c_double * 4)()
    scratch = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
    rc = lib.msst_debug_box_probe(out, ctypes.c_void_p(scratch.data_ptr()), scratch.numel(),
                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return {} if rc else dict(mfma_tflops=round(out[0], 1), shader_mhz=round(out[1], 1))


def shifting_window(args, dev):
    from maskedsst_amd.utils import stack_windows
    config, model = build(args.precision, dev, False)
    opt = optimizer(model, config, "torch")
    gen = torch.Generator().manual_seed(finetune.SEED)
    tiles = torch.randn(args.tiles, config.n_bands, 64, 64, generator=gen).to(dev)
    label = torch.randint(-1, config.n_classes, (args.tiles, 64, 64), generator=gen).to(dev)
    size = config.image_size - config.patch_sub
    slabel = stack_windows(label, size).contiguous()

    def step(name):
        opt.zero_grad()
        if name == "tiles":
            out = model.forward_windows(tiles)
        else:
            out = model(stack_windows(tiles, size).contiguous())   # the image alone: the labels are stacked once, outside
        F.cross_entropy(out, slabel, ignore_index=-1).backward()
        opt.step()

    legs = ("tiles", "stacked")
    for _ in range(args.warmup):
        for name in legs:
            step(name)
    probe = box_probe(model)
    reps = {name: [] for name in legs}
    for _ in range(args.reps):
        t = {name: [] for name in legs}
        for _ in range(args.steps):
            for name in legs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                step(name)
                e1.record()
                e1.synchronize()
                t[name].append(e0.elapsed_time(e1))
        for name in legs:
            reps[name].append(round(statistics.median(t[name]), 4))
    res = dict(tool="finetune_time", mode="shifting_window",
               shape=dict(tiles=args.tiles, windows=int(slabel.shape[0]), bands=config.n_bands, depth=config.transformer_depth,
                          n_classes=config.n_classes, image_size=config.image_size),
               precision=args.precision, steps=args.steps, warmup=args.warmup, box_probe=probe,
               step_ms={name: round(statistics.median(v), 4) for name, v in reps.items()}, step_ms_reps=reps,
               step_ms_spread={name: round(max(v) - min(v), 4) for name, v in reps.items()})
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--loss", default=None, choices=["torch", "fused", "both"],
                    help="time utils.train_step with this criterion (default: the bare F.cross_entropy step)")
    ap.add_argument("--legs", nargs="*", default=None, help="keep the legs whose name contains one of these words")
    ap.add_argument("--shifting-window", action="store_true", help="time the tile path against the stacked copy (see above)")
    ap.add_argument("--tiles", type=int, default=4, help="--shifting-window: 64 x 64 tiles per step")
    args = ap.parse_args()
    dev = torch.device("cuda")
    if args.shifting_window:
        return shifting_window(args, dev)
    legs = {}
    losses = [None] if args.loss is None else ["torch", "fused"] if args.loss == "both" else [args.loss]
    for mode, linear_eval in (("full", False), ("linear_eval", True)):
        for kind in ("torch", "fused"):
            for loss in losses:
                name = f"{mode}+{kind}" + (f"+loss_{loss}" if loss else "")
                if args.legs and not any(w in name for w in args.legs):
                    continue
                config, model = build(args.precision, dev, linear_eval)
                try:
                    opt = optimizer(model, config, kind)
                    crit = criterion(loss, config)
                except ImportError:
                    opt = None
                if opt is not None:
                    legs[name] = (model, opt, crit, config)
    if not legs:
        raise SystemExit("no leg left: this revision lacks the pieces, or --legs matches nothing")
    gen = torch.Generator().manual_seed(finetune.SEED)
    size = config.image_size - config.patch_sub
    x = torch.randn(args.batch, config.n_bands, size, size, generator=gen).to(dev)
    label = torch.randint(-1, config.n_classes, (args.batch, size, size), generator=gen).to(dev)

    def step(name):
        model, opt, crit, cfg = legs[name]
        if crit is not None:
            train_step(x, label, model, cfg, dev, crit, opt)
            return
        opt.zero_grad()
        F.cross_entropy(model(x), label, ignore_index=-1).backward()
        opt.step()

    for _ in range(args.warmup):
        for name in legs:
            step(name)
    probe = box_probe(next(iter(legs.values()))[0])
    peak = {}
    for name in legs:
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        step(name)
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() - base
    reps = {name: [] for name in legs}
    for _ in range(args.reps):
        t = {name: [] for name in legs}
        for _ in range(args.steps):
            for name in legs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                step(name)
                e1.record()
                e1.synchronize()
                t[name].append(e0.elapsed_time(e1))
        for name in legs:
            reps[name].append(round(statistics.median(t[name]), 4))
    res = dict(tool="finetune_time", shape=dict(B=args.batch, bands=config.n_bands, depth=config.transformer_depth,
                                                n_classes=config.n_classes, image_size=size),
               precision=args.precision, loss=args.loss, steps=args.steps, warmup=args.warmup, box_probe=probe,
               step_ms={name: round(statistics.median(v), 4) for name, v in reps.items()},
               step_ms_reps=reps, step_ms_spread={name: round(max(v) - min(v), 4) for name, v in reps.items()},
               peak_step_bytes=peak)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
