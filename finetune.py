#!/usr/bin/env python3
"""Finetune entry point (mirror of the reference's ``finetune.py`` for the ViTSpatialSpectral method) on the
MI355X-native kernels: build the encoder, optionally initialise it from a SimMIM checkpoint
(``load_checkpoint``), train the pixel-wise classification head with CE(ignore_index=-1).

The labelled GeoTIFF readers are out of scope: ``--synthetic`` (default) draws standardised random tiles and
random labels in {-1 .. n_classes-1}, which exercises the identical compute path (BASELINE config 5 checks the
logits / loss / gradients of that path against the CPU reference in tests/test_gpu_finetune.py).

``shifting_window: True`` in the config, or ``--shifting-window``: a step trains on every non-overlapping window of its 64 x 64
tiles (64 windows of 8 x 8 per tile; 81 of 7 x 7 with ``--pixelwise``) instead of one random crop per tile, as the reference's
``train_step`` does; the windows are read out of the tiles on the device (``ViTSpatialSpectral.forward_windows``), and the
samples/s printed count windows."""
import argparse
import random
import sys
import time

import numpy as np
import torch
import yaml

from maskedsst_amd import ViTSpatialSpectral
from maskedsst_amd.config import Dotdict, parse_flag
from maskedsst_amd.utils import get_spectral_pos_embedding, load_checkpoint, train_step

SEED = 5


def get_finetune_config(path, general_path, seed, device, pixelwise=None, shifting_window=None):
    """reference src/utils.py:337-364 (ViTSpatialSpectral branch; worldcover/dfc spectral positions).  pixelwise: overrides
    the config's flag before patch_sub is derived from it (None: the config's value).  shifting_window: overrides the config's
    flag (None: the config's value, read as the reference reads it, src/utils.py:254-257)."""
    hp = yaml.safe_load(open(path))
    if pixelwise is not None:
        hp["pixelwise"] = bool(pixelwise)
    hp["shifting_window"] = parse_flag(hp.get("shifting_window", False)) if shifting_window is None else bool(shifting_window)
    general = yaml.safe_load(open(general_path))
    hp.update(general["data"][hp["dataset"]])
    hp.update(general["transformer"])
    hp["seed"], hp["device"] = seed, device
    if hp["method_name"] != "ViTSpatialSpectral":
        raise NotImplementedError("only the ViTSpatialSpectral method is built (the DeepHyperX 'li' baseline is out of scope)")
    if hp["dataset"] == "houston2018":
        # the two sensors' band-centre tables live with the (out of scope) readers: the config carries the lookup's result
        hp["spectral_pos"] = torch.as_tensor(hp["spectral_pos"])
        assert len(hp["spectral_pos"]) == hp["n_bands"] // hp["band_patch_size"]
    else:
        hp["spectral_pos"] = get_spectral_pos_embedding(hp["dataset"], hp["n_bands"], hp["band_patch_size"])
    hp["patch_sub"] = 1 if (hp["pixelwise"] and hp["image_size"] % 2 == 0) else 0
    return Dotdict(hp)


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("dataset", nargs="?", default="enmap", choices=["enmap", "houston2018"])   # reference finetune.py:42-46
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--batch-size", type=int, default=None)
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--val-scenes", type=int, default=0,
                    help="validate on N held-out synthetic 64 x 64 scenes with predict_scene (0: no validation)")
    ap.add_argument("--val-every", type=int, default=0, help="validate every K steps (0: no validation)")
    ap.add_argument("--spectral-mlp-head", action="store_true",
                    help="classify from the S spectral tokens of a position concatenated (reference spectral_mlp_head=True); a "
                         "--checkpoint must come from an encoder built with the same head (pretrain.py --spectral-mlp-head)")
    ap.add_argument("--pixelwise", action="store_true",
                    help="the centre-pixel classifier (reference pixelwise=True): windows of image_size - 1 (odd), one class "
                         "per window; --val-scenes then predicts dense per-pixel maps (stride 1)")
    ap.add_argument("--shifting-window", action="store_true", default=None,
                    help="train on every non-overlapping window of each 64 x 64 tile at once (reference shifting_window=True; overrides "
                         "the config's shifting_window) instead of one random crop per tile")
    ap.add_argument("--train-at", default=None, choices=["labelled", "random"],
                    help="train on windows at listed positions of the step's resident tiles (ViTSpatialSpectral.forward_at, the reference's "
                         "Houston2018 sampling): labelled -- windows centred at labelled pixels, one class each (pixelwise models); random "
                         "-- windows at random positions that hold a labelled pixel (patch heads)")
    ap.add_argument("--windows-per-step", type=int, default=512, metavar="N", help="windows drawn per step under --train-at")
    ap.add_argument("--augment", default=None, choices=["d4"],
                    help="with --train-at: every listed window is read in a random one of its eight orientations (flips and quarter "
                         "turns, forward_at(..., orient=)): applied where the kernels form the window's address, no copy")
    ap.add_argument("--val-tta", action="store_true",
                    help="with --val-at: test-time augmentation, predict_at(..., tta='d4') -- the mean of the logits over the eight "
                         "orientations of every window")
    ap.add_argument("--val-at", action="store_true",
                    help="validate with predict_at on the windows centred at the validation tiles' labelled pixels (--val-scenes defaults "
                         "to 2 and --val-every to --steps when they are not given)")
    ap.add_argument("--linear-eval", action="store_true", default=None,
                    help="linear evaluation (reference finetune.py:110-136; overrides the config's linear_eval): everything outside "
                         "mlp_head is frozen, the optimizer sees the head only, the step runs no block or tokenizer backward")
    ap.add_argument("--optimizer", default="torch", choices=["torch", "fused"],
                    help="torch: torch.optim.Adam; fused: maskedsst_amd.optim.FusedAdam (the same update, one launch per step)")
    ap.add_argument("--loss", default="torch", choices=["torch", "fused"],
                    help="torch: torch.nn.CrossEntropyLoss and eager accuracy; fused: maskedsst_amd.ops.FusedCrossEntropy (loss, gradient, "
                         "accuracy and macro accuracy from one pass of the HIP loss kernels, one read-back per step; also in validation)")
    ap.add_argument("--class-weights", default="none", choices=["none", "inverse"],
                    help="inverse: weight every class by 1 / its frequency among the first step's non-ignored labels, normalised to "
                         "mean 1 over the classes present there, 0 for an absent class (CrossEntropyLoss(weight=), both --loss kinds)")
    ap.add_argument("--label-smoothing", type=float, default=0.0, metavar="EPS", help="CrossEntropyLoss(label_smoothing=EPS), in [0, 1)")
    ap.add_argument("--val-report", action="store_true",
                    help="one more line per validation: overall and average accuracy, Cohen's kappa and mean IoU from the confusion "
                         "matrix of the same pass of the HIP loss kernels (maskedsst_amd.scene.scene_report)")
    ap.add_argument("--val-embed", action="store_true",
                    help="one more line per validation: nearest-class-mean accuracy on the frozen per-pixel features of "
                         "encode_scene(normalize=True); class means from the first half of the --val-scenes, scored on the second half")
    ap.add_argument("--val-knn", type=int, default=0, metavar="K",
                    help="one more line per validation: accuracy of the weighted K-nearest-neighbour classifier (maskedsst_amd.knn_classify, "
                         "temperature 0.07) on the same frozen features and the same split as --val-embed: the bank is the first half of "
                         "the --val-scenes, scored on the second half; needs --val-scenes and --val-every")
    ap.add_argument("--val-probe", type=int, default=0, metavar="STEPS",
                    help="one more line per validation: accuracy of a linear probe (maskedsst_amd.fit_linear_probe: LayerNorm -> Linear "
                         "trained for STEPS full-batch Adam steps at lr 1e-2 on cached features) on the raw frozen features and the split "
                         "of --val-embed: the bank is the first half of the --val-scenes, scored on the second half; needs --val-scenes "
                         "and --val-every")
    ap.add_argument("--val-cluster", type=int, default=0, metavar="K",
                    help="one more line per validation: the clustering score of the frozen features, no label used for the fit: k-means "
                         "(maskedsst_amd.fit_kmeans, K clusters, cosine, k-means++) on the covered pixels of the first half of the "
                         "--val-scenes, the second half assigned and matched to the classes (Hungarian accuracy, purity, NMI); the split "
                         "of --val-embed; needs --val-scenes and --val-every")
    ap.add_argument("--val-gmm", type=int, default=0, metavar="K",
                    help="one more line per validation: the clustering score of a Gaussian mixture of the raw frozen features, no label "
                         "used for the fit: EM (maskedsst_amd.fit_mixture, K components, k-means init) on the covered pixels of the first "
                         "half of the --val-scenes, the second half assigned and matched to the classes as under --val-cluster, with the "
                         "mean log-likelihood of the second half; needs --val-scenes and --val-every")
    ap.add_argument("--val-gmm-cov", default="full", choices=["full", "diag"], help="the covariances of --val-gmm")
    ap.add_argument("--val-pca", type=int, default=0, metavar="R",
                    help="one more line per validation: the spectrum of the frozen features' covariance, no label read: "
                         "maskedsst_amd.fit_pca on the covered pixels of the first half of the --val-scenes (the R leading "
                         "explained-variance ratios and the effective rank), then the mean and largest RX anomaly score of the second "
                         "half under that fit; needs --val-scenes and --val-every")
    ap.add_argument("--val-gauss", default=None, choices=["full", "tied"], metavar="{full,tied}",
                    help="one more line per validation: accuracy of the class-conditional Gaussian classifier (maskedsst_amd.fit_gaussian: "
                         "full covariances = QDA, a tied one = LDA) on the raw frozen features and the split of --val-knn: the bank is the "
                         "first half of the --val-scenes, scored on the second half, with the mean distance to the predicted class and the "
                         "share of pixels farther than the bank's 0.99 quantile; needs --val-scenes and --val-every")
    ap.add_argument("--val-crf", type=int, default=0, metavar="ITERS",
                    help="one more line per validation: the accuracy of the class map before and after ITERS mean-field steps of the "
                         "feature-guided CRF (maskedsst_amd.crf_affinity / crf_refine at the API defaults) over predict_scene's logits "
                         "and one encode_scene pass on the --val-scenes, and the pixels whose class changed; needs --val-scenes and "
                         "--val-every")
    ap.add_argument("--val-crf-radius", type=int, default=2, metavar="R", help="the neighbourhood radius of --val-crf, 1 .. 3")
    ap.add_argument("--val-superpixel", type=int, default=0, metavar="STEP",
                    help="one more line per validation: the accuracy of the class map before and after object-based classification -- "
                         "SLIC superpixels (maskedsst_amd.fit_superpixels, grid step STEP in {4, 8, 16}, the API defaults otherwise) of "
                         "one encode_scene pass on the --val-scenes, predict_scene's logits pooled per superpixel "
                         "(superpixel_classify) -- and the pixels whose class changed; needs --val-scenes and --val-every")
    ap.add_argument("--val-superpixel-compactness", type=float, default=0.2, metavar="M",
                    help="the compactness of --val-superpixel: the weight of a step's distance against a unit of feature distance")
    ap.add_argument("--val-superpixel-connect", action="store_true",
                    help="with --val-superpixel: one more line after it, the superpixels after SLIC's connectivity pass "
                         "(maskedsst_amd.enforce_connectivity): the orphan pieces before and after, and the accuracy of the object-based "
                         "map on the connected superpixels")
    ap.add_argument("--val-sieve", type=int, default=0, metavar="MIN_SIZE",
                    help="one more line per validation: the sieve (minimum mapping unit, maskedsst_amd.sieve_classes) on predict_scene's "
                         "class maps of the --val-scenes -- connected patches of fewer than MIN_SIZE pixels merged into their largest "
                         "neighbour -- with the regions and the accuracy before and after; needs --val-scenes and --val-every")
    ap.add_argument("--val-sieve-connectivity", type=int, default=4, choices=(4, 8), help="the connectivity of --val-sieve")
    ap.add_argument("--val-saliency", action="store_true",
                    help="one more line per validation: the five bands with the largest mean |gradient x input| attribution "
                         "(maskedsst_amd.band_importance, argmax class) over the windows of the --val-scenes")
    ap.add_argument("--val-saliency-scene", action="store_true",
                    help="one more line per validation: the five bands with the largest mean |gradient x input| attribution of the "
                         "whole --val-scenes' class maps (maskedsst_amd.band_importance_scene: the overlapping windows of predict_scene "
                         "read in place, their input gradients folded into the scene); needs --val-scenes")
    ap.add_argument("--val-attention", action="store_true",
                    help="one more line per validation: the three spectral blocks that receive the most rollout attention "
                         "(maskedsst_amd.attention_rollout of model.attention_maps(stack='spectral')) over the first batch of windows "
                         "of the --val-scenes")
    ap.add_argument("--accumulate", type=int, default=1, metavar="K",
                    help="sum the gradients of K micro-steps of batch_size // K tiles (--train-at: windows_per_step // K windows) before "
                         "each optimizer step (maskedsst_amd.GradAccumulator); --steps counts optimizer steps")
    ap.add_argument("--clip-norm", type=float, default=None, metavar="X",
                    help="clip the (accumulated) gradient to the global L2 norm X before the optimizer step (clip_grad_norm_, fused)")
    return ap


def inverse_frequency_weights(label, n_classes, ignored_label):
    """--class-weights inverse: 1 / frequency of each class among the labels of `label` that are not ignored (and lie in
    [0, n_classes)), normalised to mean 1 over the classes present, 0 for a class that is absent.  -> float32 [n_classes] (CPU)"""
    lab = label.reshape(-1)
    lab = lab[(lab != ignored_label) & (lab >= 0) & (lab < n_classes)]
    count = torch.bincount(lab, minlength=n_classes).double()
    present = count > 0
    w = torch.zeros(n_classes, dtype=torch.float64)
    if present.any():
        w[present] = count.sum() / count[present]
        w /= w[present].mean()
    return w.float()


def make_criterion(kind, ignored_label, weight=None, label_smoothing=0.0):
    """reference finetune.py:136: CrossEntropyLoss(ignore_index=ignored_label); weight / label_smoothing: the DeepHyperX protocol's
    CrossEntropyLoss(weight=...) (reference DeepHyperX/models.py:37-72) and torch's label smoothing, on either kind"""
    if kind == "fused":
        from maskedsst_amd.ops import FusedCrossEntropy
        return FusedCrossEntropy(ignore_index=ignored_label, weight=weight, label_smoothing=label_smoothing)
    if weight is None and not label_smoothing:
        return torch.nn.CrossEntropyLoss(ignore_index=ignored_label)
    return torch.nn.CrossEntropyLoss(weight=weight, ignore_index=ignored_label, label_smoothing=label_smoothing)


def make_optimizer(model, config, kind):
    """reference finetune.py:110-136: Adam with coupled L2 decay; two learning rates (lr for the body, mlp_head_lr for the head), or
    under linear_eval the head parameters alone, at lr as there"""
    head = [p for n, p in model.named_parameters() if "mlp_head" in n]
    body = [p for n, p in model.named_parameters() if "mlp_head" not in n]
    if config.linear_eval:
        groups = head
    else:
        groups = [{"params": body}, {"params": head, "lr": config.mlp_head_lr}]
    if kind == "fused":
        from maskedsst_amd.optim import FusedAdam
        return FusedAdam(model, groups, lr=config.lr, weight_decay=config.weight_decay)
    return torch.optim.Adam(groups, lr=config.lr, weight_decay=config.weight_decay)


def main():
    args = build_parser().parse_args()
    if args.augment and not args.train_at:
        raise SystemExit("--augment d4 orients windows at listed positions: it needs --train-at")
    if args.val_tta and not args.val_at:
        raise SystemExit("--val-tta averages predict_at over the eight orientations: it needs --val-at")
    random.seed(SEED); np.random.seed(SEED); torch.manual_seed(SEED)
    if not torch.cuda.is_available():
        raise SystemExit("finetune.py needs an MI355X: maskedsst_amd has no CPU fallback")
    device = torch.device("cuda")
    config = get_finetune_config(f"configs/finetune_config_{args.dataset}.yaml", "configs/config.yaml", SEED, device,
                                 pixelwise=True if args.pixelwise else None, shifting_window=args.shifting_window)
    if args.batch_size:
        config.batch_size = args.batch_size
    if args.linear_eval is not None:
        config.linear_eval = args.linear_eval
    if args.checkpoint:
        config.checkpoint_path = args.checkpoint
        if config.pixelwise and config.patch_sub and not config.spectral_pos_embed and config.pos_embed_len is None:
            # the checkpoint's pos_embedding has the image_size x image_size length: the reference's strict load needs
            # pos_embed_len set to it (the model reads its first S N rows)
            config.pos_embed_len = config.n_bands // config.band_patch_size * config.image_size ** 2 + 1
    model = ViTSpatialSpectral(
        image_size=config.image_size - config.patch_sub, spatial_patch_size=config.patch_size,
        spectral_patch_size=config.band_patch_size, num_classes=config.n_classes, dim=config.transformer_dim,
        depth=config.transformer_depth, heads=config.transformer_n_heads, mlp_dim=config.transformer_mlp_dim,
        dropout=config.transformer_dropout, emb_dropout=config.transformer_emb_dropout, channels=config.n_bands,
        spectral_pos=config.spectral_pos, spectral_pos_embed=config.spectral_pos_embed,
        blockwise_patch_embed=config.blockwise_patch_embed, spectral_only=config.spectral_only,
        pixelwise=config.pixelwise, pos_embed_len=config.pos_embed_len, spectral_mlp_head=args.spectral_mlp_head,
        precision=args.precision)
    if config.checkpoint_path is not None:
        model = load_checkpoint(config, model, "mlp_head", "cpu")
    model.to(device)
    if config.linear_eval:
        for n, p in model.named_parameters():
            p.requires_grad_("mlp_head" in n)
    optimizer = make_optimizer(model, config, args.optimizer)
    accumulator, micro, micro_windows = make_accumulator(model, args.accumulate, args.clip_norm, config.batch_size, args.windows_per_step,
                                                         bool(args.train_at))
    if args.train_at == "labelled" and not config.pixelwise:
        raise SystemExit("--train-at labelled draws one class per window: it needs a pixelwise model (--pixelwise)")
    if args.train_at == "random" and config.pixelwise:
        raise SystemExit("--train-at random trains on label patches: it needs a patch head (no --pixelwise)")
    if args.train_at and args.windows_per_step < 1:
        raise SystemExit("--windows-per-step must be at least 1")
    if args.val_at:
        args.val_scenes = args.val_scenes or 2
        args.val_every = args.val_every or args.steps
    if args.val_saliency_scene and args.val_scenes < 1:
        raise SystemExit("--val-saliency-scene attributes the validation scenes: it needs --val-scenes")
    check_val_knn(args)
    check_val_probe(args)
    check_val_cluster(args)
    check_val_gmm(args)
    check_val_pca(args)
    check_val_gauss(args)
    check_val_crf(args)
    check_val_superpixel(args)
    check_val_sieve(args)
    if not 0.0 <= args.label_smoothing < 1.0:
        raise SystemExit("--label-smoothing must lie in [0, 1)")
    # --class-weights inverse: the weights come from the first step's labels, so the criterion is made there
    criterion = make_criterion(args.loss, config.ignored_label, None, args.label_smoothing) if args.class_weights == "none" else None
    fused = args.loss == "fused"
    gen = torch.Generator().manual_seed(SEED)
    val = None
    if args.val_scenes > 0 and args.val_every > 0:
        # held-out scenes from a generator of their own: the training draws (and the default output) stay as they are
        vgen = torch.Generator().manual_seed(SEED + 1)
        vimg = torch.randn(args.val_scenes, config.n_bands, 64, 64, generator=vgen)
        if config.dataset == "houston2018":
            vimg[:, 48:] = 0.0
        vlab = torch.randint(-1, config.n_classes, (args.val_scenes, 64, 64), generator=vgen)
        val = (vimg.to(device), vlab.to(device))
    # samples of a step: the tiles, or under shifting_window the windows they are cut into (train_step's condition)
    s = config.image_size - config.patch_sub
    per_step = config.batch_size * ((64 // s) ** 2 if config.shifting_window and config.image_size != 64 else 1)
    if args.train_at:
        per_step = args.windows_per_step
    model.train()
    t0 = time.time()
    for step in range(1, args.steps + 1):
        img = torch.randn(config.batch_size, config.n_bands, 64, 64, generator=gen)
        if config.dataset == "houston2018":
            img[:, 48:] = 0.0   # 48 real bands zero padded to 50 (reference src/data_houston2018.py:268-269)
        label = torch.randint(-1, config.n_classes, (config.batch_size, 64, 64), generator=gen)
        if criterion is None:
            weight = inverse_frequency_weights(label, config.n_classes, config.ignored_label)
            print("class weights " + " ".join(f"{v:.4f}" for v in weight.tolist()), flush=True)
            criterion = make_criterion(args.loss, config.ignored_label, weight, args.label_smoothing).to(device)
        # --accumulate K: K micro-steps over K slices of the step's tiles (--train-at: K draws of windows_per_step // K windows from
        # all of them); the optimizer steps inside the last one, and the step's log line is the last micro-step's
        for k in range(args.accumulate):
            if args.train_at:
                loss, acc, macro_acc = train_step_at_listed(img.to(device), label, model, config, criterion, optimizer, args.train_at,
                                                            micro_windows, gen, accumulator=accumulator, augment=args.augment)
            else:
                loss, acc, macro_acc = train_step(img[k * micro:(k + 1) * micro], label[k * micro:(k + 1) * micro], model, config, device,
                                                  criterion, optimizer, accumulator=accumulator)
        if step % config.logging_freq == 0:
            macro = f" macro_acc {float(macro_acc):.3f}" if fused else ""   # (the eager path has no macro accuracy: it repeats acc)
            print(f"step {step} loss {loss.item():.4f} acc {float(acc):.3f}{macro} {step * per_step / (time.time() - t0):.1f} samples/s",
                  flush=True)
        if val is not None and step % args.val_every == 0:
            if args.val_at:
                validate_at(model, val, step, config.ignored_label, report=args.val_report, tta=args.val_tta)
            else:
                validate(model, val, step, config.ignored_label, fused=fused, report=args.val_report)
            if args.val_embed:
                validate_embedding(model, val, step, config.n_classes, config.ignored_label)
            if args.val_knn:
                validate_knn(model, val, step, args.val_knn, config.n_classes, config.ignored_label)
            if args.val_probe:
                validate_probe(model, val, step, args.val_probe, config.n_classes, config.ignored_label)
            if args.val_cluster:
                validate_cluster(model, val, step, args.val_cluster, config.n_classes, config.ignored_label)
            if args.val_gmm:
                validate_gmm(model, val, step, args.val_gmm, args.val_gmm_cov, config.n_classes, config.ignored_label)
            if args.val_pca:
                validate_pca(model, val, step, args.val_pca)
            if args.val_gauss:
                validate_gauss(model, val, step, args.val_gauss, config.n_classes, config.ignored_label)
            if args.val_crf:
                validate_crf(model, val, step, args.val_crf, args.val_crf_radius, config.ignored_label)
            if args.val_superpixel:
                validate_superpixel(model, val, step, args.val_superpixel, args.val_superpixel_compactness, config.ignored_label,
                                    connect=args.val_superpixel_connect)
            if args.val_sieve:
                validate_sieve(model, val, step, args.val_sieve, args.val_sieve_connectivity, config.ignored_label)
            if args.val_saliency:
                validate_saliency(model, val, step)
            if args.val_saliency_scene:
                validate_saliency_scene(model, val, step)
            if args.val_attention:
                validate_attention(model, val, step)


def make_accumulator(model, accumulate, clip_norm, batch_size, windows_per_step, train_at):
    """--accumulate K / --clip-norm X -> (the GradAccumulator, or None without either flag: the step as it always was; tiles per
    micro-step; windows per micro-step under --train-at)"""
    if accumulate < 1:
        raise SystemExit("--accumulate must be at least 1")
    if clip_norm is not None and not clip_norm > 0.0:
        raise SystemExit("--clip-norm must be positive")
    if train_at and windows_per_step % accumulate:
        raise SystemExit(f"--windows-per-step {windows_per_step} does not split into --accumulate {accumulate} micro-steps")
    if not train_at and batch_size % accumulate:
        raise SystemExit(f"batch size {batch_size} does not split into --accumulate {accumulate} micro-steps")
    accumulator = None
    if accumulate > 1 or clip_norm is not None:
        from maskedsst_amd import GradAccumulator
        accumulator = GradAccumulator(model, steps=accumulate, max_norm=clip_norm)
    return accumulator, batch_size // accumulate, windows_per_step // accumulate


def train_step_at_listed(scene, label, model, config, criterion, optimizer, mode, n, gen, accumulator=None, augment=None):
    """--train-at: one step on n windows of the resident tiles scene [B, C, 64, 64] (on the device; label [B, 64, 64] on the host, where
    the table is drawn).  labelled: n of centre_origins' rows, drawn without replacement (all of them when there are fewer), each with
    its centre's class; random: n random_origins that hold a labelled pixel, with their label patches.  augment="d4": an orientation per
    window, drawn after the table from the same generator; the label patches are those of the oriented windows."""
    from maskedsst_amd import centre_origins, random_origins, random_orients, window_labels
    from maskedsst_amd.utils import train_step_at
    s = config.image_size - config.patch_sub
    if mode == "labelled":
        origins, labels = centre_origins(label, s, config.ignored_label)
        if origins.shape[0] == 0:
            raise SystemExit("--train-at labelled: the step's tiles hold no labelled pixel whose window fits")
        pick = torch.randperm(origins.shape[0], generator=gen)[:n]
        origins, labels = origins[pick], labels[pick]
    else:
        origins = random_origins(label.shape[0], label.shape[1], label.shape[2], s, n, generator=gen, labels=label,
                                 ignore_index=config.ignored_label)
        labels = window_labels(label, origins, s)
    if augment is None:
        return train_step_at(scene, labels, origins, model, config, criterion, optimizer, accumulator=accumulator)
    orient = random_orients(origins.shape[0], generator=gen)
    if mode != "labelled":
        labels = window_labels(label, origins, s, orient)
    elif s % 2 == 0:   # an even window's centre index is no fixed point of the orientations: the label under the oriented centre
        labels = window_labels(label, origins, s, orient)[:, s // 2, s // 2]
    return train_step_at(scene, labels, origins, model, config, criterion, optimizer, accumulator=accumulator, orient=orient)


def validate_at(model, val, step, ignored_label, report=False, tta=False):
    """--val-at: the Houston test protocol -- predictions only where a label exists.  One predict_at pass over the windows centred at
    the validation tiles' labelled pixels (a patch head: the logits at the window's centre), then loss, accuracies and with report
    the confusion-matrix line from one pass of the fused loss over those logits."""
    from maskedsst_amd import centre_origins
    from maskedsst_amd.ops import confusion_report, cross_entropy_stats
    img, label = val
    w = model.num_spatial_patches_sqrt
    origins, labels = centre_origins(label, w, ignored_label)
    _, logits = model.predict_at(img, origins, return_logits=True, tta="d4") if tta else model.predict_at(img, origins, return_logits=True)
    if logits.dim() == 4:
        logits = logits[:, :, w // 2, w // 2].contiguous()
    with torch.no_grad():
        _, stats = cross_entropy_stats(logits, labels, ignored_label, confusion=report)
    h = stats.host()
    print(f"val step {step} loss {h.loss:.4f} acc {h.acc:.3f} macro_acc {h.macro_acc:.3f} windows {origins.shape[0]}", flush=True)
    if report:
        r = confusion_report(h.confusion)
        print(f"val step {step} report OA {r.oa:.4f} AA {r.aa:.4f} kappa {r.kappa:.4f} mIoU {r.mean_iou:.4f} mF1 {r.mean_f1:.4f} "
              f"pixels {r.total}", flush=True)


def validate(model, val, step, ignored_label, fused=False, report=False):
    """validate_downstream (reference src/utils.py:477-605) over whole scenes: one predict_scene pass (windows of image_size,
    eval forward, the module's mode untouched; a pixelwise model: one window per pixel, its centre) and the scene metrics of
    maskedsst_amd.scene (pixels of class -1 are skipped).  report: a second line from the confusion matrix of scene_report (with
    the fused loss the same pass gives both lines)"""
    from maskedsst_amd.scene import scene_metrics, scene_report
    img, label = val
    classes, logits = model.predict_scene(img, return_logits=True)
    full = scene_report(logits, classes, label, ignore_index=ignored_label) if report else None
    m = full if (fused and report) else scene_metrics(logits, classes, label, ignore_index=ignored_label, fused=fused)
    print(f"val step {step} loss {m.loss:.4f} acc {m.acc:.3f} macro_acc {m.macro_acc:.3f} scenes {img.shape[0]}", flush=True)
    if report:
        r = full.report
        print(f"val step {step} report OA {r.oa:.4f} AA {r.aa:.4f} kappa {r.kappa:.4f} mIoU {r.mean_iou:.4f} mF1 {r.mean_f1:.4f} "
              f"pixels {r.total}", flush=True)


def frozen_split(model, val, ignored_label, normalize, all_covered=False):
    """The split --val-embed, --val-knn, --val-probe and --val-cluster share, from one encode_scene pass (windows of image_size, eval
    forward, the module's mode untouched): (ftr, ltr, fte, lte), the per-pixel 96-vectors and labels of the labelled covered pixels
    of the first half of the scenes (the bank or train rows) and of the second half (the test rows).  all_covered: the first half
    keeps ALL covered pixels, labelled or not.  A half without such a pixel (fewer than two scenes) comes back empty."""
    img, label = val
    emb = model.encode_scene(img, normalize=normalize)
    f = emb.features.permute(0, 2, 3, 1)                      # [Bs, Hs, Ws, 96]
    covered = emb.cover > 0
    ok = covered & (label != ignored_label)
    half = img.shape[0] // 2
    tr = (covered if all_covered else ok)[:half]
    return f[:half][tr], label[:half][tr], f[half:][ok[half:]], label[half:][ok[half:]]


def validate_embedding(model, val, step, n_classes, ignored_label):
    """--val-embed: how separable the classes are in the encoder's own representation, without the head.  One encode_scene pass
    (windows of image_size, eval forward, the module's mode untouched, unit-length 96-vectors per pixel); the class means of the
    labelled covered pixels of the first half of the scenes classify those of the second half by the nearest mean (plain torch on
    the returned map).  nan when either half has no such pixel (fewer than two scenes)."""
    ftr, ltr, fte, lte = frozen_split(model, val, ignored_label, True)
    acc, present = float("nan"), 0
    if len(ltr) and len(lte):
        sums = torch.zeros(n_classes, ftr.shape[-1], device=ftr.device).index_add_(0, ltr, ftr)
        count = torch.bincount(ltr, minlength=n_classes)
        means = sums / count.clamp(min=1).unsqueeze(1)
        dist = torch.cdist(fte, means)
        dist[:, count == 0] = float("inf")                   # a class the first half never shows cannot be predicted
        acc = float((dist.argmin(dim=1) == lte).double().mean())
        present = int((count > 0).sum())
    print(f"val-embed step {step} ncm_acc {acc:.3f} classes {present} train_pixels {len(ltr)} test_pixels {len(lte)} "
          f"scenes {val[0].shape[0]}", flush=True)


def check_val_knn(args):
    if not args.val_knn:
        return
    if not 1 <= args.val_knn <= 64:
        raise SystemExit("--val-knn K must lie in [1, 64]")
    if args.val_scenes < 1 or args.val_every < 1:
        raise SystemExit("--val-knn scores the validation scenes: it needs --val-scenes and --val-every")


def validate_knn(model, val, step, k, n_classes, ignored_label, temperature=0.07):
    """--val-knn K: the weighted K-nearest-neighbour accuracy of the frozen features (Wu et al. 2018), the split of --val-embed: the
    labelled covered pixels of the first half of the scenes are the bank (maskedsst_amd.KnnBank), those of the second half the
    queries; two HIP launches (msst_knn_topk, msst_knn_vote), no score matrix.  nan when either half has no such pixel."""
    from maskedsst_amd import KnnBank, knn_classify
    ftr, ltr, fte, lte = frozen_split(model, val, ignored_label, True)
    acc = float("nan")
    if len(ltr) and len(lte):
        res = knn_classify(KnnBank(ftr.contiguous(), ltr, n_classes), fte.contiguous(), k=k, temperature=temperature)
        acc = float((res.classes == lte).double().mean())
    print(f"val-knn step {step} k {k} knn_acc {acc:.3f} bank_pixels {len(ltr)} test_pixels {len(lte)} scenes {val[0].shape[0]}", flush=True)


def check_val_probe(args):
    if not args.val_probe:
        return
    if args.val_probe < 1:
        raise SystemExit("--val-probe STEPS must be at least 1")
    if args.val_scenes < 1 or args.val_every < 1:
        raise SystemExit("--val-probe scores the validation scenes: it needs --val-scenes and --val-every")


def validate_probe(model, val, step, steps, n_classes, ignored_label, lr=1e-2):
    """--val-probe STEPS: the linear-probe accuracy of the frozen features, the split of --val-embed on the RAW features
    (encode_scene(normalize=False): what mlp_head of the patch-head model consumes): a fresh LayerNorm -> Linear is trained on the
    labelled covered pixels of the first half of the scenes for STEPS full-batch Adam steps (maskedsst_amd.fit_linear_probe: two HIP
    launches per step on the cached rows, the body never runs again) and scored on those of the second half.  The model's own head
    is not touched.  nan when either half has no such pixel."""
    from maskedsst_amd import KnnBank, fit_linear_probe
    ftr, ltr, fte, lte = frozen_split(model, val, ignored_label, False)
    acc = float("nan")
    if len(ltr) and len(lte):
        probe = fit_linear_probe(KnnBank(ftr.contiguous(), ltr, n_classes), steps=steps, lr=lr)
        acc = float((probe.classify(fte.contiguous()) == lte).double().mean())
    print(f"val-probe step {step} steps {steps} probe_acc {acc:.3f} bank_pixels {len(ltr)} test_pixels {len(lte)} scenes {val[0].shape[0]}",
          flush=True)


def check_val_cluster(args):
    if not args.val_cluster:
        return
    if not 1 <= args.val_cluster <= 128:
        raise SystemExit("--val-cluster K must lie in [1, 128]")
    if args.val_scenes < 1 or args.val_every < 1:
        raise SystemExit("--val-cluster scores the validation scenes: it needs --val-scenes and --val-every")


def validate_cluster(model, val, step, k, n_classes, ignored_label, iters=50):
    """--val-cluster K: the clustering score of the frozen features, the split of --val-embed: k-means (maskedsst_amd.fit_kmeans: two
    HIP launches per iteration, cosine, k-means++ with seed 0) is fitted on ALL covered pixels of the first half of the scenes --
    no label is read -- and the labelled covered pixels of the second half are assigned and matched to the classes
    (maskedsst_amd.match_clusters: Hungarian accuracy, purity, NMI).  nan when a half has no such pixel or fewer than K."""
    from maskedsst_amd import contingency, fit_kmeans, match_clusters
    ftr, _, fte, lte = frozen_split(model, val, ignored_label, True, all_covered=True)
    acc = purity = nmi = inertia = float("nan")
    if len(ftr) >= k and len(lte):
        km = fit_kmeans(ftr.contiguous(), k=k, iters=iters, metric="cosine", init="kmeans++", seed=0, check_every=10)
        m = match_clusters(contingency(km.assign(fte.contiguous())[0], lte, k, n_classes, ignored_label))
        acc, purity, nmi, inertia = m.accuracy, m.purity, m.nmi, km.inertia
    print(f"val-cluster step {step} k {k} cluster_acc {acc:.3f} purity {purity:.3f} nmi {nmi:.3f} inertia {inertia:.4g} "
          f"test_pixels {len(lte)} train_pixels {len(ftr)} scenes {val[0].shape[0]}", flush=True)


def check_val_gmm(args):
    if not args.val_gmm:
        return
    if not 1 <= args.val_gmm <= 32:
        raise SystemExit("--val-gmm K must lie in [1, 32]")
    if args.val_scenes < 1 or args.val_every < 1:
        raise SystemExit("--val-gmm scores the validation scenes: it needs --val-scenes and --val-every")


def validate_gmm(model, val, step, k, covariance, n_classes, ignored_label, iters=30):
    """--val-gmm K: the clustering score of a Gaussian mixture of the RAW frozen features, the protocol of --val-cluster: EM
    (maskedsst_amd.fit_mixture: k-means init with seed 0, three HIP launches per iteration) is fitted on ALL covered pixels of the
    first half of the scenes -- no label is read -- and the labelled covered pixels of the second half are assigned to their most
    probable component and matched to the classes (maskedsst_amd.match_clusters).  mean_ll: the mean log-likelihood of those pixels;
    starved: the components the last iteration left without rows.  nan when a half has no such pixel or fewer than K."""
    from maskedsst_amd import contingency, fit_mixture, match_clusters
    ftr, _, fte, lte = frozen_split(model, val, ignored_label, False, all_covered=True)
    acc = purity = nmi = mean_ll = float("nan")
    starved = 0
    if len(ftr) >= k and len(lte):
        gm = fit_mixture(ftr.contiguous(), k=k, covariance=covariance, iters=iters, seed=0, check_every=5)
        res = gm.predict(fte.contiguous())
        m = match_clusters(contingency(res.classes, lte, k, n_classes, ignored_label))
        acc, purity, nmi, mean_ll, starved = m.accuracy, m.purity, m.nmi, float(res.log_likelihood.double().mean()), int(gm.history[-1, 2])
    print(f"val-gmm step {step} k {k} cov {covariance} cluster_acc {acc:.3f} purity {purity:.3f} nmi {nmi:.3f} mean_ll {mean_ll:.4g} "
          f"starved {starved} test_pixels {len(lte)} train_pixels {len(ftr)} scenes {val[0].shape[0]}", flush=True)


def check_val_pca(args):
    if not args.val_pca:
        return
    if not 1 <= args.val_pca <= 96:
        raise SystemExit("--val-pca R must lie in [1, 96]")
    if args.val_scenes < 1 or args.val_every < 1:
        raise SystemExit("--val-pca reads the validation scenes: it needs --val-scenes and --val-every")


def validate_pca(model, val, step, r):
    """--val-pca R: the label-free health check of the frozen features.  One encode_scene pass (raw features, eval forward, the
    module's mode untouched); maskedsst_amd.fit_pca reads the map of the first half of the scenes in place (uncovered pixels skipped,
    no label read): the R leading explained-variance ratios and the effective rank (exp of the entropy of the normalised eigenvalues:
    1 for a collapsed encoder, 96 for an isotropic one).  The second half is scored under that fit by the RX detector
    (FeaturePCA.mahalanobis on its map): the mean and the largest score over its covered pixels.  nan with fewer than two scenes or
    fewer than two covered pixels in the first half."""
    from maskedsst_amd import fit_pca
    emb = model.encode_scene(val[0], normalize=False)
    half = val[0].shape[0] // 2
    rows, evr, erank, rx_mean, rx_max = 0, [float("nan")] * r, float("nan"), float("nan"), float("nan")
    if half >= 1 and int((emb.cover[:half] > 0).sum()) >= 2:
        pca = fit_pca(emb.features[:half].contiguous())
        rows, evr, erank = pca.count, pca.explained_variance_ratio[:r].tolist(), pca.effective_rank
        if pca.rank >= 1:
            score = pca.mahalanobis(emb.features[half:].contiguous())
            score = score[emb.cover[half:] > 0]
            if len(score):
                rx_mean, rx_max = float(score.double().mean()), float(score.max())
    print(f"val-pca step {step} rows {rows} evr {' '.join(f'{v:.4f}' for v in evr)} effective_rank {erank:.3f} rx_mean {rx_mean:.4g} "
          f"rx_max {rx_max:.4g} scenes {val[0].shape[0]}", flush=True)


def check_val_gauss(args):
    if not args.val_gauss:
        return
    if args.val_gauss not in ("full", "tied"):
        raise SystemExit("--val-gauss must be full or tied")
    if args.val_scenes < 1 or args.val_every < 1:
        raise SystemExit("--val-gauss scores the validation scenes: it needs --val-scenes and --val-every")


def validate_gauss(model, val, step, covariance, n_classes, ignored_label):
    """--val-gauss {full,tied}: maximum-likelihood classification of the frozen features, the split of --val-knn on the RAW features:
    class-conditional Gaussians (maskedsst_amd.fit_gaussian: the moments kernels on every class's rows, the eigendecompositions on
    the host) are fitted on the labelled covered pixels of the first half of the scenes and those of the second half are scored in
    one HIP launch (msst_gauss_score).  gauss_acc: the accuracy; mean_d2: the mean squared Mahalanobis distance to the predicted
    class; rejected: the share of test pixels farther from their predicted class than 99 % of the bank's pixels are from their own
    (clf.threshold(bank, 0.99): the open-set rule).  nan when either half has no such pixel or a class has too few rows for its
    covariance."""
    from maskedsst_amd import KnnBank, fit_gaussian
    ftr, ltr, fte, lte = frozen_split(model, val, ignored_label, False)
    acc = mean_d2 = rejected = float("nan")
    if len(ltr) and len(lte):
        bank = KnnBank(ftr.contiguous(), ltr, n_classes)
        try:
            clf = fit_gaussian(bank, covariance=covariance)
        except ValueError as e:
            print(f"val-gauss not fitted at step {step}: {e}", flush=True)
            clf = None
        if clf is not None:
            res = clf.classify(fte.contiguous(), scores=False)
            limit = clf.threshold(bank, 0.99)
            acc = float((res.classes == lte).double().mean())
            mean_d2 = float(res.distance.double().mean())
            rejected = float((res.distance > limit).double().mean())
    print(f"val-gauss step {step} cov {covariance} gauss_acc {acc:.3f} mean_d2 {mean_d2:.4g} rejected {rejected:.3f} bank_pixels {len(ltr)} "
          f"test_pixels {len(lte)} scenes {val[0].shape[0]}", flush=True)


def check_val_crf(args):
    if not args.val_crf:
        return
    if args.val_crf < 1:
        raise SystemExit("--val-crf ITERS must be at least 1")
    if not 1 <= args.val_crf_radius <= 3:
        raise SystemExit("--val-crf-radius R must lie in [1, 3]")
    if args.val_scenes < 1 or args.val_every < 1:
        raise SystemExit("--val-crf refines the validation scenes: it needs --val-scenes and --val-every")


def validate_crf(model, val, step, iters, radius, ignored_label):
    """--val-crf ITERS: the spectral-spatial last stage on the validation scenes.  predict_scene(return_logits=True) gives the logit
    map, one encode_scene(normalize=True) pass the feature map; maskedsst_amd.crf_affinity (one HIP launch, radius --val-crf-radius,
    the API defaults otherwise) and crf_refine (ITERS + 1 launches of msst_crf_step) refine it.  acc_before: the accuracy of the
    argmax of softmax(logits) (step 0) on the labelled live pixels; acc_after: that of the refined map; changed: the pixels whose
    class differs between the two.  nan when no labelled pixel is live."""
    from maskedsst_amd import crf_affinity, crf_refine
    img, lab = val
    _, logits = model.predict_scene(img, return_logits=True)
    aff = crf_affinity(model.encode_scene(img, normalize=True), radius=radius)
    before = crf_refine(logits, aff, iters=0).classes
    after = crf_refine(logits, aff, iters=iters).classes
    ok = (lab != ignored_label) & (after >= 0)
    acc0 = acc1 = float("nan")
    if bool(ok.any()):
        acc0, acc1 = float((before[ok] == lab[ok]).double().mean()), float((after[ok] == lab[ok]).double().mean())
    print(f"val-crf step {step} iters {iters} radius {radius} acc_before {acc0:.3f} acc_after {acc1:.3f} changed {int((before != after).sum())} "
          f"pixels {int(ok.sum())} scenes {img.shape[0]}", flush=True)


def check_val_superpixel(args):
    if args.val_superpixel_connect and not args.val_superpixel:
        raise SystemExit("--val-superpixel-connect connects the superpixels of --val-superpixel STEP: it needs that flag")
    if not args.val_superpixel:
        return
    if args.val_superpixel not in (4, 8, 16):
        raise SystemExit("--val-superpixel STEP must be 4, 8 or 16")
    c = args.val_superpixel_compactness
    if not (c >= 0.0 and c < float("inf")):
        raise SystemExit("--val-superpixel-compactness M must be a finite number >= 0")
    if args.val_scenes < 1 or args.val_every < 1:
        raise SystemExit("--val-superpixel segments the validation scenes: it needs --val-scenes and --val-every")


def validate_superpixel(model, val, step, sp_step, compactness, ignored_label, connect=False):
    """--val-superpixel STEP: object-based classification of the validation scenes.  predict_scene(return_logits=True) gives the
    logit map, one encode_scene(normalize=True) pass the feature map; maskedsst_amd.fit_superpixels (grid step STEP, compactness
    --val-superpixel-compactness, the API default of 10 iterations) segments it and superpixel_classify pools the logits per
    superpixel and gives every pixel its superpixel's class.  acc_before: the accuracy of predict_scene's class map on the labelled
    live pixels; acc_after: that of the object-based map; changed: the live pixels whose class differs between the two; superpixels:
    those with at least one pixel.  nan when no labelled pixel is live.
    connect (--val-superpixel-connect): one more line, after maskedsst_amd.enforce_connectivity at its defaults on the same
    superpixels: fragments_before / fragments_after: the pieces beyond one per superpixel; acc_after: the accuracy of the object-based
    map on the connected superpixels."""
    from maskedsst_amd import enforce_connectivity, fit_superpixels, superpixel_classify
    img, lab = val
    before, logits = model.predict_scene(img, return_logits=True)
    sp = fit_superpixels(model.encode_scene(img, normalize=True), step=sp_step, compactness=compactness)
    after = superpixel_classify(sp, logits).classes
    live = after >= 0
    ok = (lab != ignored_label) & live
    acc0 = acc1 = float("nan")
    if bool(ok.any()):
        acc0, acc1 = float((before[ok] == lab[ok]).double().mean()), float((after[ok] == lab[ok]).double().mean())
    print(f"val-superpixel step {step} sp_step {sp_step} superpixels {int((sp.counts > 0).sum())} acc_before {acc0:.3f} acc_after {acc1:.3f} "
          f"changed {int(((before != after) & live).sum())} pixels {int(ok.sum())} scenes {img.shape[0]}", flush=True)
    if not connect:
        return
    con = enforce_connectivity(sp)
    joined = superpixel_classify(con.superpixels, logits).classes
    frag0 = int(con.history[0, 1]) if len(con.history) else 0
    frag1 = int(con.regions.count.sum()) - int((con.superpixels.counts > 0).sum())
    acc2 = float((joined[ok] == lab[ok]).double().mean()) if bool(ok.any()) else float("nan")
    print(f"val-superpixel-connected step {step} fragments_before {frag0} fragments_after {frag1} acc_after {acc2:.3f} "
          f"pixels {int(ok.sum())} scenes {img.shape[0]}", flush=True)


def check_val_sieve(args):
    if not args.val_sieve:
        return
    if args.val_sieve < 1:
        raise SystemExit("--val-sieve MIN_SIZE must be at least 1")
    if args.val_scenes < 1 or args.val_every < 1:
        raise SystemExit("--val-sieve sieves the validation scenes' class maps: it needs --val-scenes and --val-every")


def validate_sieve(model, val, step, min_size, connectivity, ignored_label):
    """--val-sieve MIN_SIZE: the minimum mapping unit on the validation scenes.  predict_scene gives the class maps;
    maskedsst_amd.sieve_classes (connectivity --val-sieve-connectivity, the API default of 4 rounds) merges every connected patch of
    fewer than MIN_SIZE pixels into its largest neighbour.  regions_before / regions_after: the connected regions of the maps;
    acc_before / acc_after: the accuracy on the labelled live pixels; changed: the pixels whose class differs.  nan when no labelled
    pixel is live."""
    from maskedsst_amd import sieve_classes
    img, lab = val
    before = model.predict_scene(img).contiguous()
    res = sieve_classes(before, min_size, connectivity=connectivity)
    after = res.classes
    ok = (lab != ignored_label) & (after >= 0)
    acc0 = acc1 = float("nan")
    if bool(ok.any()):
        acc0, acc1 = float((before[ok] == lab[ok]).double().mean()), float((after[ok] == lab[ok]).double().mean())
    print(f"val-sieve step {step} min_size {min_size} regions_before {int(res.history[0, 0])} regions_after {int(res.regions.count.sum())} "
          f"acc_before {acc0:.3f} acc_after {acc1:.3f} changed {int((before != after).sum())} pixels {int(ok.sum())} scenes {img.shape[0]}",
          flush=True)


def validate_saliency(model, val, step, batch=256, top=5):
    """--val-saliency: which bands drive the decisions.  The validation scenes are cut into their non-overlapping image_size
    windows (a torch reshape); band_importance (gradient x input of the argmax class's logit, through the HIP backward down to
    the input) runs on them in eval mode, `batch` windows at a time, and the bands are ranked by the mean |attribution| over all
    windows.  The module's mode is put back as found."""
    from maskedsst_amd import band_importance
    img, _ = val
    s = model.num_spatial_patches_sqrt
    V, C, H, W = img.shape
    nr, nq = H // s, W // s
    win = img[:, :, :nr * s, :nq * s].reshape(V, C, nr, s, nq, s).permute(0, 2, 4, 1, 3, 5).reshape(V * nr * nq, C, s, s).contiguous()
    was_training = model.training
    model.eval()
    try:
        total = torch.zeros(C, dtype=torch.float64, device=img.device)
        for i in range(0, win.shape[0], batch):
            total += band_importance(model, win[i:i + batch]).abs().sum(dim=0).double()
    finally:
        model.train(was_training)
    mean = (total / win.shape[0]).cpu()
    order = torch.argsort(mean, descending=True)[:top].tolist()
    print(f"val-saliency step {step} top bands " + " ".join(f"{b}:{float(mean[b]):.3e}" for b in order) + f" windows {win.shape[0]}",
          flush=True)


def validate_saliency_scene(model, val, step, top=5):
    """--val-saliency-scene: which bands drive the class maps of the whole validation scenes.  band_importance_scene (gradient x input of
    predict_scene's logit map at its own classes, the windows read in place and their input gradients folded into the scenes by
    msst_scene_fold_at) at predict_scene's default stride; the bands are ranked by the mean |attribution| over the scenes.  Eval forward,
    the module's mode and its parameters' flags and gradients left as found."""
    from maskedsst_amd import band_importance_scene
    img, _ = val
    mean = band_importance_scene(model, img).abs().double().mean(dim=0).cpu()
    order = torch.argsort(mean, descending=True)[:top].tolist()
    print(f"val-saliency-scene step {step} top bands " + " ".join(f"{b}:{float(mean[b]):.3e}" for b in order) + f" scenes {img.shape[0]}",
          flush=True)


def validate_attention(model, val, step, batch=256, top=3):
    """--val-attention: which spectral blocks the spectral stack looks at.  The first `batch` non-overlapping image_size windows of
    the validation scenes go through model.attention_maps(stack="spectral") (eval forward, the module's mode untouched; the maps come
    out of msst_attn_maps averaged over a window's positions); attention_rollout multiplies the blocks' head-averaged maps, and a
    spectral block's score is the mean over windows and queries of its column."""
    from maskedsst_amd import attention_rollout
    img, _ = val
    s = model.num_spatial_patches_sqrt
    V, C, H, W = img.shape
    nr, nq = H // s, W // s
    win = img[:, :, :nr * s, :nq * s].reshape(V, C, nr, s, nq, s).permute(0, 2, 4, 1, 3, 5).reshape(V * nr * nq, C, s, s)[:batch].contiguous()
    roll = attention_rollout(model.attention_maps(win, stack="spectral").spectral)    # [B, S, S] float64
    received = roll.mean(dim=(0, 1)).cpu()
    order = torch.argsort(received, descending=True)[:top].tolist()
    print(f"val-attention step {step} top spectral blocks " + " ".join(f"{b}:{float(received[b]):.4f}" for b in order)
          + f" windows {win.shape[0]}", flush=True)


if __name__ == "__main__":
    main()
