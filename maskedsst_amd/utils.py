"""Host-side helpers mirroring the parts of reference ``src/utils.py`` that touch the model:
optimizer construction (``:36-59``), checkpoint hand-off pretrain -> finetune (``:276-313``), the
finetune training step (``:608-663``) and the Houston spectral-position lookup (``:415-429``)."""
import numpy as np
import torch


def get_optimizers(model, config, fused=True):
    """reference src/utils.py:36-59 (Adam / AdamW + ReduceLROnPlateau / cosine).  ``fused=True`` swaps
    AdamW for the one-launch FusedAdamW (same update rule)."""
    if config.optimizer == "Adam":
        optimizer = torch.optim.Adam(model.parameters(), lr=config.lr, weight_decay=config.weight_decay)
    elif config.optimizer == "AdamW":
        if fused:
            from .optim import FusedAdamW
            optimizer = FusedAdamW(model, lr=config.lr, weight_decay=config.weight_decay)
        else:
            optimizer = torch.optim.AdamW(model.parameters(), lr=config.lr, weight_decay=config.weight_decay)
    else:
        raise ValueError(f"unknown optimizer {config.optimizer}")
    if config.scheduler == "ReduceLROnPlateau":
        scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, factor=0.9, patience=5)
    elif config.scheduler == "cosine":
        scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=50, eta_min=0, last_epoch=-1)
    else:
        raise ValueError(f"unknown scheduler {config.scheduler}")
    return optimizer, scheduler


def get_pos_for_spectral_embedding(spectral_patch_depth, wavelengths, reference_wavelengths):
    """For every spectral block (``spectral_patch_depth`` consecutive bands, last block ragged) of a sensor with band
    centres ``wavelengths``: the index of the block of ``reference_wavelengths`` whose mean wavelength is closest
    (reference src/vit_spatial_spectral.py:767-800).  Used to address the spectral position table of a model pre-trained
    on the reference sensor with another sensor's bands (Houston2018 on an EnMAP model: [0, 3, 5, 7, 9])."""
    def block_means(w):
        w = np.asarray(w, dtype=np.float64)
        edges = np.arange(0, len(w), spectral_patch_depth)
        return np.add.reduceat(w, edges) / np.diff(np.append(edges, len(w)))
    bm, rm = block_means(wavelengths), block_means(reference_wavelengths)
    return [int(i) for i in np.abs(rm[None, :] - bm[:, None]).argmin(axis=1)]


def get_spectral_pos_embedding(dataset, n_bands, band_patch_size, wavelengths=None, reference_wavelengths=None):
    """reference src/utils.py:415-429: positions of a dataset's spectral tokens in the pre-training sensor's spectral
    sequence -- the identity for the EnMAP-derived label sets (worldcover / dfc), the nearest-block lookup for
    Houston2018 (its band-centre table and the reference sensor's are data the caller supplies; the readers that carry
    them are out of scope here).  Any other name raises, as in the reference (dataset: enmap is a pre-training set and
    has no finetune labels there either)."""
    if dataset in ("worldcover", "dfc"):
        return torch.arange(n_bands // band_patch_size)
    if dataset == "houston2018":
        if wavelengths is None or reference_wavelengths is None:
            raise ValueError("houston2018 needs the band-centre tables of both sensors")
        return get_pos_for_spectral_embedding(band_patch_size, wavelengths, reference_wavelengths)
    raise NotImplementedError(f"Unknown dataset {dataset=}")


def load_checkpoint(config, model, classifier_name="mlp_head", device="cpu", checkpoint=None):
    """Initialise a bare encoder from a SimMIM pre-training checkpoint, with the reference's semantics
    (src/utils.py:276-313): keys ``encoder.X`` are renamed to ``X``; every other key (``mask_token``,
    ``to_pixels.*``) is dropped; the checkpoint's classifier Linear is replaced by the freshly initialised
    one of ``model`` (its output shape differs); then a STRICT ``load_state_dict``.
    ``checkpoint`` may be an already loaded dict (else ``config.checkpoint_path`` is read)."""
    if checkpoint is None:
        checkpoint = torch.load(config.checkpoint_path, map_location=device, weights_only=False)
    src = checkpoint["model_state_dict"]
    weights = {k[len("encoder."):]: v for k, v in src.items() if k.startswith("encoder.")}
    linear_idx = 2 if getattr(model, "pixelwise", False) else 1
    head = getattr(model, classifier_name)[linear_idx]
    patch_sub = getattr(config, "patch_sub", 0)
    if patch_sub != 0 and weights.get("pos_embed") is not None:
        assert model.pos_embed.shape[1] == (config.image_size - patch_sub) ** 2
        weights["pos_embed"] = weights["pos_embed"][:, : model.pos_embed.shape[1], :]
    weights.pop(f"{classifier_name}.1.bias", None)
    weights.pop(f"{classifier_name}.1.weight", None)
    weights[f"{classifier_name}.{linear_idx}.bias"] = head.bias.detach().clone()
    weights[f"{classifier_name}.{linear_idx}.weight"] = head.weight.detach().clone()
    print(model.load_state_dict(weights))
    return model


def stack_image_batch(config, img, label):
    """reference src/utils.py:451-474: cut img [B, C, H, W] and label [B, H, W] into their non-overlapping s x s windows,
    s = image_size - patch_sub, stacked along the batch axis in (tile, window row, window column) order -- the numbering of
    maskedsst_amd.scene.scene_windows(H, W, s, s) per tile; the trailing H % s rows and W % s columns are dropped (the reference
    asserts that both remainders are equal).  Plain torch: train_step stacks the labels with its label half (stack_windows), the images stay where they are
    (ViTSpatialSpectral.forward_windows reads the windows out of the tiles)."""
    s = config.image_size - getattr(config, "patch_sub", 0)
    cutoff_h, cutoff_w = img.shape[2] % s, img.shape[3] % s
    assert cutoff_h == cutoff_w
    return stack_windows(img, s), stack_windows(label, s)


def stack_windows(t, s):
    """one tensor's half of stack_image_batch: t [B, C, H, W] -> [B nr nq, C, s, s], or a label map [B, H, W] -> [B nr nq, s, s]"""
    nr, nq = t.shape[-2] // s, t.shape[-1] // s
    lead = t.shape[:-2]   # (B, C) or (B,)
    t = t[..., :nr * s, :nq * s].reshape(*lead, nr, s, nq, s)
    if len(lead) == 2:
        return t.permute(0, 2, 4, 1, 3, 5).reshape(lead[0] * nr * nq, lead[1], s, s)
    return t.permute(0, 1, 3, 2, 4).reshape(lead[0] * nr * nq, s, s)


def train_step(img, label, model, config, device, criterion, optimizer, acc_criterion=None, accumulator=None):
    """reference src/utils.py:608-663 for the ViTSpatialSpectral method: optional random crop, forward,
    CE(ignore_index) loss, pixel accuracy on valid labels, backward, optimizer step.  With ``config.pixelwise`` a label
    map [B, s, s] is reduced to its centre pixel ``label[:, c, c]``, ``c = (image_size - patch_sub) // 2`` (reference
    :630-636); a label that is already one class per sample ([B]) passes through unchanged.
    ``criterion`` a ``maskedsst_amd.ops.FusedCrossEntropy``: loss, gradient and counts come from one pass of the HIP loss kernels,
    ``macro_acc`` is the true macro accuracy (mean per-class recall) and the step reads the device back once (``_fused_tail``).  Any
    other criterion: the eager path below, unchanged.
    ``config.shifting_window`` (reference :608-613) on 64 x 64 tiles: no crop -- the step trains on every non-overlapping window of
    the tiles at once (``stack_image_batch`` order; 64 windows of 8 x 8 per tile, 81 of 7 x 7 for a pixelwise model), the labels are
    stacked, the images are not: ``model.forward_windows`` reads the windows out of the tiles on the device.
    ``accumulator`` (a ``maskedsst_amd.optim.GradAccumulator``; default None: the step as it always was): this call is one micro-step
    -- its gradients join the accumulator's sum and the optimizer steps, on the mean of the micro-steps' gradients (each the mean over
    its own valid labels), only when the accumulator's cycle is complete."""
    patch_sub = getattr(config, "patch_sub", 0)
    windows = bool(getattr(config, "shifting_window", False)) and config.image_size != 64 and img.shape[-1] == 64
    if windows:
        assert img.shape[2] % (config.image_size - patch_sub) == img.shape[3] % (config.image_size - patch_sub)   # stack_image_batch's
        label = stack_windows(label, config.image_size - patch_sub)   # the labels alone: the tiles go to the device as they are
    elif config.image_size != 64 and img.shape[-1] == 64:
        x, y = torch.randint(0, 64 - config.image_size - patch_sub, size=(2,))
        s = config.image_size - patch_sub
        img = img[:, :, x:x + s, y:y + s]
        label = label[:, x:x + s, y:y + s]
    if getattr(config, "pixelwise", False) and label.dim() == 3:
        c = (config.image_size - patch_sub) // 2
        label = label[:, c, c]
    img = img.to(device)
    label = label.to(device)
    optimizer.zero_grad()
    output = model.forward_windows(img) if windows else model(img)
    if getattr(criterion, "fused_stats", False):
        return _fused_tail(output, label, criterion, optimizer, accumulator)
    loss = criterion(output, label)
    if torch.isnan(loss):
        raise ValueError("Loss is NaN")
    pred = output.argmax(dim=1)
    valid = label != config.ignored_label
    acc = (pred[valid] == label[valid]).sum() / max(int(valid.sum()), 1)
    macro_acc = acc_criterion(pred[valid].to(int), label[valid]) if (acc_criterion is not None and valid.any()) else acc
    loss.backward()
    _optimizer_step(optimizer, accumulator)
    return loss, acc, macro_acc


def train_step_at(scene, labels, origins, model, config, criterion, optimizer, acc_criterion=None, accumulator=None, orient=None):
    """train_step on the windows of resident scenes listed in origins [n, 3] = (scene, y0, x0) (the reference's Houston2018 sampling,
    src/data_houston2018.py:303-329): train_step's body with ``model.forward_at(scene, origins)`` in place of crop, stack and
    ``model(img)`` -- no window is copied.  scene [Bs, C, Hs, Ws] is on the device already; labels and origins are moved to it.
    labels: one entry per window -- [n] for a pixelwise model (``centre_origins``' second result), [n, s, s] for the patch heads
    (``window_labels``) -- or the label maps [Bs, Hs, Ws] of the scenes, from which exactly those are gathered here (pixelwise: the
    label at the window's centre, index s // 2 of the window).  Loss, accuracy, backward and optimizer step as in train_step, the
    fused criterion and ``accumulator`` included.
    orient [n] (D4 augmentation, ``random_orients``): handed to ``forward_at``, and the labels gathered from label maps are those of the
    oriented windows (``window_labels(..., orient=)``; pixelwise: the label under the oriented window's centre, the same pixel for an
    odd window).  Labels given per window are taken as they are: in the oriented frame."""
    from .scene import window_labels
    s = config.image_size - getattr(config, "patch_sub", 0)
    if labels.dim() == 3 and tuple(labels.shape) == (scene.shape[0],) + tuple(scene.shape[-2:]):
        if getattr(config, "pixelwise", False):
            if orient is not None and s % 2 == 0:   # an even window's centre index is no fixed point of the orientations
                label = window_labels(labels, origins, s, orient)[:, s // 2, s // 2]
            else:
                o = origins.to(labels.device).long()
                label = labels[o[:, 0], o[:, 1] + s // 2, o[:, 2] + s // 2].long()
        else:
            label = window_labels(labels, origins, s) if orient is None else window_labels(labels, origins, s, orient)
    else:
        label = labels
        if getattr(config, "pixelwise", False) and label.dim() == 3:
            label = label[:, s // 2, s // 2]
    if label.shape[0] != origins.shape[0]:
        raise ValueError(f"{label.shape[0]} labels for {origins.shape[0]} windows")
    label = label.to(scene.device)
    optimizer.zero_grad()
    output = model.forward_at(scene, origins) if orient is None else model.forward_at(scene, origins, orient=orient)
    if getattr(criterion, "fused_stats", False):
        return _fused_tail(output, label, criterion, optimizer, accumulator)
    loss = criterion(output, label)
    if torch.isnan(loss):
        raise ValueError("Loss is NaN")
    pred = output.argmax(dim=1)
    valid = label != config.ignored_label
    acc = (pred[valid] == label[valid]).sum() / max(int(valid.sum()), 1)
    macro_acc = acc_criterion(pred[valid].to(int), label[valid]) if (acc_criterion is not None and valid.any()) else acc
    loss.backward()
    _optimizer_step(optimizer, accumulator)
    return loss, acc, macro_acc


def _optimizer_step(optimizer, accumulator):
    """the end of a training step: the optimizer step -- or, with a ``maskedsst_amd.optim.GradAccumulator``, one micro-step of it:
    the gradients join its sum and the optimizer steps on the (clipped) mean only after the last micro-step of the cycle"""
    if accumulator is None or accumulator.add():
        optimizer.step()


def _fused_tail(output, label, criterion, optimizer, accumulator=None):
    """train_step from the loss on, for a FusedCrossEntropy: loss + record (two launches), ONE read-back of the record, the
    reference's NaN check on it (before the backward, as there), backward (one launch up to the head's), optimizer step.
    -> (loss: 0-d device tensor, acc, macro_acc: floats; acc = 0 and macro_acc = acc when no label is valid, as on the eager path)"""
    loss, stats = criterion(output, label, return_stats=True)
    h = stats.host()
    if h.loss != h.loss:
        raise ValueError("Loss is NaN" + (f" ({h.nonfinite} non-finite rows)" if h.nonfinite else " (no valid label)" if not h.n_valid else ""))
    if h.bad_labels:
        raise ValueError(f"{h.bad_labels} labels outside [0, {stats.n_classes}) that are not the ignored label")
    loss.backward(criterion.unit_gradient(loss.device))
    _optimizer_step(optimizer, accumulator)
    acc = h.n_correct / max(h.n_valid, 1)
    return loss, acc, (h.macro_acc if h.n_valid else acc)
