"""Input attributions: which bands and pixels of a hyperspectral cube drive a model output.

Thin host code over the autograd path of the package -- the model's forward and backward run in its HIP kernels, the input
gradient comes out of ``msst_tokenize_bwd_input`` (``maskedsst_amd/csrc/msst_input_grad.hip``); nothing of the model is restated here.

    input_gradient        d(score) / d(img)
    band_importance       the attribution summed over a window's pixels, per band
    integrated_gradients  Riemann-midpoint integrated gradients with the completeness gap

The score of a classifier is the sum over samples and positions of the logit of a target class; that of a SimMIM model is its
reconstruction loss.
"""
import torch

__all__ = ["input_gradient", "band_importance", "integrated_gradients"]


def _is_simmim(model):
    from .vit_simmim_original import SimMIMSpatialSpectral
    return isinstance(model, SimMIMSpatialSpectral)


def _logits_of(model, img):
    """model(img) as [B, n_classes, *positions] (a pixelwise model's squeeze of a batch of one undone)"""
    out = model(img)
    if out.dim() == 1 and img.shape[0] == 1:
        out = out.unsqueeze(0)
    return out


def _resolve_target(logits, target):
    """target (None: the argmax class; an int; a tensor [B]; a tensor [B, *positions] with -1 = skip) -> (index [B, *positions]
    int64 with the skipped entries at 0, valid [B, *positions] in the logits' dtype)"""
    B, pos = logits.shape[0], tuple(logits.shape[2:])
    if target is None:
        idx = logits.detach().argmax(dim=1)
    elif isinstance(target, int):
        idx = torch.full((B,) + pos, target, dtype=torch.int64, device=logits.device)
    else:
        t = torch.as_tensor(target).to(device=logits.device, dtype=torch.int64)
        if tuple(t.shape) == (B,):
            idx = t.view((B,) + (1,) * len(pos)).expand((B,) + pos)
        elif tuple(t.shape) == (B,) + pos:
            idx = t
        else:
            raise ValueError(f"target must be None, an int, a tensor [{B}] or a tensor {(B,) + pos}, got {tuple(t.shape)}")
    valid = idx >= 0
    if int(idx.max()) >= logits.shape[1]:
        raise ValueError(f"target class {int(idx.max())} outside the model's {logits.shape[1]} classes")
    return idx.clamp(min=0).contiguous(), valid.to(logits.dtype)


def _class_scores(logits, idx, valid):
    """per-sample score [B]: the sum over the positions that count of the logit of the position's target class"""
    sel = logits.gather(1, idx.unsqueeze(1)).squeeze(1) * valid
    return sel.reshape(sel.shape[0], -1).sum(dim=1)


class _Frozen:
    """every parameter of the model with requires_grad off for the duration (the frozen path of the engine: no parameter gradient is
    handed out); the flags and the .grad of every parameter are put back as found"""

    def __init__(self, model):
        self.params = list(model.parameters())

    def __enter__(self):
        self.flags = [p.requires_grad for p in self.params]
        self.grads = [p.grad for p in self.params]
        for p in self.params:
            p.requires_grad_(False)

    def __exit__(self, *exc):
        for p, f, g in zip(self.params, self.flags, self.grads):
            p.requires_grad_(f)
            p.grad = g
        return False


def input_gradient(model, img, target=None, masks=None):
    """d(score) / d(img), a tensor of img's shape.

    Classifier (``ViTSpatialSpectral``): score = the sum over samples and positions of the logit of class ``target`` -- an int,
    a tensor [B] (one class per sample), a tensor [B, H, W] (one per position, -1 = skip), or None for the argmax class of every
    position.  SimMIM model: score = the reconstruction loss; ``target`` is ignored and ``masks`` (the pair ``forward`` takes) may
    be passed through, otherwise fresh masks are drawn as in ``forward``.

    The model runs in the mode it is in (call ``model.eval()`` first for a dropout-free gradient); its training mode, the
    requires_grad flags and the .grad of its parameters are left as found."""
    with _Frozen(model):
        x = img.detach().requires_grad_(True)
        with torch.enable_grad():
            if _is_simmim(model):
                score = model(x, masks)
            else:
                logits = _logits_of(model, x)
                score = _class_scores(logits, *_resolve_target(logits, target)).sum()
            (grad,) = torch.autograd.grad(score, x)
    return grad


def band_importance(model, img, target=None, mode="grad_x_input", masks=None):
    """[B, C]: the attribution of every band, summed over the window's pixels.  mode "grad_x_input": gradient x input (signed);
    "abs_grad": |gradient|.  model, target, masks: as for ``input_gradient``."""
    if mode not in ("grad_x_input", "abs_grad"):
        raise ValueError(f"unknown mode {mode!r} (use 'grad_x_input' or 'abs_grad')")
    g = input_gradient(model, img, target, masks)
    a = g * img.detach().to(g.dtype) if mode == "grad_x_input" else g.abs()
    return a.reshape(a.shape[0], a.shape[1], -1).sum(dim=2)


def integrated_gradients(model, img, target, baseline=None, steps=16, max_batch=256):
    """Riemann-midpoint integrated gradients of a classifier's score (``input_gradient``'s) along the straight path from
    ``baseline`` (default: zeros) to ``img``:  attr = (img - baseline) * mean_k grad(baseline + (k + 1/2) / steps (img - baseline)).

    The ``steps`` interpolated cubes of a sample go through the model as one batch, max(1, max_batch // steps) samples at a time.
    target: as for ``input_gradient``; None fixes the argmax classes of ``img`` for the whole path.
    Pick a baseline that is a cube (a mean spectrum, a blurred or another sample): the tokenizer's pre-norm LayerNorm makes the model
    invariant to the scale of a patch, so along the ray from the default zero cube the score is constant and all of its change sits
    at the origin -- the gap then equals the score difference.
    -> (attr of img's shape, gap [B]): gap = |sum(attr) - (score(img) - score(baseline))| per sample, the completeness error of the
    midpoint rule (O(1 / steps^2) for a smooth model)."""
    if _is_simmim(model):
        raise ValueError("integrated_gradients attributes a classifier's logits; use input_gradient for the SimMIM loss")
    if steps < 1:
        raise ValueError("steps must be at least 1")
    img = img.detach()
    base = torch.zeros_like(img) if baseline is None else torch.as_tensor(baseline).to(img).expand_as(img)
    B = img.shape[0]
    with _Frozen(model), torch.no_grad():
        logits = _logits_of(model, img)
        idx, valid = _resolve_target(logits, target)
        ends = _class_scores(logits, idx, valid) - _class_scores(_logits_of(model, base), idx, valid)
    alphas = ((torch.arange(steps, device=img.device, dtype=img.dtype) + 0.5) / steps).view(1, steps, *([1] * (img.dim() - 1)))
    per = max(1, int(max_batch) // steps)
    attr = torch.empty_like(img)
    for b0 in range(0, B, per):
        b1 = min(B, b0 + per)
        delta = img[b0:b1] - base[b0:b1]
        path = (base[b0:b1].unsqueeze(1) + alphas * delta.unsqueeze(1)).reshape((b1 - b0) * steps, *img.shape[1:])
        tgt = idx[b0:b1].repeat_interleave(steps, dim=0)
        tgt = torch.where(valid[b0:b1].repeat_interleave(steps, dim=0) > 0, tgt, torch.full_like(tgt, -1))
        g = input_gradient(model, path, tgt)
        attr[b0:b1] = delta * g.reshape(b1 - b0, steps, *img.shape[1:]).mean(dim=1).to(img.dtype)
    gap = (attr.reshape(B, -1).sum(dim=1) - ends).abs()
    return attr, gap
