"""Input attributions: which bands and pixels of a hyperspectral cube drive a model output.

Thin host code over the autograd path of the package -- the model's forward and backward run in its HIP kernels, the input
gradient comes out of ``msst_tokenize_bwd_input`` (``maskedsst_amd/csrc/msst_input_grad.hip``); nothing of the model is restated here.

    input_gradient        d(score) / d(img)
    band_importance       the attribution summed over a window's pixels, per band
    integrated_gradients  Riemann-midpoint integrated gradients with the completeness gap
    scene_saliency        d(score) / d(scene) of a whole scene's class map, through the overlapping windows read in place
    band_importance_scene the scene attribution summed over the pixels, per band

The score of a classifier is the sum over samples and positions of the logit of a target class; that of a SimMIM model is its
reconstruction loss.
"""
from collections import namedtuple

import torch

__all__ = ["input_gradient", "band_importance", "integrated_gradients", "scene_saliency", "band_importance_scene", "SceneSaliency"]

# what scene_saliency returns: grad [Bs, C, Hs, Ws] fp32, classes [Bs, Hs, Ws] int64 (-1: uncovered), cover [Bs, Hs, Ws] int32
SceneSaliency = namedtuple("SceneSaliency", ["grad", "classes", "cover"])


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


def _scene_cover(Bs, Hs, Ws, w, stride, pixelwise, device):
    """how many windows of the grid (origins 0, stride, 2 stride, ... that fit) count at a pixel -> [Bs, Hs, Ws] int32.  Patch heads: the
    windows covering it; a pixelwise model: 1 at a window's centre, 0 elsewhere -- where predict_scene's classes are not -1."""
    def axis(L):
        n = (L - w) // stride + 1
        pos = torch.arange(L, device=device)
        org = torch.arange(n, device=device) * stride
        if pixelwise:
            return (pos[:, None] == org[None, :] + w // 2).sum(dim=1)
        return ((pos[:, None] >= org[None, :]) & (pos[:, None] < org[None, :] + w)).sum(dim=1)
    return (axis(Hs)[:, None] * axis(Ws)[None, :]).to(torch.int32).expand(Bs, Hs, Ws).contiguous()


def _check_scene_target(target, Bs, Hs, Ws, nc):
    """target of scene_saliency before anything runs: None, an int in [0, nc), or an integer tensor [Bs, Hs, Ws] below nc (-1 = skip)"""
    if target is None:
        return None
    if isinstance(target, int) and not isinstance(target, bool):
        if not 0 <= target < nc:
            raise ValueError(f"target class {target} outside the model's {nc} classes")
        return target
    if not torch.is_tensor(target) or tuple(target.shape) != (Bs, Hs, Ws) or target.is_floating_point() or target.dtype == torch.bool:
        raise ValueError(f"target must be None, an int or an integer tensor [{Bs}, {Hs}, {Ws}] (-1 = skip), "
                         f"got {tuple(target.shape) if torch.is_tensor(target) else type(target)}")
    if target.numel() and int(target.max()) >= nc:
        raise ValueError(f"target class {int(target.max())} outside the model's {nc} classes")
    return target


def scene_saliency(model, scene, target=None, stride=None, max_windows=None):
    """d(score) / d(scene) of a classifier over whole scenes [Bs, C, Hs, Ws]: which bands, at which pixels, drive the class map.

    The score is the sum, over the pixels that count, of the logit map ``predict_scene(..., return_logits=True)`` returns at the pixel's
    target class: for a patch head the mean over the windows covering the pixel (every window's logit there weighs 1 / cover), for a
    pixelwise model the centre logit of the pixel's window.  target: None -- ``predict_scene``'s own class map at this stride; an int;
    or an integer tensor [Bs, Hs, Ws] with -1 = skip.  Pixels no window covers (class -1) never count.  stride and its validation:
    ``predict_scene``'s.

    Eval forward with frozen parameters; the module's mode, the requires_grad flags and the .grad of its parameters are left as found.
    The windows are read in place (``forward_at``) in chunks of max_windows (None: scene.SCENE_MAX_WINDOWS), in grid order; every
    chunk's backward folds its per-window input gradients into the one map with ``msst_scene_fold_at``'s accumulate, whose fixed
    summation order makes the result independent of max_windows, bit for bit.  For that every window must also keep the bits it has in
    one pass over all windows, and the block kernels give a window bits that depend on its place in the batch modulo
    A = ``Engine.window_alignment()`` (21 for 30 bands, 3 for 200): a chunk size of at least A is rounded down to a multiple of A (the
    chunks then start at multiples of A); a smaller one is kept, and every chunk is run behind as many windows with a zero gradient
    as put its windows at their place modulo A (up to A - 1 windows more per chunk, in time and in memory).

    -> SceneSaliency(grad [Bs, C, Hs, Ws] fp32, classes [Bs, Hs, Ws] int64 (predict_scene's, -1 where uncovered), cover [Bs, Hs, Ws]
    int32 (the windows that count at the pixel)).  Raises ValueError for a scene or stride ``predict_scene`` refuses, a target of the
    wrong shape or type, or a class outside the model's."""
    from .engine import SceneGradSink
    from .scene import SCENE_MAX_WINDOWS, _check_scene, forward_at, predict_scene
    if _is_simmim(model):
        raise ValueError("scene_saliency attributes a classifier's class map")
    stride, max_windows = _check_scene(model, scene, stride, SCENE_MAX_WINDOWS if max_windows is None else max_windows)
    Bs, C, Hs, Ws = scene.shape
    w, nc = model.num_spatial_patches_sqrt, model.num_classes
    pix = bool(getattr(model, "pixelwise", False))
    target = _check_scene_target(target, Bs, Hs, Ws, nc)
    model.engine()._require_cuda(scene)
    dev = scene.device
    align = model.engine().window_alignment()
    step = max_windows - max_windows % align if max_windows >= align else max_windows
    classes = predict_scene(model, scene, stride, False, max(step, align))   # chunks that start at multiples of align: one pass's bits
    cover = _scene_cover(Bs, Hs, Ws, w, stride, pix, dev)
    if target is None:
        tmap = classes
    elif isinstance(target, int):
        tmap = torch.full_like(classes, target)
    else:
        tmap = target.to(device=dev, dtype=torch.int64)
    counts = (cover > 0) & (tmap >= 0)
    weight = torch.where(counts, 1.0 / cover.clamp(min=1).float(), torch.zeros((), device=dev))   # [Bs, Hs, Ws] fp32
    tmap = tmap.clamp(min=0)
    nr, nq = (Hs - w) // stride + 1, (Ws - w) // stride + 1
    total = Bs * nr * nq
    number = torch.arange(total, device=dev)
    origins = torch.stack((number // (nr * nq), number % (nr * nq) // nq * stride, number % nq * stride), dim=1).to(torch.int32)
    r = torch.arange(w, device=dev)
    grad = torch.empty(Bs, C, Hs, Ws, dtype=torch.float32, device=dev)
    sink = SceneGradSink(grad)
    was_training = model.training
    if was_training:
        model.eval()
    try:
        with _Frozen(model), torch.enable_grad():
            x = scene.detach().contiguous().float().requires_grad_(True)
            for i in range(0, total, step):
                o = origins[i:i + step]
                n = o.shape[0]
                lead = i % align   # windows run in front of the chunk's, with a zero gradient: 0 when step is a multiple of align
                sc, y0, x0 = o.long().unbind(1)
                if pix:
                    at = (sc, y0 + w // 2, x0 + w // 2)
                    idx, wgt = tmap[at].view(n, 1), weight[at].view(n, 1)
                else:
                    at = (sc[:, None, None], (y0[:, None] + r)[:, :, None], (x0[:, None] + r)[:, None, :])
                    idx, wgt = tmap[at].view(n, 1, w, w), weight[at].view(n, 1, w, w)
                if lead:
                    o = torch.cat((o[:1].expand(lead, 3), o))
                out = forward_at(model, x, o, check=False, scene_grad=sink)
                out = out.view((lead + n, nc) if pix else (lead + n, nc, w, w))
                # d(score)/d(logits): the pixel's weight at its target class, what autograd gives (logits.gather * weight).sum()
                dlogits = torch.zeros_like(out)
                dlogits[lead:].scatter_(1, idx, wgt)
                torch.autograd.backward(out, grad_tensors=dlogits, inputs=[x])
    finally:
        if was_training:
            model.train()
    return SceneSaliency(grad, classes, cover)


def band_importance_scene(model, scene, target=None, stride=None, max_windows=None, mode="grad_x_input"):
    """[Bs, C]: ``scene_saliency``'s attribution of every band, summed over the scene's pixels.  mode "grad_x_input": gradient x input
    (signed); "abs_grad": |gradient|.  model, target, stride, max_windows: as for ``scene_saliency``."""
    if mode not in ("grad_x_input", "abs_grad"):
        raise ValueError(f"unknown mode {mode!r} (use 'grad_x_input' or 'abs_grad')")
    g = scene_saliency(model, scene, target, stride, max_windows).grad
    a = g * scene.detach().to(g.dtype) if mode == "grad_x_input" else g.abs()
    return a.reshape(a.shape[0], a.shape[1], -1).sum(dim=2)
