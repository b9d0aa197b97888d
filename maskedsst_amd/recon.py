"""Reading a SimMIM reconstruction: which bands does the model reconstruct badly?

``SimMIMSpatialSpectral.reconstruct`` returns, beside the reconstructed cube, two small tables per sample and band: the sum of
|prediction - input| over the band's masked pixels and their number (one HIP pass, ``msst_recon_fwd``).  ``recon_report`` turns
them into mean absolute errors on the host, in float64: arithmetic on [B, C] tables only.

``SimMIMSpatialSpectral.reconstruct_scene`` does the same for whole scenes with a mask in scene coordinates (one byte per spectral
block and pixel); ``window_masks_to_scene`` / ``scene_mask_to_windows`` carry masks between the two coordinate systems on the host.
"""
from collections import namedtuple

import torch

# mae: masked MAE over everything (nan when nothing is masked); band_mae [C]: per band, nan for a band with no masked pixel;
# block_mae [S]: per spectral block (P consecutive bands), nan likewise (None when P was not given); band_present [C] bool: the band has masked pixels;
# worst_bands: the present bands, worst first; masked: how many pixels count
ReconReport = namedtuple("ReconReport", ["mae", "band_mae", "block_mae", "band_present", "worst_bands", "masked"])


def recon_report(rec, pixels_per_patch=None):
    """rec: the Reconstruction of ``SimMIMSpatialSpectral.reconstruct`` (or any object with band_err [B, C] and band_cnt [B, C]).
    pixels_per_patch: the bands per spectral block P (``model.pixel_values_per_patch``) for block_mae; None: block_mae is None.
    Bands (blocks) with no masked pixel are ABSENT: nan in band_mae (block_mae), False in band_present, left out of worst_bands --
    never a 0 / 0."""
    err = torch.as_tensor(rec.band_err).detach().to("cpu", torch.float64)
    cnt = torch.as_tensor(rec.band_cnt).detach().to("cpu", torch.float64)
    if err.dim() != 2 or err.shape != cnt.shape:
        raise ValueError(f"band_err {tuple(err.shape)} and band_cnt {tuple(cnt.shape)} must be equal [B, C] tables")
    C = err.shape[1]
    P = None if pixels_per_patch is None else int(pixels_per_patch)
    if P is not None and (P < 1 or C % P):
        raise ValueError(f"{C} bands are not whole spectral blocks of {P}")
    nan = float("nan")

    def ratio(e, n):
        return torch.where(n > 0, e / n.clamp(min=1.0), torch.full_like(e, nan))

    e_band, n_band = err.sum(0), cnt.sum(0)
    band_mae = ratio(e_band, n_band)
    block_mae = None if P is None else ratio(e_band.view(C // P, P).sum(1), n_band.view(C // P, P).sum(1))
    present = n_band > 0
    total = float(n_band.sum())
    mae = float(e_band.sum()) / total if total > 0 else nan
    order = torch.argsort(torch.where(present, band_mae, torch.full_like(band_mae, -1.0)), descending=True, stable=True)
    worst = [int(i) for i in order if present[i]]
    return ReconReport(mae, band_mae, block_mae, present, worst, int(total))


def _window_grid(Hs, Ws, window, stride):
    if isinstance(window, bool) or isinstance(stride, bool) or int(window) != window or int(stride) != stride:
        raise ValueError(f"window and stride must be integers, got {window!r} and {stride!r}")
    window, stride = int(window), int(stride)
    if window < 1 or not 1 <= stride <= window:
        raise ValueError(f"stride must be an integer in [1, {window}] (the window size), got {stride!r}")
    if Hs < window or Ws < window:
        raise ValueError(f"scene {Hs} x {Ws} is smaller than one {window} x {window} window")
    return window, stride, (Hs - window) // stride + 1, (Ws - window) // stride + 1


def window_masks_to_scene(bm, Bs, S, Hs, Ws, window, stride=None):
    """Per-window token masks in scene coordinates: bm bool [Bs nr nq, S window window] (windows in the kernels' order: scene, window
    row, window column; tokens c N + n) -> bool [Bs, S, Hs, Ws], False where no window covers the pixel.  Non-overlapping windows
    only (stride == window, the default): per-window masks of overlapping windows would contradict each other."""
    stride = window if stride is None else stride
    window, stride, nr, nq = _window_grid(Hs, Ws, window, stride)
    if stride != window:
        raise ValueError(f"window masks can be placed in a scene only for stride == window ({window}), got stride {stride}")
    bm = torch.as_tensor(bm)
    if bm.dtype != torch.bool or tuple(bm.shape) != (Bs * nr * nq, S * window * window):
        raise ValueError(f"mask must be a bool [{Bs * nr * nq}, {S * window * window}] tensor (windows, tokens), got {bm.dtype} "
                         f"{tuple(bm.shape)}")
    out = torch.zeros(Bs, S, Hs, Ws, dtype=torch.bool, device=bm.device)
    out[:, :, :nr * window, :nq * window] = (bm.view(Bs, nr, nq, S, window, window).permute(0, 3, 1, 4, 2, 5)
                                             .reshape(Bs, S, nr * window, nq * window))
    return out


def scene_mask_to_windows(mask, window, stride):
    """The inverse view: mask bool [Bs, S, Hs, Ws] -> bool [Bs nr nq, S window window], the token mask of every window (origins 0,
    stride, 2 stride, ...; any stride in 1 .. window) in the kernels' window order and token order c N + n -- what
    ``reconstruct`` takes for the stacked windows."""
    mask = torch.as_tensor(mask)
    if mask.dtype != torch.bool or mask.dim() != 4:
        raise ValueError(f"mask must be a bool [scenes, spectral blocks, H, W] tensor, got {mask.dtype} {tuple(mask.shape)}")
    Bs, S, Hs, Ws = mask.shape
    window, stride, nr, nq = _window_grid(Hs, Ws, window, stride)
    w = mask.unfold(2, window, stride).unfold(3, window, stride)   # [Bs, S, nr, nq, window, window]
    return w.permute(0, 2, 3, 1, 4, 5).reshape(Bs * nr * nq, S * window * window)
