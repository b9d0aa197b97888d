"""Reading a SimMIM reconstruction: which bands does the model reconstruct badly?

``SimMIMSpatialSpectral.reconstruct`` returns, beside the reconstructed cube, two small tables per sample and band: the sum of
|prediction - input| over the band's masked pixels and their number (one HIP pass, ``msst_recon_fwd``).  ``recon_report`` turns
them into mean absolute errors on the host, in float64: arithmetic on [B, C] tables only.
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
