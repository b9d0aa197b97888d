"""Attention maps: which spectral blocks attend to which, and which positions of a window attend to which.

The probabilities come out of ``msst_attn_maps`` (``maskedsst_amd/csrc/msst_attn_maps.hip``) through
``ViTSpatialSpectral.attention_maps`` / ``SimMIMSpatialSpectral.attention_maps``; nothing of the model is restated here.  What
follows the kernel is thin torch code on its result:

    attention_rollout   the product of the head-averaged maps of a stack (Abnar & Zuidema 2020)
    attention_received  how much attention each key receives, per block
"""
from collections import namedtuple

import torch

__all__ = ["AttentionMaps", "attention_rollout", "attention_received"]

AttentionMaps = namedtuple("AttentionMaps", "spatial spectral")

_STACKS = {"spatial": ("spatial",), "spectral": ("spectral",), "both": ("spatial", "spectral")}


def _attention_maps(enc, img, mask_u8, stack, reduce, blocks):
    """the checks and the engine call behind both modules' attention_maps; mask_u8: [B, T] uint8 on img's device, or None"""
    from . import _lib
    s = enc.num_spatial_patches_sqrt
    C = enc.num_spectral_patches * enc.patch_depth
    if not torch.is_tensor(img) or img.dim() != 4:
        raise ValueError(f"img must be a 4-D tensor [batch, bands, H, W], got {getattr(img, 'shape', type(img))}")
    if img.shape[0] < 1 or tuple(img.shape[1:]) != (C, s, s):
        raise ValueError(f"img {tuple(img.shape)} is not [batch, {C}, {s}, {s}] (the model's bands and image size)")
    if not isinstance(stack, str) or stack not in _STACKS:
        raise ValueError(f"unknown stack {stack!r} (use 'spatial', 'spectral' or 'both')")
    if reduce is not None and reduce != "mean":
        raise ValueError(f"unknown reduce {reduce!r} (use 'mean' or None)")
    if blocks is None:
        blocks = list(range(enc.depth))
    else:
        blocks = list(blocks)
        for l in blocks:
            if isinstance(l, bool) or not isinstance(l, int) or not 0 <= l < enc.depth:
                raise ValueError(f"block index {l!r} outside the stack's layers 0 .. {enc.depth - 1}")
        if not blocks or len(set(blocks)) != len(blocks):
            raise ValueError(f"blocks must name at least one layer and none twice, got {blocks}")
    eng = enc.engine()
    eng._require_cuda(img)
    spatial, spectral = eng.attention_maps(img, mask_u8, _STACKS[stack], blocks,
                                           _lib.ATTN_MEAN_SEQ if reduce == "mean" else _lib.ATTN_PER_SEQ)
    return AttentionMaps(spatial, spectral)


def _check_maps(maps):
    if not torch.is_tensor(maps) or maps.dim() != 5 or maps.shape[-1] != maps.shape[-2]:
        raise ValueError(f"maps must be [B, nblk, heads, L, L] (attention_maps with reduce='mean'), got "
                         f"{tuple(getattr(maps, 'shape', ()))}")


def attention_rollout(maps, residual=True):
    """Attention rollout of one stack: maps [B, nblk, heads, L, L] (``attention_maps(...).spatial`` or ``.spectral`` with
    ``reduce="mean"``, blocks in forward order) -> [B, L, L] float64.  The heads are averaged; with ``residual`` every block's map
    becomes (A + I) / 2 -- the skip connection carries half of the token itself; the result is the product A_last ... A_0, so row i
    says how much of each INPUT token of the stack has flowed into token i after the last block.  Rows sum to 1."""
    _check_maps(maps)
    a = maps.to(torch.float64).mean(dim=2)
    if residual:
        a = (a + torch.eye(a.shape[-1], dtype=torch.float64, device=a.device)) / 2
    out = a[:, 0]
    for l in range(1, a.shape[1]):
        out = a[:, l] @ out
    return out


def attention_received(maps):
    """[B, nblk, L]: for every block the mean over heads and queries of each key's column of maps [B, nblk, heads, L, L] -- which
    spectral blocks (or window positions) are attended to.  Every [b, blk] row sums to 1; the maps' dtype is kept."""
    _check_maps(maps)
    return maps.mean(dim=(2, 3))
