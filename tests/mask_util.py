"""numpy restatement of the device mask generator (maskedsst_amd/csrc/msst_mask.hip: mask_mix / mask_row_word / mask_key and the
selection), written the way tests/dropout.py restates the dropout hash: the keys and "the m smallest (key, index) pairs" are derived
here; the index rows come from the existing MaskGenerator._indices on the materialised mask of global rows 0 .. hi (code pinned to the
reference's bool_mask_to_indices), and the CSR from the existing inverse_csr."""
from collections import namedtuple

import numpy as np

from maskedsst_amd._lib import MASK_TOPK as TOPK, MASK_BLOCK as BLOCK, MASK_TUBE as TUBE   # include/msst.h: MSST_MASK_*

# S spectral blocks, N positions per block (side^2), K index entries per row; BLOCK / TUBE: rand_size^2 cells per draw, each scale x scale
# positions, mask_count of them masked
MaskCfg = namedtuple("MaskCfg", ["mode", "S", "N", "K", "rand_size", "scale", "mask_count"])


def make_cfg(image_size, S, mask_patch_size, ratio, tube=False):
    """the configuration SimMIMSpatialSpectral(masking_ratio=ratio, mask_patch_size=..., tube_masking=tube) hands the kernel for an
    encoder of image_size^2 positions and S spectral blocks (spatial patch 1)"""
    N = image_size * image_size
    K = int(ratio * S * N)
    if mask_patch_size == 1:
        return MaskCfg(TOPK, S, N, K, 0, 0, 0)
    assert image_size % mask_patch_size == 0
    rand = image_size // mask_patch_size
    return MaskCfg(TUBE if tube else BLOCK, S, N, K, rand, mask_patch_size, int(np.ceil(rand * rand * ratio)))


def cfg_of(model):
    enc = model.encoder
    return make_cfg(enc.image_size, enc.num_spectral_patches, model.mask_patch_size, model.masking_ratio, model.tube_masking)


def trues_per_row(cfg):
    return cfg.K if cfg.mode == TOPK else cfg.S * cfg.mask_count * cfg.scale ** 2


def _u32(x):
    return np.asarray(x).astype(np.uint32)


def mask_mix(x):
    with np.errstate(over="ignore"):
        x = _u32(x).copy()
        x = (x * np.uint32(0x9E3779B1)).astype(np.uint32); x ^= x >> np.uint32(15)
        x = (x * np.uint32(0x85EBCA6B)).astype(np.uint32); x ^= x >> np.uint32(13)
        x = (x * np.uint32(0xC2B2AE35)).astype(np.uint32); x ^= x >> np.uint32(16)
    return x


def mask_row_word(seed, stream, rows, salt):
    rows = np.asarray(rows, dtype=np.uint64)
    first = np.uint32(((stream * 2 + salt + 1) * 0x9E3779B9) & 0xFFFFFFFF) ^ np.uint32(seed)
    h = mask_mix(np.full(rows.shape, first, dtype=np.uint32))
    h = mask_mix(h ^ (rows & np.uint64(0xFFFFFFFF)).astype(np.uint32))
    return mask_mix(h ^ (rows >> np.uint64(32)).astype(np.uint32))


def mask_keys(seed, mode, rows, block, elem):
    """rows [..] uint64 global rows, block / elem integer arrays; all three broadcast -> uint32 keys"""
    rows = np.asarray(rows, dtype=np.uint64)
    ra, rb = mask_row_word(seed, mode + 1, rows, 0), mask_row_word(seed, mode + 1, rows, 1)
    with np.errstate(over="ignore"):
        x = ((_u32(block) << np.uint32(12)) | _u32(elem)) ^ ra
        x = (x * np.uint32(0x9E3779B1)).astype(np.uint32); x ^= x >> np.uint32(15)
        x = (x + rb).astype(np.uint32)
        x = (x * np.uint32(0x85EBCA6B)).astype(np.uint32); x ^= x >> np.uint32(13)
        x = (x * np.uint32(0xC2B2AE35)).astype(np.uint32); x ^= x >> np.uint32(16)
    return x


def smallest(keys, m):
    """bool, same shape: the m entries of the last axis with the smallest (key, index) pairs"""
    order = np.argsort(keys, axis=-1, kind="stable")   # stable: equal keys stay in index order
    out = np.zeros(keys.shape, dtype=bool)
    np.put_along_axis(out, order[..., :m], True, axis=-1)
    return out


def cell_masks(seed, cfg, rows):
    """BLOCK / TUBE: the masked cells, bool [rows, S or 1, rand_size^2]"""
    rows = np.asarray(rows, dtype=np.uint64)
    nblk = 1 if cfg.mode == TUBE else cfg.S
    tc = cfg.rand_size ** 2
    keys = mask_keys(seed, cfg.mode, rows[:, None, None], np.arange(nblk)[None, :, None], np.arange(tc)[None, None, :])
    return smallest(keys, cfg.mask_count)


def bool_mask(seed, cfg, rows):
    """the token mask of the listed global rows: bool [len(rows), S N]"""
    rows = np.asarray(rows, dtype=np.uint64)
    T = cfg.S * cfg.N
    if cfg.mode == TOPK:
        return smallest(mask_keys(seed, TOPK, rows[:, None], 0, np.arange(T)[None, :]), cfg.K)
    cells = cell_masks(seed, cfg, rows).reshape(len(rows), -1, cfg.rand_size, cfg.rand_size)
    fine = cells.repeat(cfg.scale, axis=2).repeat(cfg.scale, axis=3)          # MaskGenerator._draw's expansion
    if cfg.mode == TUBE:
        fine = np.broadcast_to(fine, (len(rows), cfg.S) + fine.shape[2:])
    return np.ascontiguousarray(fine.reshape(len(rows), T))


def closed_form_indices(seed, cfg, lo, hi):
    """index rows lo .. hi - 1 by the row arithmetic of the kernel: list position p = K g + k lies in mask row q = p // R at rank
    j = p % R.  Only the source rows are generated, so lo may be large."""
    K, R = cfg.K, trues_per_row(cfg)
    p = np.arange(lo, hi, dtype=object)[:, None] * K + np.arange(K, dtype=object)[None, :]    # python integers: no overflow
    q, j = p // R, (p % R).astype(np.int64)
    need = sorted(set(q.ravel().tolist()))
    m = bool_mask(seed, cfg, np.array(need, dtype=np.uint64))
    cols = {g: np.nonzero(m[i])[0] for i, g in enumerate(need)}
    out = np.empty((hi - lo, K), dtype=np.int64)
    for r in range(hi - lo):
        for k in range(K):
            out[r, k] = cols[q[r, k]][j[r, k]]
    return out


def device_masks(seed, cfg, lo, hi, closed_form=False):
    """what msst_draw_masks writes for global rows lo .. hi - 1: (mask bool [n, T], idx int32 [n, K], csr_ptr int32 [n, T + 1],
    csr_pos int32 [n, K]).  idx: MaskGenerator._indices on the mask of rows 0 .. hi - 1, rows lo .. hi - 1 of it; closed_form (a lo too
    large to materialise rows 0 .. lo): closed_form_indices, which test_device_masks_host.py holds equal to it."""
    from maskedsst_amd.masking import MaskGenerator, inverse_csr
    T = cfg.S * cfg.N
    if closed_form:
        mask = bool_mask(seed, cfg, np.arange(lo, hi, dtype=np.uint64))
        idx = closed_form_indices(seed, cfg, lo, hi)
    else:
        full = bool_mask(seed, cfg, np.arange(hi, dtype=np.uint64))
        mask, idx = full[lo:hi], MaskGenerator._indices(full, hi, cfg.K)[lo:hi]
    ptr, pos = inverse_csr(idx, T)
    return mask, idx.astype(np.int32), ptr.astype(np.int32), pos.astype(np.int32)
