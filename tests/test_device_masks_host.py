"""Device-side SimMIM masks, host side (no GPU needed): the statistics of the generator as tests/mask_util.py restates it (the GPU
tests hold the kernel to that restatement bit for bit), the closed form of the index rule against MaskGenerator._indices, the C ABI of
msst_draw_masks (additive under MSST_VERSION 109) and its refusals (they run before any HIP call, so host buffers and no device are
enough to see them), and the Python surface as far as it runs before a device is asked for.

The 6 sigma bars are conditions, not measurements: at the same n the host generator topk_masks stays below 4.2 sigma on all three
statistics."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from util import build_product
import mask_util as mu

BADARG, UNSUPPORTED = -3, -2   # include/msst.h: MSST_ERR_BADARG, MSST_ERR_UNSUPPORTED
SEED = 20240917
NROWS = 4096


def sigmas(freq, p, n):
    return float(np.abs(freq - p).max() / np.sqrt(p * (1.0 - p) / n))


# ------------------------------------------------------------------------------------------------------------------ statistics
@pytest.mark.parametrize("image,S", [(6, 7), (8, 20), (4, 3)])   # T = 252, 1280, 48
def test_topk_mode_statistics(image, S):
    cfg = mu.make_cfg(image, S, 1, 0.5)
    T, K = cfg.S * cfg.N, cfg.K
    m = mu.bool_mask(SEED, cfg, np.arange(NROWS))
    assert m.shape == (NROWS, T) and (m.sum(1) == K).all()
    p = K / T
    assert sigmas(m.mean(0), p, NROWS) < 6.0                                     # every token's masked frequency
    assert sigmas((m[:, :-1] & m[:, 1:]).mean(0), p * (K - 1) / (T - 1), NROWS) < 6.0   # adjacent tokens, jointly
    assert sigmas((m[:-1] & m[1:]).mean(0), p * p, NROWS - 1) < 6.0               # the same token in adjacent rows
    other = mu.bool_mask(SEED + 1, cfg, np.arange(64))
    assert (other != m[:64]).any(1).all()                                         # another seed: every row differs


@pytest.mark.parametrize("tube", [False, True])
@pytest.mark.parametrize("image,S,mps,ratio", [(8, 20, 4, 0.7), (8, 20, 2, 0.5), (4, 3, 2, 0.7)])
def test_block_and_tube_mode_statistics(image, S, mps, ratio, tube):
    cfg = mu.make_cfg(image, S, mps, ratio, tube)
    T, tc = cfg.S * cfg.N, cfg.rand_size ** 2
    R = mu.trues_per_row(cfg)
    assert R >= cfg.K
    m = mu.bool_mask(SEED, cfg, np.arange(NROWS))
    assert m.shape == (NROWS, T) and (m.sum(1) == R).all()
    cells = mu.cell_masks(SEED, cfg, np.arange(NROWS))                            # [rows, S or 1, cells]
    assert (cells.sum(2) == cfg.mask_count).all()
    p = cfg.mask_count / tc
    n = cells.shape[0] * cells.shape[1]
    if p < 1.0:
        assert sigmas(cells.reshape(n, tc).mean(0), p, n) < 6.0                   # per-cell frequency, over rows and blocks
        assert sigmas(cells[:, 0].mean(0), p, NROWS) < 6.0                        # ... and of one block over the rows
        assert sigmas((cells[:-1, 0] & cells[1:, 0]).mean(0), p * p, NROWS - 1) < 6.0   # the same cell in adjacent rows
        pj = p * (cfg.mask_count - 1) / (tc - 1)
        if 0.0 < pj:
            assert sigmas((cells[:, :, :-1] & cells[:, :, 1:]).reshape(n, tc - 1).mean(0), pj, n) < 6.0   # adjacent cells, jointly
    # every cell covers scale x scale positions (MaskGenerator._draw's expansion)
    side = cfg.rand_size * cfg.scale
    fine = m.reshape(NROWS, cfg.S, side, side)
    for dy in range(cfg.scale):
        for dx in range(cfg.scale):
            assert np.array_equal(fine[:, :, dy::cfg.scale, dx::cfg.scale], fine[:, :, ::cfg.scale, ::cfg.scale])
    blocks = m.reshape(NROWS, cfg.S, cfg.N)
    if tube:
        assert (blocks == blocks[:, :1]).all()                                    # one draw per row, repeated over the blocks
    elif p < 1.0:
        assert (blocks != blocks[:, :1]).any(axis=(1, 2)).mean() > 0.5            # the blocks of a row are separate draws
        assert sigmas((cells[:, 0] & cells[:, 1]).mean(0), p * p, NROWS) < 6.0    # the same cell in adjacent blocks
    other = mu.bool_mask(SEED + 1, cfg, np.arange(64))
    assert (other != m[:64]).any(1).mean() > 0.5
    assert not np.array_equal(mu.bool_mask(SEED, mu.make_cfg(image, S, mps, ratio, not tube), np.arange(8)), m[:8])   # the modes' streams differ


def test_rows_do_not_depend_on_the_batch():
    """row g is a function of (seed, g): drawn alone, in any range, or as a 64-bit row"""
    for cfg in (mu.make_cfg(4, 3, 1, 0.5), mu.make_cfg(4, 3, 2, 0.7), mu.make_cfg(4, 3, 2, 0.7, True)):
        full = mu.bool_mask(SEED, cfg, np.arange(32))
        assert np.array_equal(mu.bool_mask(SEED, cfg, np.arange(5, 8)), full[5:8])
        assert np.array_equal(mu.bool_mask(SEED, cfg, np.array([31])), full[31:])
        big = np.array([2 ** 33 + 3, 3, 2 ** 32 + 3], dtype=np.uint64)
        far = mu.bool_mask(SEED, cfg, big)
        if cfg.mode == mu.TOPK:   # 24 of 48 tokens: no chance of equal rows (the block modes here have four cells)
            assert not np.array_equal(far[0], far[1]) and not np.array_equal(far[2], far[1]) and not np.array_equal(far[0], far[2])


# ------------------------------------------------------------------------------------------------------------ the index rule
@pytest.mark.parametrize("image,S,mps,ratio,tube", [(8, 20, 4, 0.7, False), (8, 20, 4, 0.7, True), (8, 20, 2, 0.5, False),
                                                    (8, 20, 2, 0.5, True), (4, 3, 2, 0.7, False), (4, 3, 2, 0.7, True), (4, 3, 1, 0.5, False)])
def test_closed_form_of_the_index_rule(image, S, mps, ratio, tube):
    """list position K g + k lies in mask row (K g + k) // R at rank (K g + k) % R: equal to MaskGenerator._indices on the
    materialised global mask, for R > K (misaligned rows) and R == K"""
    from maskedsst_amd.masking import MaskGenerator
    cfg = mu.make_cfg(image, S, mps, ratio, tube)
    R, K, hi = mu.trues_per_row(cfg), cfg.K, 16
    assert R >= K
    full = mu.bool_mask(SEED, cfg, np.arange(hi))
    want = MaskGenerator._indices(full, hi, K)
    assert np.array_equal(mu.closed_form_indices(SEED, cfg, 0, hi), want)
    assert np.array_equal(mu.closed_form_indices(SEED, cfg, 11, hi), want[11:])
    own = np.stack([np.nonzero(r)[0][:K] for r in full])
    if R == K:
        assert np.array_equal(want, own)                     # aligned: every index row lists its own row's trues
    else:
        assert not np.array_equal(want[1:], own[1:])         # misaligned from row 1 on
        assert ((K * np.arange(hi) + K - 1) // R < np.arange(hi)).any()   # ... and some index row lies wholly in an earlier mask row
    # device_masks' two routes agree, CSR included
    a, b = mu.device_masks(SEED, cfg, 3, hi), mu.device_masks(SEED, cfg, 3, hi, closed_form=True)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_duplicates_inside_an_index_row():
    """An index row is the tail of one mask row (ranks >= j0) followed by the head of the next (ranks < j0 - (R - K)); a rank's
    spectral block is rank // (trues per block) in every row.  A token can therefore occur twice only where R - K is smaller than the
    trues per block: at image 4, mask_patch_size 2, S = 3, ratio 0.7 (R = 36, K = 33, 12 per block) it does, at image 8,
    mask_patch_size 4, S = 20, ratio 0.7 (R = 960, K = 896, 48 per block) it cannot -- for this generator and for the host one."""
    cfg = mu.make_cfg(4, 3, 2, 0.7)
    idx = mu.device_masks(SEED, cfg, 0, 16)[1]
    assert any(len(set(r)) < len(r) for r in idx.tolist())
    ptr = mu.device_masks(SEED, cfg, 0, 16)[2]
    assert (np.diff(ptr, axis=1) == 2).any() and np.diff(ptr, axis=1).max() == 2
    cfg = mu.make_cfg(8, 20, 4, 0.7)
    assert mu.trues_per_row(cfg) - cfg.K >= cfg.mask_count * cfg.scale ** 2
    assert all(len(set(r)) == len(r) for r in mu.device_masks(SEED, cfg, 0, 16)[1].tolist())


# --------------------------------------------------------------------------------------------------------------------- C ABI
def test_c_abi_declares_and_exports_msst_draw_masks():
    from maskedsst_amd import _lib
    header = open(_lib.HEADER_PATH).read()
    assert _lib.header_version() == 109   # additive: the revision does not move
    lib = _lib.load()
    assert lib.msst_version() == 109
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"^int msst_draw_masks\(", header, re.M)
    assert "msst_draw_masks" in _lib.declared_symbols()
    assert re.search(r" T msst_draw_masks$", out, re.M)
    for name, value in (("MSST_MASK_TOPK", _lib.MASK_TOPK), ("MSST_MASK_BLOCK", _lib.MASK_BLOCK), ("MSST_MASK_TUBE", _lib.MASK_TUBE)):
        assert re.search(r"^#define %s %d$" % (name, value), header, re.M), name
    assert (mu.TOPK, mu.BLOCK, mu.TUBE) == (_lib.MASK_TOPK, _lib.MASK_BLOCK, _lib.MASK_TUBE)
    import maskedsst_amd
    assert "DeviceMasks" in maskedsst_amd.__all__ and hasattr(maskedsst_amd, "DeviceMasks")
    assert "msst_mask.hip" in __import__("maskedsst_amd.build", fromlist=["SOURCES"]).SOURCES


def test_draw_masks_refuses_bad_arguments_before_launch():
    """host memory stands in for the device buffers: a refused call dereferences nothing and launches nothing"""
    from maskedsst_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * 64)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    names = ["mask", "idx", "csr_ptr", "csr_pos"]

    def call(seed=1, row0=0, rows=2, S=20, N=64, K=896, mode=1, rand_size=2, scale=4, mask_count=3, **null):
        a = [None if null.get(k) else p for k in names]
        return lib.msst_draw_masks(*a, seed, row0, rows, S, N, K, mode, rand_size, scale, mask_count, None)

    all_null = {k: True for k in names}
    for dim in ("rows", "S", "N", "K"):
        for v in (0, -1):
            assert call(**{dim: v}) == BADARG, (dim, v)
    assert b"msst_draw_masks" in lib.msst_last_error()
    assert call(row0=-1) == BADARG
    assert call(K=20 * 64 + 1) == BADARG and call(mode=0, K=20 * 64 + 1) == BADARG     # K > T
    for mode in (-1, 3):
        assert call(mode=mode) == BADARG
    for over in (dict(rand_size=3), dict(scale=2), dict(rand_size=0), dict(scale=0), dict(rand_size=4, scale=4), dict(N=60)):
        for mode in (1, 2):
            assert call(mode=mode, **over) == BADARG, over                               # rand_size * scale is not the spatial side
    for mc in (0, -1, 5):
        assert call(mask_count=mc) == BADARG and call(mode=2, mask_count=mc) == BADARG   # mask_count outside 1 .. token_count
    assert call(mask_count=2) == BADARG and call(mode=2, mask_count=2) == BADARG         # R = 20 * 2 * 16 = 640 < K = 896
    assert b"fewer than K" in lib.msst_last_error()
    assert call(mask_count=2, K=640, **all_null) == BADARG                               # ... R == K is inside; the null pointers are not
    assert b"null" in lib.msst_last_error()
    for k in names:
        assert call(**{k: True}) == BADARG and call(mode=0, **{k: True}) == BADARG, k
    # the top-k mode ignores the three block arguments
    assert call(mode=0, rand_size=0, scale=0, mask_count=0, **all_null) == BADARG and b"null" in lib.msst_last_error()
    # beyond the N / S limits: decided by the sizes alone
    for over in (dict(S=65), dict(N=65), dict(N=81, rand_size=3, scale=3)):
        for mode in (0, 1, 2):
            assert call(mode=mode, **over) == UNSUPPORTED and call(mode=mode, **over, **all_null) == UNSUPPORTED, over
    assert call(S=65, K=0) == BADARG                         # a size below 1 wins over a size beyond the kernel
    assert call(S=64, N=64, K=4096, mode=0, **all_null) == BADARG and b"null" in lib.msst_last_error()   # the limits themselves are inside


# ------------------------------------------------------------------------------------------------------------ Python surface
CFG = dict(bands=30, depth=1, B=2, heads=2, image_size=4, mask_patch_size=2, masking_ratio=0.7, tube_masking=False)


def cpu_device_masks(cfg, lo, hi, seed=SEED):
    from maskedsst_amd import DeviceMasks
    m, idx, ptr, pos = mu.device_masks(seed, cfg, lo, hi)
    return DeviceMasks(torch.from_numpy(m), torch.from_numpy(idx), torch.from_numpy(ptr), torch.from_numpy(pos), seed, lo)


def test_mask_source_validation():
    model, _, _ = build_product(CFG)
    assert model.mask_source == "host"
    for bad in ("gpu", "Device", None, 1, ""):
        with pytest.raises(ValueError, match="mask_source"):
            model.mask_source = bad
    assert model.mask_source == "host"
    model.mask_source = "device"
    assert model.mask_source == "device"
    assert "_mask_source" not in model.state_dict() and not any("mask_source" in k for k in model.state_dict())
    model.mask_source = "host"
    assert model.mask_source == "host"
    bm, idx = model.draw_masks(2)                            # the host source is what it was
    assert bm.shape == (2, 48) and idx.shape == (2, 33)


def test_draw_masks_device_checks_then_refuses_the_cpu():
    from maskedsst_amd import DeviceMasks
    assert DeviceMasks._fields == ("bool_mask", "idx", "csr_ptr", "csr_pos", "seed", "row0")
    model, _, x = build_product(CFG)
    assert mu.cfg_of(model) == mu.make_cfg(4, 3, 2, 0.7)
    for bad in (0, -1, 2.0, True, None, "2"):
        with pytest.raises(ValueError, match="batch"):
            model.draw_masks_device(bad)
    for bad in (-1, 2 ** 32, 1.5, True, "7"):
        with pytest.raises(ValueError, match="seed"):
            model.draw_masks_device(2, seed=bad)
    state = torch.get_rng_state()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.draw_masks_device(2, seed=7)
    assert torch.equal(torch.get_rng_state(), state)         # a given seed leaves torch's generator alone
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.draw_masks_device(2)
    want = torch.get_rng_state()
    torch.set_rng_state(state)
    torch.randint(0, 2 ** 31 - 1, (1,))
    assert torch.equal(torch.get_rng_state(), want)          # seed=None: one draw, the way the dropout seed is drawn
    model.mask_source = "device"
    model.last_masks = None
    for call in (lambda: model(x), lambda: model.reconstruct(x), lambda: model.forward_at(x, torch.tensor([[0, 0, 0], [1, 0, 0]]))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    assert model.last_masks is None


def test_device_masks_argument_is_checked_without_a_device():
    model, _, x = build_product(CFG)
    cfg = mu.cfg_of(model)
    dm = cpu_device_masks(cfg, 0, 2)
    bad = [dm._replace(bool_mask=dm.bool_mask.to(torch.uint8)), dm._replace(idx=dm.idx.long()), dm._replace(csr_ptr=dm.csr_ptr[:, :-1]),
           dm._replace(csr_pos=dm.csr_pos[:1]), dm._replace(idx=dm.idx.t().contiguous().t()), dm._replace(csr_ptr=dm.csr_ptr.numpy()),
           cpu_device_masks(cfg, 0, 3)]
    origins = torch.tensor([[0, 0, 0], [1, 0, 0]])
    for b in bad:
        with pytest.raises(ValueError, match="DeviceMasks"):
            model(x, masks=b)
        with pytest.raises(ValueError, match="DeviceMasks"):
            model.forward_at(x, origins, masks=b)
    model.last_masks = None
    with pytest.raises(RuntimeError, match="no CPU fallback"):   # a well-formed one passes the checks; only the device is missing
        model(x, masks=dm)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.forward_at(x, origins, masks=dm)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.reconstruct(x, masks=dm)
    with pytest.raises(ValueError, match="mask must be a bool"):
        model.reconstruct(x, masks=cpu_device_masks(cfg, 0, 3))
    assert torch.equal(model._token_mask(dm, 2), dm.bool_mask)


def test_micro_masks_on_device_masks():
    from maskedsst_amd import DeviceMasks, micro_masks
    cfg = mu.make_cfg(4, 3, 2, 0.7)
    dm = cpu_device_masks(cfg, 8, 16)
    for K in (1, 2, 4, 8):
        parts = [micro_masks(dm, k, K) for k in range(K)]
        m = 8 // K
        for k, part in enumerate(parts):
            assert isinstance(part, DeviceMasks) and part.seed == dm.seed and part.row0 == 8 + k * m
            for got, whole in zip(part[:4], dm[:4]):
                assert torch.equal(got, whole[k * m:(k + 1) * m]) and got.is_contiguous()
                assert got.data_ptr() == whole[k * m:(k + 1) * m].data_ptr()        # views: no copy
            lone = cpu_device_masks(cfg, part.row0, part.row0 + m)                  # ... and the rows a draw at row0 gives
            assert all(torch.equal(a, b) for a, b in zip(part[:4], lone[:4]))
    for bad in ((dm, 0, 3), (dm, 2, 2), (dm, -1, 2), (dm, 0, 0), (dm._replace(idx=dm.idx[:-1]), 0, 2)):
        with pytest.raises(ValueError):
            micro_masks(*bad)
    bm, idx = micro_masks((dm.bool_mask, dm.idx), 1, 2)                             # the host pair as before
    assert torch.equal(bm, dm.bool_mask[4:]) and torch.equal(idx, dm.idx[4:])


def test_pretrain_parser_takes_device_masks():
    import pretrain
    ap = pretrain.build_parser()
    assert ap.parse_args([]).device_masks is False
    a = ap.parse_args(["--device-masks", "--accumulate", "2"])
    assert a.device_masks is True and a.accumulate == 2


def test_product_still_does_not_import_oracle():
    code = ("import sys; sys.path.insert(0, %r); import maskedsst_amd, maskedsst_amd.engine, maskedsst_amd.masking, pretrain; "
            "assert not any(m == 'oracle' or m.startswith('oracle.') for m in sys.modules), 'oracle imported'" % ROOT)
    subprocess.run([sys.executable, "-c", code], check=True)
    for f in ("masking.py", "vit_simmim_original.py", "engine.py"):
        src = open(os.path.join(ROOT, "maskedsst_amd", f)).read()
        assert "import oracle" not in src and "from oracle" not in src, f
