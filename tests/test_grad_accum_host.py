"""Gradient accumulation, host side (no GPU needed): the C ABI of the two launches (additive under MSST_VERSION 109) and their
argument checks, the range table ``GradAccumulator`` builds (``maskedsst_amd.optim.grad_ranges``, on CPU-flattened models) and
``micro_masks``."""
import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import seed_all
from util import build_product

BADARG, UNSUPPORTED = -3, -2   # include/msst.h: MSST_ERR_BADARG, MSST_ERR_UNSUPPORTED
CALLS = ("msst_grad_accumulate", "msst_grad_finalize", "msst_grad_accum_scratch_bytes")


def test_c_abi_declares_and_exports_the_two_launches():
    import maskedsst_amd
    from maskedsst_amd import _lib
    header = open(_lib.HEADER_PATH).read()
    for name in CALLS:
        assert re.search(r"^(int|long) %s\(" % name, header, re.M), name
    assert re.search(r"\}\s*MsstGradRange;", header)
    assert _lib.header_version() == 109
    lib = _lib.load()
    assert lib.msst_version() == 109 and set(CALLS) <= set(_lib.declared_symbols())
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in CALLS:
        assert re.search(r" T %s$" % name, out, re.M), name
    assert ctypes.sizeof(_lib.MsstGradRange) == 16
    m = re.search(r"#define\s+MSST_GRAD_MAX_RANGES\s+(\d+)", header)
    assert m and int(m.group(1)) == _lib.GRAD_MAX_RANGES == 64
    names = [lib.msst_profile_name(i).decode() for i in range(lib.msst_profile_kernels())]
    assert "grad_accumulate" in names and "grad_finalize" in names and "?" not in names
    # 12 bytes per workgroup of the capped grid, one workgroup more per range at most
    assert lib.msst_grad_accum_scratch_bytes(0) == 0 and lib.msst_grad_accum_scratch_bytes(65) == 0
    assert lib.msst_grad_accum_scratch_bytes(1) >= 12 * 513 and lib.msst_grad_accum_scratch_bytes(64) >= 12 * (512 + 64)
    for name in ("GradAccumulator", "micro_masks"):
        assert name in maskedsst_amd.__all__ and hasattr(maskedsst_amd, name)


def test_both_launches_refuse_bad_arguments_on_the_host_in_the_stated_order():
    """every check runs before anything is enqueued, so host memory and no device are enough to see it"""
    from maskedsst_amd import _lib
    lib = _lib.load()
    G = _lib.MsstGradRange
    nbytes = ctypes.sizeof(G)
    buf = [(ctypes.c_double * 64)() for _ in range(4)]
    a, g, s, r = (ctypes.cast(b, ctypes.c_void_p) for b in buf)

    def table(rows):
        return (G * max(1, len(rows)))(*[G(*x) for x in rows])

    def accumulate(rows, acc=a, grad=g, n=None, range_bytes=nbytes, tab=True):
        return lib.msst_grad_accumulate(acc, grad, table(rows) if tab else None, len(rows) if n is None else n, range_bytes, 1, None, 1.0,
                                        None, None)

    def finalize(rows, acc=a, grad=g, n=None, range_bytes=nbytes, tab=True, scratch=s, record=r):
        return lib.msst_grad_finalize(acc, grad, table(rows) if tab else None, len(rows) if n is None else n, range_bytes, 1.0, 1.0,
                                      scratch, record, None)

    ok = [(0, 8)]
    over = [(i, i + 1) for i in range(_lib.GRAD_MAX_RANGES + 1)]
    for call in (accumulate, finalize):
        # 1. null required pointers, ahead of everything else
        for kw in (dict(acc=None), dict(grad=None), dict(tab=False)):
            assert call([], range_bytes=nbytes - 4, **kw) == BADARG and b"null" in lib.msst_last_error(), kw
        # 2. nranges < 1, ahead of the struct size
        assert call([], range_bytes=nbytes - 4) == BADARG and b"nranges < 1" in lib.msst_last_error()
        assert call(ok, n=-1) == BADARG and b"nranges < 1" in lib.msst_last_error()
        # 3. another revision's struct, ahead of the table's length
        assert call(over, range_bytes=nbytes + 8) == BADARG and b"revision" in lib.msst_last_error()
        # 4. more ranges than the table holds: unsupported, ahead of the table's contents
        assert call([(5, 5)] + over[1:]) == UNSUPPORTED and b"MSST_GRAD_MAX_RANGES" in lib.msst_last_error()
        # 5. empty, inverted and negative ranges
        for rows in ([(5, 5)], [(8, 4)], [(-4, 4)], [(0, 8), (12, 12)]):
            assert call(rows) == BADARG and b"end <= start" in lib.msst_last_error(), rows
        # 6. overlapping and descending ranges
        for rows in ([(0, 8), (4, 12)], [(8, 16), (0, 8)], [(0, 8), (8, 16), (15, 20)]):
            assert call(rows) == BADARG and b"overlap" in lib.msst_last_error(), rows
    for kw in (dict(scratch=None), dict(record=None)):
        assert finalize(ok, **kw) == BADARG and b"null" in lib.msst_last_error(), kw
    # after the table: a scratch that is not 8-byte aligned, an output that is the accumulation buffer
    odd = ctypes.c_void_p(s.value + 4)
    assert finalize(ok, scratch=odd) == BADARG and b"aligned" in lib.msst_last_error()
    assert finalize(ok, grad=a) == BADARG and b"must not be acc" in lib.msst_last_error()
    assert lib.msst_grad_accumulate(a, g, table(ok), 1, nbytes, 1, None, 1.0, odd, None) == BADARG and b"aligned" in lib.msst_last_error()
    assert lib.msst_grad_accumulate(a, g, table(ok), 1, nbytes, 1, a, 1.0, None, None) == BADARG and b"must not be acc" in lib.msst_last_error()


# ----------------------------------------------------------------------------------------------- the range table
def give_grads(named, fp, skip=()):
    """what the HIP backward leaves: every .grad the parameter's own view of the flat gradient buffer"""
    base = fp.flat.data_ptr()
    for n, p in named:
        if p.requires_grad and n not in skip:
            off = (p.data_ptr() - base) // 4
            p.grad = fp.grad[off:off + p.numel()].view(p.shape)


def simmim(depth=1):
    from maskedsst_amd.flat import FlatParams
    model, _, _ = build_product(dict(bands=20, depth=depth, B=2, heads=2))
    fp = FlatParams(model.encoder, model).flatten()
    trainable = [(n, p) for _, g in fp._ordered()[0] for n, p in g]   # Engine.trainable()
    return model, fp, trainable


def encoder(depth=2):
    from maskedsst_amd import ViTSpatialSpectral
    from maskedsst_amd.flat import FlatParams
    seed_all(5)
    enc = ViTSpatialSpectral(image_size=8, spatial_patch_size=1, spectral_patch_size=10, num_classes=8, dim=96, depth=depth, heads=8,
                             mlp_dim=64, channels=50, spectral_pos_embed=False, spectral_pos=torch.arange(5))
    fp = FlatParams(enc, None).flatten()
    return enc, fp, [(n, p) for _, g in fp._ordered()[0] for n, p in g]


def test_ranges_of_a_trainable_simmim_model_are_the_trainable_prefix():
    from maskedsst_amd.optim import grad_ranges
    model, fp, trainable = simmim()
    assert grad_ranges(fp, [p for _, p in trainable]) == []          # no backward yet: nothing holds a gradient
    give_grads(trainable, fp)
    r = grad_ranges(fp, [p for _, p in trainable])
    assert [(x.start, x.end) for x in r] == [(0, fp.n_trainable)]    # every neighbouring segment merged
    assert 0 < fp.n_trainable < fp.total and len(r[0].params) == len(trainable)
    assert fp.accum is None and fp.accum_buffer().shape == fp.grad.shape and fp.accum_buffer() is fp.accum
    fp.flatten()
    assert fp.accum is None   # a re-flatten drops it: the next use allocates it for the new layout


def test_ranges_linear_eval_is_the_head_alone():
    from maskedsst_amd.optim import grad_ranges
    enc, fp, trainable = encoder()
    for n, p in enc.named_parameters():
        p.requires_grad_("mlp_head" in n)
    give_grads(trainable, fp)
    r = grad_ranges(fp, [p for _, p in trainable])
    segs = [v for k, v in fp.segments.items() if k.startswith("mlp_head.")]
    assert [(x.start, x.end) for x in r] == [(0, max(o + n for o, n, _ in segs))] and len(r[0].params) == 4


def test_ranges_frozen_tensor_in_the_middle_leaves_a_hole():
    from maskedsst_amd.optim import grad_ranges
    enc, fp, trainable = encoder()
    frozen = dict(enc.named_parameters())["spatial_spectral_transformer.1.layers.0.1.fn.net.0.weight"]   # w1 of spatial block 0
    nograd = dict(enc.named_parameters())["to_patch_embedding.pre_norm.weight"]
    frozen.requires_grad_(False)
    give_grads(trainable, fp)
    nograd.grad = None
    r = grad_ranges(fp, [p for _, p in trainable])
    assert len(r) == 3 and r[0].start == 0 and r[-1].end == fp.total
    holes = [(a.end, b.start) for a, b in zip(r, r[1:])]
    want = sorted(((p.data_ptr() - fp.flat.data_ptr()) // 4, (p.data_ptr() - fp.flat.data_ptr()) // 4 + p.numel()) for p in (frozen, nograd))
    assert holes == want
    assert all(a.end < b.start for a, b in zip(r, r[1:]))


def test_ranges_over_the_cap_and_foreign_gradients_raise():
    from maskedsst_amd import _lib
    from maskedsst_amd.optim import grad_ranges
    enc, fp, trainable = encoder(depth=6)
    for i, (_, p) in enumerate(trainable):   # every other tensor frozen: one range per surviving tensor
        p.requires_grad_(i % 2 == 0)
    give_grads(trainable, fp)
    assert len(trainable) // 2 > _lib.GRAD_MAX_RANGES
    with pytest.raises(ValueError, match="ranges"):
        grad_ranges(fp, [p for _, p in trainable], _lib.GRAD_MAX_RANGES)
    enc, fp, trainable = encoder()
    give_grads(trainable, fp)
    p = trainable[3][1]
    p.grad = p.grad.clone()
    with pytest.raises(RuntimeError, match="no view of the flat gradient buffer"):
        grad_ranges(fp, [p for _, p in trainable])


# ----------------------------------------------------------------------------------------------- micro_masks
def rng_state():
    return np.random.get_state()[1].copy(), np.random.get_state()[2], torch.get_rng_state().clone()


def same_state(a, b):
    return bool((a[0] == b[0]).all()) and a[1] == b[1] and torch.equal(a[2], b[2])


@pytest.mark.parametrize("K", [1, 2, 4])
@pytest.mark.parametrize("kind", ["tube", "non_tube", "mask_patch_1"])
def test_micro_masks_are_the_rows_of_the_global_draw(kind, K):
    from maskedsst_amd import micro_masks
    cfg = dict(bands=20, depth=1, B=8, heads=2, **{"tube": {}, "non_tube": dict(tube_masking=False), "mask_patch_1": dict(mask_patch_size=1)}[kind])
    model, _, _ = build_product(cfg)
    seed_all(9)
    start = rng_state()
    bm, idx = model.draw_masks(8)
    after = rng_state()
    assert not same_state(start, after)
    parts = [micro_masks((bm, idx), k, K) for k in range(K)]
    assert same_state(after, rng_state())   # slicing draws nothing: the generators have advanced exactly once, for the global batch
    assert all(p[0].shape[0] == 8 // K and p[1].shape[0] == 8 // K for p in parts)
    assert torch.equal(torch.cat([p[0] for p in parts]), bm) and torch.equal(torch.cat([p[1] for p in parts]), idx)
    # ... and once more gives what a second global draw gives
    again = model.draw_masks(8)
    seed_all(9)
    model.draw_masks(8)
    second = model.draw_masks(8)
    assert torch.equal(again[0], second[0]) and torch.equal(again[1], second[1])
    for bad in ((bm, idx, 0, 3), (bm, idx, 2, 2), (bm, idx, -1, 2), (bm[:4], idx, 0, 2)):
        with pytest.raises(ValueError):
            micro_masks((bad[0], bad[1]), bad[2], bad[3])
