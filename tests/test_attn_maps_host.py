"""Attention maps, host side (no GPU needed): the C ABI of msst_attn_maps (additive under MSST_VERSION 109) and its argument checks
(they run before any HIP call, so null pointers, host buffers and no device are enough to see them), the ValueErrors of
attention_maps that need no device, the refusal of CPU tensors, attention_rollout / attention_received against a numpy float64
restatement, and the flag of finetune.py."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

BADARG, UNSUPPORTED = -3, -2   # include/msst.h: MSST_ERR_BADARG, MSST_ERR_UNSUPPORTED


def make_encoder(**kw):
    from maskedsst_amd import ViTSpatialSpectral
    torch.manual_seed(5)
    return ViTSpatialSpectral(image_size=kw.pop("image_size", 8), spatial_patch_size=1, spectral_patch_size=10, num_classes=4, dim=96,
                              depth=kw.pop("depth", 2), heads=8, mlp_dim=64, channels=50, spectral_pos=torch.arange(5),
                              blockwise_patch_embed=True, **kw)


def make_mim():
    from maskedsst_amd import SimMIMSpatialSpectral
    return SimMIMSpatialSpectral(encoder=make_encoder(), masking_ratio=0.7, mask_patch_size=4, tube_masking=True,
                                 to_pixels_per_spectral_block=True)


# --------------------------------------------------------------------------------------------------------------------- C ABI
def test_c_abi_declares_and_exports_the_entry_point():
    from ctypes import c_int, c_long, c_void_p
    from maskedsst_amd import _lib
    header = open(_lib.HEADER_PATH).read()
    assert _lib.header_version() == 109   # additive: the revision does not move
    lib = _lib.load()
    assert lib.msst_version() == 109
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"^int msst_attn_maps\(", header, re.M)
    assert re.search(r"^#define MSST_ATTN_PER_SEQ\s+0$", header, re.M) and re.search(r"^#define MSST_ATTN_MEAN_SEQ\s+1$", header, re.M)
    assert (_lib.ATTN_PER_SEQ, _lib.ATTN_MEAN_SEQ) == (0, 1)
    assert "msst_attn_maps" in _lib.declared_symbols()
    assert re.search(r" T msst_attn_maps$", out, re.M)
    P = c_void_p
    # const float* x, ln_g, ln_b, wqkv, float* maps, long sample_stride, int mode, B, S, N, heads, reduce, void* stream
    assert _lib._SIGS["msst_attn_maps"] == (c_int, [P, P, P, P, P, c_long] + [c_int] * 6 + [P])
    assert (lib.msst_attn_maps.restype, list(lib.msst_attn_maps.argtypes)) == _lib._SIGS["msst_attn_maps"]
    import maskedsst_amd
    for name in ("AttentionMaps", "attention_rollout", "attention_received"):
        assert name in maskedsst_amd.__all__ and hasattr(maskedsst_amd, name), name
    assert maskedsst_amd.AttentionMaps._fields == ("spatial", "spectral")
    assert hasattr(maskedsst_amd.ViTSpatialSpectral, "attention_maps") and hasattr(maskedsst_amd.SimMIMSpatialSpectral, "attention_maps")
    from maskedsst_amd.engine import Engine
    assert hasattr(Engine, "attn_maps_block") and hasattr(Engine, "attention_maps")
    assert "msst_attn_maps.hip" in __import__("maskedsst_amd.build", fromlist=["SOURCES"]).SOURCES


def _ptr():
    buf = (ctypes.c_char * 64)()
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)


def test_attn_maps_refuses_bad_arguments_before_launch():
    from maskedsst_amd import _lib
    lib = _lib.load()
    buf, p = _ptr()
    names = ("x", "ln_g", "ln_b", "wqkv", "maps")

    def call(stride=None, mode=1, B=2, S=5, N=64, heads=8, reduce=1, **ptr):
        a = {k: ptr.get(k, p) for k in names}
        if stride is None:
            L, G = (N, S) if mode == 0 else (S, N)
            stride = max(1, (G if reduce == 0 else 1) * heads * L * L)
        return lib.msst_attn_maps(a["x"], a["ln_g"], a["ln_b"], a["wqkv"], a["maps"], stride, mode, B, S, N, heads, reduce, None)

    null = {k: None for k in names}
    for over in (dict(N=65), dict(S=65), dict(heads=17), dict(N=65, S=65, heads=17)):
        assert call(**over) == UNSUPPORTED and call(**over, **null) == UNSUPPORTED, over   # decided by the sizes alone
        assert call(mode=7, reduce=-1, stride=0, **over) == UNSUPPORTED, over
    assert b"msst_attn_maps" in lib.msst_last_error()
    for dim in ("B", "S", "N", "heads"):
        for v in (0, -1):
            assert call(**{dim: v}) == BADARG and call(**{dim: v}, **null) == BADARG, (dim, v)
    assert b"msst_attn_maps" in lib.msst_last_error()
    assert call(N=65, S=0) == BADARG and call(heads=17, B=0) == BADARG     # a size below 1 wins over a size beyond the kernel
    assert call(N=64, S=64, heads=16, **null) == BADARG                   # the limits themselves are inside (then: null pointers)
    for mode in (-1, 2):
        assert call(mode=mode, stride=1 << 20) == BADARG, mode
    for reduce in (-1, 2):
        assert call(reduce=reduce, stride=1 << 20) == BADARG, reduce
    for k in names:
        assert call(**{k: None}) == BADARG, k
    off = ctypes.c_void_p(p.value + 4)
    assert call(x=off) == BADARG and call(maps=off) == BADARG             # 16-byte loads of x; the slices of maps start on 16 bytes
    # sample_stride: one sample's maps, by mode and reduce (spectral: L = S = 5, G = N = 64; spatial: L = N = 64, G = S = 5)
    for mode, reduce, need in ((1, 1, 8 * 25), (1, 0, 64 * 8 * 25), (0, 1, 8 * 4096), (0, 0, 5 * 8 * 4096)):
        assert call(mode=mode, reduce=reduce, stride=need - 1) == BADARG, (mode, reduce)
        assert call(mode=mode, reduce=reduce, stride=0) == BADARG and call(mode=mode, reduce=reduce, stride=-need) == BADARG
    assert b"sample_stride" in lib.msst_last_error()


# ------------------------------------------------------------------------------------------------------------------ the models' call
def test_attention_maps_refuses_bad_arguments():
    enc, mim = make_encoder(), make_mim()
    good = torch.zeros(2, 50, 8, 8)
    for model in (enc, mim):
        for shape in ((50, 8, 8), (2, 40, 8, 8), (2, 50, 7, 8), (2, 50, 8, 9), (0, 50, 8, 8)):   # rank, band count, image size, empty batch
            with pytest.raises(ValueError):
                model.attention_maps(torch.zeros(shape))
        for stack in ("", "all", None, 0, "Spatial"):
            with pytest.raises(ValueError, match="stack"):
                model.attention_maps(good, stack=stack)
        for reduce in ("sum", "none", 0, False, "Mean"):
            with pytest.raises(ValueError, match="reduce"):
                model.attention_maps(good, reduce=reduce)
        for blocks in ([2], [-1], [0, 5], [1.0], [True], [], [0, 0]):                            # depth 2: layers 0 and 1
            with pytest.raises(ValueError, match="block"):
                model.attention_maps(good, blocks=blocks)
    with pytest.raises(ValueError, match="mask"):
        mim.attention_maps(good, masks=torch.zeros(2, 5 * 64 - 1, dtype=torch.bool))
    with pytest.raises(ValueError, match="mask"):
        mim.attention_maps(good, masks=torch.zeros(2, 5 * 64))


def test_attention_maps_has_no_cpu_fallback():
    enc, mim = make_encoder(), make_mim()
    img = torch.zeros(2, 50, 8, 8)
    enc.train()
    for kw in (dict(), dict(stack="spectral", reduce=None), dict(blocks=[1], stack="spatial")):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            enc.attention_maps(img, **kw)
    assert enc.training
    mim.eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mim.attention_maps(img)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mim.attention_maps(img, masks=mim.draw_masks(2))
    assert not mim.training


def test_docstrings_state_the_precision_rule_and_the_size():
    import maskedsst_amd
    doc = " ".join(maskedsst_amd.ViTSpatialSpectral.attention_maps.__doc__.split())
    assert "fp32 softmax" in doc and "bf16 model" in doc and "half rounding" in doc
    assert "B S heads N^2 4 bytes per spatial block" in doc


# ---------------------------------------------------------------------------------------------------- rollout / received, float64
def _maps(B, nblk, H, L, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.softmax(2.0 * torch.randn(B, nblk, H, L, L, generator=g), dim=-1)


def _rollout_np(maps, residual):
    a = maps.numpy().astype(np.float64).mean(axis=2)
    if residual:
        a = (a + np.eye(a.shape[-1])) / 2
    out = a[:, 0]
    for l in range(1, a.shape[1]):
        out = np.einsum("bij,bjk->bik", a[:, l], out)
    return out


@pytest.mark.parametrize("B,nblk,H,L", [(2, 3, 4, 5), (1, 1, 2, 20), (3, 12, 8, 7), (2, 2, 3, 64)])
def test_rollout_and_received_against_numpy_float64(B, nblk, H, L):
    from maskedsst_amd import attention_rollout, attention_received
    maps = _maps(B, nblk, H, L, 11 + L)
    for residual in (True, False):
        got = attention_rollout(maps, residual=residual)
        assert got.dtype == torch.float64 and tuple(got.shape) == (B, L, L)
        assert np.abs(got.numpy() - _rollout_np(maps, residual)).max() <= 1e-12
    maps64 = maps.double() / maps.double().sum(dim=-1, keepdim=True)
    for residual in (True, False):                                            # rows that sum to 1 in float64: so do the rollout's
        assert np.abs(attention_rollout(maps64, residual=residual).numpy().sum(axis=-1) - 1.0).max() <= 1e-12
    rec = attention_received(maps64)
    assert tuple(rec.shape) == (B, nblk, L) and rec.dtype == torch.float64
    assert np.abs(rec.numpy() - maps64.numpy().mean(axis=(2, 3))).max() <= 1e-12
    assert np.abs(rec.numpy().sum(axis=-1) - 1.0).max() <= 1e-12
    assert attention_received(maps).dtype == torch.float32


def test_rollout_special_cases():
    from maskedsst_amd import attention_rollout, attention_received
    maps = _maps(2, 1, 4, 6, 3)
    one = attention_rollout(maps, residual=False)                             # one block, no residual: the head mean
    assert np.abs(one.numpy() - maps.double().mean(dim=2)[:, 0].numpy()).max() <= 1e-12
    eye = torch.eye(6).expand(2, 5, 4, 6, 6)
    for residual in (True, False):                                            # identity maps give the identity
        assert torch.equal(attention_rollout(eye, residual=residual), torch.eye(6, dtype=torch.float64).expand(2, 6, 6))
    assert torch.equal(attention_received(eye), torch.full((2, 5, 6), 1.0 / 6))
    # order: the LAST block multiplies from the left
    a = _maps(1, 2, 1, 4, 9)
    want = a[0, 1, 0].double() @ a[0, 0, 0].double()
    assert np.abs(attention_rollout(a, residual=False)[0].numpy() - want.numpy()).max() <= 1e-12
    for bad in (torch.zeros(2, 3, 4, 5), torch.zeros(2, 3, 4, 5, 6), None):
        with pytest.raises(ValueError):
            attention_rollout(bad)
        with pytest.raises(ValueError):
            attention_received(bad)


# ------------------------------------------------------------------------------------------------------------------- scripts
def test_finetune_parser_takes_val_attention():
    import finetune
    ap = finetune.build_parser()
    assert ap.parse_args(["enmap"]).val_attention is False
    assert ap.parse_args(["enmap", "--val-scenes", "2", "--val-attention"]).val_attention is True


def test_product_still_does_not_import_oracle():
    code = ("import sys; sys.path.insert(0, %r); import maskedsst_amd, maskedsst_amd.engine, maskedsst_amd.attention; "
            "assert not any(m == 'oracle' or m.startswith('oracle.') for m in sys.modules), 'oracle imported'" % ROOT)
    subprocess.run([sys.executable, "-c", code], check=True)
    src = open(os.path.join(ROOT, "maskedsst_amd", "attention.py")).read()
    assert "import oracle" not in src and "from oracle" not in src
    assert "layer_norm" not in src and "torch.softmax" not in src and "matmul" not in src   # nothing of the model is restated
