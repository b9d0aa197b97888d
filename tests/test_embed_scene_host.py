"""Whole-scene embedding maps, host side (no GPU needed): the C ABI of msst_pool_spectral_fwd / msst_scene_embed_assemble (additive under
MSST_VERSION 109) and their argument checks (they run before any HIP call, so null pointers, host buffers and no device are enough to
see them), the ValueErrors of encode_scene that need no device, the refusal of CPU tensors, and the flag of finetune.py."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

BADARG, UNSUPPORTED = -3, -2   # include/msst.h: MSST_ERR_BADARG, MSST_ERR_UNSUPPORTED
CALLS = ("msst_pool_spectral_fwd", "msst_scene_embed_assemble")


def make_encoder(**kw):
    from maskedsst_amd import ViTSpatialSpectral
    torch.manual_seed(5)
    return ViTSpatialSpectral(image_size=kw.pop("image_size", 8), spatial_patch_size=1, spectral_patch_size=10, num_classes=4, dim=96, depth=1,
                              heads=8, mlp_dim=64, channels=50, spectral_pos=torch.arange(5), blockwise_patch_embed=True, **kw)


# --------------------------------------------------------------------------------------------------------------------- C ABI
def test_c_abi_declares_and_exports_the_entry_points():
    from ctypes import c_int, c_long, c_void_p
    from maskedsst_amd import _lib
    header = open(_lib.HEADER_PATH).read()
    assert _lib.header_version() == 109   # additive: the revision does not move
    lib = _lib.load()
    assert lib.msst_version() == 109
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in CALLS:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in _lib.declared_symbols()
        assert re.search(r" T %s$" % name, out, re.M), name
    P = c_void_p
    # const float* y, float* out, int B, int S, int N, void* stream
    assert _lib._SIGS["msst_pool_spectral_fwd"] == (c_int, [P, P, c_int, c_int, c_int, P])
    assert (lib.msst_pool_spectral_fwd.restype, list(lib.msst_pool_spectral_fwd.argtypes)) == _lib._SIGS["msst_pool_spectral_fwd"]
    # const float* win_feat, long win0, int nwin, float* feat, int32_t* cover, int Bs, D, Hs, Ws, window, stride, finalize, l2norm, void* stream
    assert _lib._SIGS["msst_scene_embed_assemble"] == (c_int, [P, c_long, c_int, P, P] + [c_int] * 8 + [P])
    assert (lib.msst_scene_embed_assemble.restype, list(lib.msst_scene_embed_assemble.argtypes)) == _lib._SIGS["msst_scene_embed_assemble"]
    import maskedsst_amd
    assert "SceneEmbedding" in maskedsst_amd.__all__ and maskedsst_amd.SceneEmbedding._fields == ("features", "cover")
    assert hasattr(maskedsst_amd.ViTSpatialSpectral, "encode_scene")


def _ptr():
    buf = (ctypes.c_char * 64)()
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)


def test_pool_spectral_refuses_bad_arguments_before_launch():
    from maskedsst_amd import _lib
    lib = _lib.load()
    buf, p = _ptr()

    def call(y=p, out=p, B=2, S=5, N=64):
        return lib.msst_pool_spectral_fwd(y, out, B, S, N, None)

    for over in (dict(N=65), dict(S=65), dict(N=65, S=65)):
        assert call(**over) == UNSUPPORTED and call(y=None, out=None, **over) == UNSUPPORTED, over   # decided by the sizes alone
    assert b"msst_pool_spectral_fwd" in lib.msst_last_error()
    for dim in ("B", "S", "N"):
        for v in (0, -1):
            assert call(**{dim: v}) == BADARG and call(y=None, out=None, **{dim: v}) == BADARG, (dim, v)
    assert call(N=65, S=0) == BADARG                                  # a size below 1 wins over a size beyond the kernel
    assert call(y=None, out=None, N=64, S=64) == BADARG              # the limits themselves are inside
    assert call(y=None) == BADARG and call(out=None) == BADARG
    assert call(y=ctypes.c_void_p(p.value + 4)) == BADARG            # 16-byte loads


def test_scene_embed_assemble_refuses_bad_arguments_before_launch():
    from maskedsst_amd import _lib
    lib = _lib.load()
    buf, p = _ptr()
    names = ["win_feat", "feat", "cover"]

    def call(win0=0, nwin=4, Bs=2, D=96, Hs=19, Ws=21, window=8, stride=3, finalize=1, l2norm=0, **null):
        a = {k: (None if null.get(k) else p) for k in names}
        return lib.msst_scene_embed_assemble(a["win_feat"], win0, nwin, a["feat"], a["cover"], Bs, D, Hs, Ws, window, stride, finalize,
                                             l2norm, None)

    all_null = {k: True for k in names}
    for dim in ("Bs", "D", "Hs", "Ws", "window", "stride"):
        for v in (0, -1):
            assert call(**{dim: v}) == BADARG and call(**{dim: v}, **all_null) == BADARG, (dim, v)
    assert call(nwin=-1) == BADARG and call(win0=-1) == BADARG
    assert b"msst_scene_embed_assemble" in lib.msst_last_error()
    for over in (dict(D=129), dict(window=9, stride=9, Hs=20), dict(stride=9), dict(Hs=7), dict(Ws=7), dict(window=20, Hs=20, Ws=20)):
        assert call(**over) == UNSUPPORTED and call(**over, **all_null) == UNSUPPORTED, over   # decided by the sizes alone
    assert call(D=128, **all_null) == BADARG                     # the limit itself is inside
    assert call(D=129, stride=0) == BADARG                       # a size below 1 wins over a size beyond the kernel
    for k in names:
        assert call(**{k: True}) == BADARG, k
    assert call(win0=2 * 4 * 5 - 3, **all_null) == BADARG and call(nwin=2 * 4 * 5 + 1, **all_null) == BADARG
    assert call(win0=2 * 4 * 5 - 3) == BADARG and call(nwin=2 * 4 * 5 + 1) == BADARG   # windows beyond Bs nr nq (4 x 5 per scene)
    assert b"out of range" in lib.msst_last_error()


# ------------------------------------------------------------------------------------------------------------------ the model's call
def test_encode_scene_refuses_bad_scenes_and_strides():
    enc = make_encoder()
    for shape in ((50, 16, 16), (2, 40, 16, 16), (2, 50, 7, 16), (2, 50, 16, 7)):   # rank 3, wrong band count, smaller than a window
        with pytest.raises(ValueError):
            enc.encode_scene(torch.zeros(shape))
    for stride in (0, 9, 2.5, True, -1):
        with pytest.raises(ValueError, match="stride"):
            enc.encode_scene(torch.zeros(2, 50, 16, 16), stride=stride)
    for mw in (0, -3, 1.5, True):
        with pytest.raises(ValueError, match="max_windows"):
            enc.encode_scene(torch.zeros(2, 50, 16, 16), max_windows=mw)
    # a pixelwise model: None still means image_size (its strides 1 .. 7 are all accepted, 8 is not)
    pix = make_encoder(image_size=7, pixelwise=True)
    with pytest.raises(ValueError, match="stride"):
        pix.encode_scene(torch.zeros(1, 50, 9, 9), stride=8)


def test_encode_scene_has_no_cpu_fallback():
    enc = make_encoder()
    scene = torch.zeros(2, 50, 19, 21)
    enc.train()
    for kw in (dict(), dict(stride=3), dict(stride=8, normalize=True, max_windows=3)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            enc.encode_scene(scene, **kw)
    assert enc.training
    from maskedsst_amd import SimMIMSpatialSpectral
    model = SimMIMSpatialSpectral(encoder=make_encoder(), masking_ratio=0.7, mask_patch_size=4, tube_masking=True,
                                  to_pixels_per_spectral_block=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.encoder.encode_scene(scene)


# ------------------------------------------------------------------------------------------------------------------- scripts
def test_finetune_parser_takes_val_embed():
    import finetune
    ap = finetune.build_parser()
    assert ap.parse_args(["enmap"]).val_embed is False
    assert ap.parse_args(["enmap", "--val-scenes", "2", "--val-embed"]).val_embed is True


def test_product_still_does_not_import_oracle():
    code = ("import sys; sys.path.insert(0, %r); import maskedsst_amd, maskedsst_amd.engine, maskedsst_amd.scene; "
            "assert not any(m == 'oracle' or m.startswith('oracle.') for m in sys.modules), 'oracle imported'" % ROOT)
    subprocess.run([sys.executable, "-c", code], check=True)
    for f in ("scene.py", "vit_spatial_spectral.py", "engine.py", "_lib.py"):
        src = open(os.path.join(ROOT, "maskedsst_amd", f)).read()
        assert "import oracle" not in src and "from oracle" not in src, f
    assert "encode_scene" in open(os.path.join(ROOT, "maskedsst_amd", "scene.py")).read()
