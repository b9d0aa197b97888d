"""Default classifier head, host side (no GPU needed): the C ABI's argument checks of msst_cls_head_fwd / _bwd, and a model with more
than 32 classes (the backward kernel stages dlogits 32 classes at a time, so any class count is supported)."""
import pytest
import torch

from conftest import seed_all

BADARG, UNSUPPORTED = -3, -2   # include/msst.h: MSST_ERR_BADARG, MSST_ERR_UNSUPPORTED


def test_c_abi_refuses_bad_shapes_before_launch():
    """msst_cls_head_* check B, S, N, n_classes and their pointers before anything is launched: sizes below 1 and null pointers are
    bad arguments, N or S above 64 are beyond the kernels; n_classes has no upper limit"""
    from maskedsst_amd import _lib
    lib = _lib.load()
    for (B, S, N, nc), want in [((0, 20, 64, 8), BADARG), ((2, 0, 64, 8), BADARG), ((2, 20, 0, 8), BADARG), ((2, 20, 64, 0), BADARG),
                                ((-1, 20, 64, 8), BADARG), ((2, 20, 65, 8), UNSUPPORTED), ((2, 65, 64, 8), UNSUPPORTED),
                                ((2, 65, 65, 40), UNSUPPORTED)]:
        assert lib.msst_cls_head_fwd(*([None] * 6), B, S, N, nc, None) == want, (B, S, N, nc)
        assert lib.msst_cls_head_bwd(*([None] * 11), B, S, N, nc, None) == want, (B, S, N, nc)
    # shapes the kernels take, with null pointers: refused as bad arguments, not launched
    for B, S, N, nc in [(2, 20, 64, 8), (1, 64, 1, 40), (3, 1, 64, 97)]:
        assert lib.msst_cls_head_fwd(*([None] * 6), B, S, N, nc, None) == BADARG, (B, S, N, nc)
        assert lib.msst_cls_head_bwd(*([None] * 11), B, S, N, nc, None) == BADARG, (B, S, N, nc)


def test_default_head_with_40_classes_constructs():
    """num_classes = 40 with the default head: the reference's head shapes, and the flat parameters' first gradient bucket
    ("cls_head") holds exactly LayerNorm(96) + Linear(96 -> 40)"""
    from maskedsst_amd import ViTSpatialSpectral
    from maskedsst_amd.flat import FlatParams
    seed_all(5)
    enc = ViTSpatialSpectral(image_size=8, spatial_patch_size=1, spectral_patch_size=10, num_classes=40, dim=96, depth=1, heads=8,
                             mlp_dim=64, channels=50, spectral_pos_embed=False, spectral_pos=torch.arange(5))
    sd = enc.state_dict()
    assert sd["mlp_head.0.weight"].shape == (96,) and sd["mlp_head.1.weight"].shape == (40, 96) and sd["mlp_head.1.bias"].shape == (40,)
    fp = FlatParams(enc, None).flatten()
    name, start, end = fp.buckets[0][:3]
    assert name == "cls_head" and end - start == 96 * 2 + 40 * 96 + 40
    for k in ("pixelwise", "spectral_mlp_head"):   # the other two heads keep their 32-class limit
        with pytest.raises(NotImplementedError, match="num_classes=40"):
            ViTSpatialSpectral(image_size=7 if k == "pixelwise" else 8, spatial_patch_size=1, spectral_patch_size=10, num_classes=40,
                               dim=96, depth=1, heads=8, mlp_dim=64, channels=50, spectral_pos_embed=False,
                               spectral_pos=torch.arange(5), **{k: True})
