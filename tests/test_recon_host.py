"""SimMIM reconstruction, host side (no GPU needed): the C ABI of msst_recon_fwd (additive under MSST_VERSION 109), its argument checks
(they run before any HIP call, so host buffers and no device are enough to see them), and the Python surface: reconstruct has no CPU
fallback and checks its shapes first, recon_report is host arithmetic on the [B, C] tables, pretrain.py takes --recon-report."""
import ctypes
import math
import re
import subprocess
from collections import namedtuple

import pytest
import torch

from util import build_product

BADARG, UNSUPPORTED = -3, -2   # include/msst.h: MSST_ERR_BADARG, MSST_ERR_UNSUPPORTED


def test_c_abi_declares_and_exports_recon_fwd():
    from maskedsst_amd import _lib
    header = open(_lib.HEADER_PATH).read()
    assert re.search(r"^int msst_recon_fwd\(", header, re.M)
    assert _lib.header_version() == 109   # additive: the revision does not move
    lib = _lib.load()                      # refuses a library that lacks a declared symbol
    assert lib.msst_version() == _lib.header_version() == 109
    assert "msst_recon_fwd" in _lib.declared_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T msst_recon_fwd$", out, re.M)
    names = [lib.msst_profile_name(i).decode() for i in range(lib.msst_profile_kernels())]
    assert "recon_fwd" in names and "?" not in names


def test_recon_fwd_refuses_bad_arguments_before_launch():
    from maskedsst_amd import _lib
    lib = _lib.load()
    # host memory stands in for the device buffers: a refused call dereferences nothing and launches nothing
    buf = (ctypes.c_char * 64)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)   # 16-byte aligned, as y must be
    names = ["y", "img", "mask", "w_pix", "b_pix", "recon", "band_err", "band_cnt"]

    def call(B=2, S=3, N=4, P=5, **null):
        a = {k: (None if null.get(k) else p) for k in names}
        return lib.msst_recon_fwd(a["y"], a["img"], a["mask"], a["w_pix"], a["b_pix"], 1, 1, a["recon"], a["band_err"], a["band_cnt"],
                                  B, S, N, P, None)

    for dim in ("B", "S", "N", "P"):
        for v in (0, -1):
            assert call(**{dim: v}) == BADARG, (dim, v)
    assert b"msst_recon_fwd" in lib.msst_last_error()
    for k in ("y", "img", "mask", "w_pix", "b_pix", "recon"):
        assert call(**{k: True}) == BADARG, k
    assert call(band_err=True) == BADARG and call(band_cnt=True) == BADARG   # statistics: both or neither
    # beyond the constructor's limits -- decided by the sizes alone, before any pointer is looked at
    all_null = {k: True for k in names}
    for over in (dict(N=65), dict(S=65), dict(P=17)):
        assert call(**over) == UNSUPPORTED and call(**over, **all_null) == UNSUPPORTED, over
    assert call(N=64, S=64, P=16, **all_null) == BADARG        # the limits themselves are inside
    assert call(N=65, P=0) == BADARG                            # a size below 1 wins over a size beyond the kernel
    y_odd = ctypes.c_void_p(p.value + 4)
    assert lib.msst_recon_fwd(y_odd, p, p, p, p, 1, 1, p, p, p, 2, 3, 4, 5, None) == BADARG   # y is read as 16-byte pieces
    assert b"aligned" in lib.msst_last_error()


CFG = dict(bands=20, depth=1, B=2, heads=2)


def test_reconstruct_checks_shapes_then_refuses_the_cpu():
    model, _, x = build_product(CFG)
    T = model.encoder.num_patches
    masks = model.draw_masks(2)
    for bad in (x[0], x[:, :10], x[:, :, :4], x[:, :, :, :4], torch.randn(2, 30, 8, 8), x[:0]):
        with pytest.raises(ValueError):
            model.reconstruct(bad, masks)
    for bad in (masks[0][:1], masks[0][:, :-1], masks[0].float(), (masks[0].t(), masks[1]), torch.zeros(2, T + 1, dtype=torch.bool)):
        with pytest.raises(ValueError):
            model.reconstruct(x, bad)
    model.train()
    for ok in (masks, masks[0], None):   # the pair forward takes, a bare bool [B, T] tensor, or drawn here
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            model.reconstruct(x, ok)
    assert model.training and model.last_masks is not None and model.last_masks[0].shape == (2, T)
    from maskedsst_amd.engine import recon_fwd
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        recon_fwd(torch.zeros(1, 4, 96), torch.zeros(1, 6, 2), torch.zeros(1, 4, dtype=torch.uint8), torch.zeros(1, 3, 96),
                  torch.zeros(1, 3), 0, True, 2, 2, 3)


def test_recon_report_against_a_hand_computed_table():
    from maskedsst_amd import recon_report, ReconReport
    Rec = namedtuple("Rec", "band_err band_cnt")
    # 2 samples x 4 bands (two spectral blocks of 2 bands); band 2 has no masked pixel in either sample
    rec = Rec(torch.tensor([[1.0, 2.0, 0.0, 4.0], [3.0, 0.0, 0.0, 4.0]], dtype=torch.float64),
              torch.tensor([[2, 4, 0, 1], [2, 0, 0, 3]], dtype=torch.int32))
    r = recon_report(rec, pixels_per_patch=2)
    assert isinstance(r, ReconReport) and r.masked == 12
    assert r.mae == 14.0 / 12.0
    assert r.band_mae.dtype == torch.float64
    assert r.band_mae[[0, 1, 3]].tolist() == [4.0 / 4.0, 2.0 / 4.0, 8.0 / 4.0] and math.isnan(float(r.band_mae[2]))
    assert r.band_present.tolist() == [True, True, False, True]
    assert r.worst_bands == [3, 0, 1]                  # worst first, the absent band left out
    assert r.block_mae.tolist() == [6.0 / 8.0, 8.0 / 4.0]
    r1 = recon_report(rec)                              # no block size given: no block table
    assert r1.block_mae is None and r1.mae == r.mae and torch.equal(r1.band_present, r.band_present)
    # nothing masked anywhere: every rate is absent, nothing divides by zero
    r0 = recon_report(Rec(torch.zeros(2, 4, dtype=torch.float64), torch.zeros(2, 4, dtype=torch.int32)), 4)
    assert math.isnan(r0.mae) and r0.worst_bands == [] and r0.masked == 0 and not r0.band_present.any()
    assert torch.isnan(r0.band_mae).all() and torch.isnan(r0.block_mae).all()
    with pytest.raises(ValueError):
        recon_report(rec, pixels_per_patch=3)
    with pytest.raises(ValueError):
        recon_report(Rec(torch.zeros(2, 4), torch.zeros(2, 3)))


def test_pretrain_parser_takes_recon_report():
    import pretrain
    ap = pretrain.build_parser()
    assert ap.parse_args([]).recon_report is False
    assert ap.parse_args(["--recon-report"]).recon_report is True
