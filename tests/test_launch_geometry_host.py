"""Host side of tests/test_gpu_launch_geometry.py (no GPU needed): the batch picker's tile counts over every case of that file, against
the library's own tiling, and the workspace sizes it hands msst_block_bwd against include/msst.h and the layout the library uses."""
import os
import re

from conftest import ROOT
import test_gpu_launch_geometry as lg
import test_gpu_seq_lengths as sl


def all_cases():
    for family, (prec, heads, _, _, _, cases) in lg.FAMILIES.items():
        for mode, L in cases:
            yield family, mode, L, heads, 1
    for mode, L in lg.PRODUCTION_CASES:
        yield "production", mode, L, 8, 2


def test_case_lists_are_the_ones_named():
    """spectral 1, 3, 20, 22, 33, 50, 64 pack 64, 21, 3, 2, 1, 1, 1 sequences per tile; spatial sides 1, 3, 5, 7, 8"""
    assert [L for _, L in lg.SPECTRAL_ALL] == [1, 3, 20, 22, 33, 50, 64] and [64 // L for _, L in lg.SPECTRAL_ALL] == [64, 21, 3, 2, 1, 1, 1]
    assert [L for _, L in lg.SPATIAL_ALL] == [1, 9, 25, 49, 64] and sl.SPATIAL_S == 5
    assert lg.FAMILIES["bf16_h8"][5] == lg.SPECTRAL_ALL + lg.SPATIAL_ALL
    assert lg.FAMILIES["bf16_h8_drop0.1"][5] == [(1, 3), (1, 22), (1, 50), (0, 9), (0, 49)] == lg.PRODUCTION_CASES
    for f in ("bf16_h2", "bf16_h3", "fp32_h8", "fp32_h3"):
        assert lg.FAMILIES[f][5] == [(1, 3), (1, 22), (1, 64), (0, 25), (0, 64)]


def test_batches_give_seven_tiles_and_a_partly_filled_last_one():
    """every case: T_a >= 7 attention tiles (the library's count), T_r >= 7 row tiles, the last attention tile partly filled where a
    tile packs more than one sequence, no smaller batch with these properties, a few thousand tokens at most; a production case
    has seven attention tiles in its other stack too"""
    from maskedsst_amd import _lib
    lib = _lib.load()
    for family, mode, L, heads, depth in all_cases():
        cfg = lg.geometry_cfg(mode, L, heads, depth)
        B, S, N = lg.shape_of(cfg)
        assert (N if mode == 0 else S) == L and cfg["depth"] == depth and cfg["heads"] == heads
        assert cfg["qkv_scale"] == (sl.qkv_scale_of(L) if mode == 1 else (4 if int(round(L ** 0.5)) % 2 else 1))

        def ok(b):
            nseq, TS = (b * S if mode == 0 else b * N), 64 // L
            return (lib.msst_block_tiles(mode, b, S, N) >= lg.MIN_TILES and lg.row_tiles(b, S, N) >= lg.MIN_TILES
                    and (TS == 1 or nseq % TS != 0))
        assert ok(B) and not any(ok(b) for b in range(1, B)), (family, mode, L, B)
        assert lib.msst_block_tiles(mode, B, S, N) == lg.attn_tiles(mode, B, S, N)
        assert B * S * N <= 4096, (family, mode, L, B * S * N)
        if depth == 2:
            assert lib.msst_block_tiles(1 - mode, B, S, N) == lg.attn_tiles(1 - mode, B, S, N) >= lg.MIN_TILES, (mode, L)


def test_default_batches_of_the_length_sweep_are_unchanged():
    """pick_B's defaults (two attention tiles, 256 tokens) choose what they chose before it learned a minimum tile count"""
    def before(per_b, L, tokens_per_b, partial=True, min_tokens=256):
        TS = 64 // L
        B = 1
        while not (B * per_b > TS and (not partial or TS == 1 or (B * per_b) % TS) and B * tokens_per_b >= min_tokens):
            B += 1
        return B
    for L in sl.SPECTRAL_L:
        for partial in (True, False):
            N = sl.spectral_cfg(L, 8, partial)["image_size"] ** 2
            assert sl.spectral_cfg(L, 8, partial)["B"] == before(N, L, L * N, partial)
    for side in sl.SIDES:
        assert sl.spatial_cfg(side, 8)["B"] == before(sl.SPATIAL_S, side * side, sl.SPATIAL_S * side * side)


def test_workspace_sizes_are_the_documented_ones():
    """the slab constants are include/msst.h's; at every case and geometry the layout the library uses (slab_layout: each grid clamped
    to its tiles) fits the size the header documents for msst_block_bwd, and the engine's own workspace is no smaller than that"""
    from maskedsst_amd import _lib
    text = open(os.path.join(ROOT, "include", "msst.h")).read()
    for name, val in (("MSST_MLP_SLAB", lg.MLP_SLAB), ("MSST_ATTN_SLAB", lg.ATTN_SLAB), ("MSST_LN1_SLAB", lg.LN1_SLAB)):
        expr = re.search(r"#define %s\s+(.+)" % name, text).group(1)
        assert re.fullmatch(r"[\d\s()*+]+", expr) and eval(expr) == val, (name, expr)
    assert (lg.MLP_SLAB, lg.ATTN_SLAB, lg.LN1_SLAB) == (_lib.MLP_SLAB, _lib.ATTN_SLAB, _lib.LN1_SLAB)
    assert "slab grid_rows*(2*MSST_MLP_SLAB + MSST_LN1_SLAB) + nchunk*heads*MSST_ATTN_SLAB" in text
    for family, mode, L, heads, depth in all_cases():
        if depth != 1:
            continue
        bf16 = lg.FAMILIES[family][0] == "bf16"
        B, S, N = lg.shape_of(lg.geometry_cfg(mode, L, heads))
        T_a, T_r = lg.attn_tiles(mode, B, S, N), lg.row_tiles(B, S, N)
        for gname, geo in lg.geometries(T_a, T_r).items():
            mg, ac, gr = geo if geo is not None else (0, 64, 256)
            n = lg.workspace_floats(gr, ac, heads, B * S * N, bf16)
            written = lg.slab_written(gr, ac, heads, T_r, T_a, bf16)
            assert 0 < written <= n["slab"], (family, mode, L, gname)
            assert n["slab"] <= gr * (3 * lg.MLP_SLAB + lg.LN1_SLAB) + ac * heads * lg.ATTN_SLAB      # Engine._bwd_workspace
            assert n["dx1"] == B * S * N * 96 and n["part"] * 4 == heads * B * S * N * 96 * (2 if bf16 else 4)
            if geo is not None:     # several tiles per workgroup in every launch of the backward
                assert gr < T_r and ac < T_a and mg < T_a
