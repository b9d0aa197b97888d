"""Transformer blocks, host side (no GPU needed): the C ABI's shape checks of the five block entry points.  They run before the
pointer checks, before the tile map (which divides 64 by the sequence length) and before any HIP call, so every call here passes
null data pointers only: no call can reach a kernel launch, whatever the library does with the shape."""

BADARG, UNSUPPORTED = -3, -2   # include/msst.h: MSST_ERR_BADARG, MSST_ERR_UNSUPPORTED

# (mode, B, S, N, heads) -> the code every block entry point returns for it
BAD_SHAPES = [
    ((1, 2, 0, 4, 8), BADARG),        # S = 0: 64 / L divided by zero in spectral mode before the check existed
    ((0, 2, 5, 0, 8), BADARG),        # N = 0: the same in spatial mode
    ((1, 2, 5, 0, 8), BADARG),
    ((0, 0, 5, 4, 8), BADARG),
    ((1, -1, 5, 4, 8), BADARG),
    ((0, 2, 5, 4, 0), BADARG),
    ((1, 2, 5, 4, -2), BADARG),
    ((2, 2, 5, 4, 8), BADARG),        # mode outside {spatial, spectral}
    ((-1, 2, 5, 4, 8), BADARG),
    ((1, 2, 65, 4, 8), UNSUPPORTED),  # one sequence longer than a 64-row tile: 64 / L = 0 sequences per tile
    ((0, 2, 5, 65, 8), UNSUPPORTED),
    ((1, 2, 5, 65, 8), UNSUPPORTED),
    ((0, 2, 65, 65, 2), UNSUPPORTED),
    ((0, 0, 65, 4, 8), BADARG),       # a size below 1 wins over a length beyond the kernels
]


def _calls(lib, mode, B, S, N, heads):
    """every block entry point with this shape, null data pointers, and otherwise valid scalars"""
    return {
        "msst_block_fwd": lambda: lib.msst_block_fwd(None, None, None, None, mode, B, S, N, heads, 1, 0, 0.0, 0, 0, None, None, None, None),
        "msst_block_fwd_stack": lambda: lib.msst_block_fwd_stack(None, 2, None, None, None, None, None, mode, B, S, N, heads, 1, 0, 0.0, 0, 0,
                                                                 None, None),
        "msst_block_bwd": lambda: lib.msst_block_bwd(None, None, *([None] * 7), 1, 1, mode, B, S, N, heads, 1, 0.0, 0, 0, None, None, None,
                                                     None),
        "msst_block_bwd_chain": lambda: lib.msst_block_bwd_chain(None, None, None, None, *([None] * 8), 1, 1, mode, B, S, N, heads, 1, 0.0, 0,
                                                                 1, None, None, None, 1, None, None),
        "msst_block_bwd_reduce": lambda: lib.msst_block_bwd_reduce(None, None, None, 0, 0, 1, 0, 1, 1, 1, mode, B, S, N, heads, 1, None),
    }


def test_c_abi_refuses_bad_block_shapes_before_launch():
    """B, S, N or heads below 1 and a mode outside {0, 1} are bad arguments; S or N above 64 is beyond the kernels -- returned by
    msst_block_fwd, msst_block_fwd_stack, msst_block_bwd, msst_block_bwd_chain and msst_block_bwd_reduce before they look at a
    pointer.  (msst_block_bwd_reduce had no length check at all: S = 65 gave 0 sequences per tile and a division by zero.)"""
    from maskedsst_amd import _lib
    lib = _lib.load()
    for shape, want in BAD_SHAPES:
        for name, call in _calls(lib, *shape).items():
            assert call() == want, (name, shape, want)
    # shapes the kernels take, with null pointers: past the shape check, refused as bad arguments, nothing launched
    for shape in [(1, 2, 64, 4, 8), (1, 3, 1, 9, 8), (0, 2, 5, 64, 2), (0, 1, 7, 1, 16), (1, 5, 33, 9, 1)]:
        for name, call in _calls(lib, *shape).items():
            assert call() == BADARG, (name, shape)


def test_block_size_queries_refuse_bad_shapes():
    """Pins behaviour the library already had (this test passes on the parent too): msst_block_tiles / msst_block_lse_floats, with
    which callers size their buffers, answer 0 for the shapes above -- msst_block_tiles takes no head count, so it answers 0 exactly
    when B, S or N is below 1 or above 64 -- and count 64 // L whole sequences per tile for the shapes the kernels take."""
    from maskedsst_amd import _lib
    lib = _lib.load()
    for (mode, B, S, N, heads), _ in BAD_SHAPES:
        if mode not in (0, 1):
            continue
        shape_ok = min(B, S, N) >= 1 and max(S, N) <= 64
        L = N if mode == 0 else S
        want_tiles = -(-(B * (S if mode == 0 else N)) // (64 // L)) if shape_ok else 0
        assert lib.msst_block_tiles(mode, B, S, N) == want_tiles, (mode, B, S, N)
        assert lib.msst_block_lse_floats(mode, B, S, N, heads) == 0, (mode, B, S, N, heads)
    for S in range(1, 65):
        for N in (4, 9):
            B = 3
            TS = 64 // S
            assert lib.msst_block_tiles(1, B, S, N) == -(-(B * N) // TS), (S, N)
            assert lib.msst_block_lse_floats(1, B, S, N, 8) == -(-(B * N) // TS) * 8 * 64 + B * S * N, (S, N)
