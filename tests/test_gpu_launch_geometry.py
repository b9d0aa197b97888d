"""The block kernels with several tiles per workgroup, teacher-forced against float64.

Every block kernel is a persistent grid: a workgroup takes tile blockIdx.x, then blockIdx.x + gridDim.x, ... and the tuned kernels
overlap, prefetch and address by that walk (the next tile's rows, sequence bases and saved statistics a step ahead, a four-slot ring of
drawn tiles under the tile queue, one partial-gradient slab per workgroup).  The host clamps every grid to the tile count, and the
sweeps of tests/test_gpu_seq_lengths.py run a handful of tiles on grids of 64 .. 256: one tile per workgroup, the walk's loop body once,
no next tile.  This file runs the same comparison (same inputs with one offset per sequence, same float64 oracle, same bars) at shapes
of at least seven attention tiles and seven row tiles -- the last attention tile partly filled whenever a tile packs more than one
sequence -- with the grids forced through Engine.max_grid / attn_chunks / grid_rows (plain attributes the launch calls read):

  (g, g, g), g = 1, 2, 3   one workgroup walks a prologue, middle and epilogue tile (g = 2), unequal counts 3 / 2 / 2 (g = 3)
  (T_a - 1, T_a - 1, T_r - 1)   exactly one workgroup walks two tiles; its second one is the last, partly filled tile
  the engine's defaults    one tile per workgroup: the baseline

(The bf16 MLP half runs 2 * grid_rows workgroups: grid_rows = 1 still launches two of them, each with three or more tiles.)
The float64 reference is computed once per case; per geometry the kernels run once and are held against

  1. float64, on the bars of test_gpu_seq_lengths.py unchanged (BF16_BARS, FP32_BARS, LSE_BARS, 1e-5 for rstd),
  2. the default geometry, bit for bit: y, the saved x1 rows, the saved LN1 rows and the statistics (lse of every real row, the rstd
     tail).  Padding rows of the statistics are no tile's output -- what the kernel leaves there is not compared,
  3. the default geometry, bit for bit: dx (row-local; the d(LN1 out) partials are summed over heads in a fixed order),
  4. the default geometry: relative L2 over the block's concatenated parameter gradients < 1e-5 (the same sums in another order: the
     bar of test_gpu_boundary.py::test_cu_thief_probe_does_not_change_results); the worst tensor is recorded,
  5. the workspace bounds of include/msst.h: dx1, the d(LN1 out) partials, the bf16 da rows and the slabs are sized as msst_block_bwd
     documents for that (grid_rows, nchunk), each followed by 4096 sentinel floats that must survive; the slab itself starts as
     sentinels and must be written exactly up to the end of the layout the forced grid gives (MLP slabs of min(2 grid_rows, T_r)
     workgroups, attention slabs of min(nchunk, T_a) chunks x heads, LN1 slabs of min(grid_rows, T_r)) -- which is also the evidence
     that the forced grid was the one launched: the clamp did not turn it back into one tile per workgroup.

test_production_path runs blocks_fwd (msst_block_fwd_stack: (tile, block) steps) and blocks_bwd (msst_block_bwd_chain with the fused
LN1 + MLP launch and MSST_LN1_FROM_XN) of a depth-2 model at the same geometries against float64 autograd through all four blocks,
then the tile queue: at (1, 1, 1) one workgroup per head pair and one fused workgroup draw tiles 0, 1, 2, ... -- the static order -- so
dx0 and every gradient are bit-identical to the static run; at (2, 2, 2) and (3, 3, 3) the partition depends on timing (bars of
test_gpu_boundary.py::test_tile_queue_at_bench_batch against the static run at the same grid, plus the float64 bars).

Every error goes to util.record (launch_geometry_teacher_forced, launch_geometry_production).  The whole file runs in about 6 s on one
MI355X (5.7 s measured, 2.4 s of it the first test's library start; every other test 0.1 - 0.3 s).

Worst errors measured on MI355X (relative L2 for bf16, max-norm relative for fp32; increment / dx - dy / worst parameter gradient at the
default geometry | worst parameter gradient over the forced geometries).  The forward and dx are bit-identical at every geometry, so
only the gradient column can move, and it moves in the seventh digit:
  bf16, 8 heads              7.8e-4 (spatial 49)    1.31e-2 (spatial 49)   1.45e-2 (spectral 50)  | 1.45e-2 (spectral 50, all but one)
  bf16, 8 heads, dropout 0.1 8.2e-4 (spatial 49)    1.32e-2 (spatial 49)   1.43e-2 (spectral 50)  | 1.43e-2 (spectral 50, g = 1)
  bf16, 2 heads              5.8e-3 (spatial 25)    1.30e-2 (spatial 25)   1.13e-2 (spatial 25)   | 1.13e-2 (spatial 25, g = 2)
  bf16, 3 heads              5.9e-3 (spectral 22)   1.26e-2 (spatial 25)   1.23e-2 (spectral 22)  | 1.23e-2 (spectral 22, g = 2)
  fp32, 8 heads              1.0e-6 (spectral 22)   1.0e-6 (spectral 22)   1.5e-6 (spatial 25)    | 1.8e-6 (spatial 25, g = 1)
  fp32, 3 heads              9.9e-7 (spatial 25)    1.7e-6 (spectral 3)    1.2e-6 (spatial 25)    | 1.5e-6 (spatial 25, g = 1)
  production path, depth 2   1.68e-3 (spectral 22)  2.05e-2 (spatial 49)   2.39e-2 (spatial 9)    | 2.39e-2 (spatial 9; static and queue alike)
  saved statistics (bf16, 8 heads): lse 4.8e-3 absolute (spatial 1, peaky rows), rstd 1.5e-7 -- the same bits at every geometry
  gradients against the default geometry (bar 1e-5): concatenated 1.5e-7 (bf16), 4.6e-7 (fp32); worst single tensor 2.5e-7 / 5.5e-7
  tile queue at (2, 2, 2) and (3, 3, 3) against the static run: dx0 bit-identical in the measured runs, worst tensor 1.7e-7
Mutations this file catches, each applied alone to a scratch copy of the kernels (wrong but in-range tiles only).  With every one of
them all eleven tests report nothing at the default geometry -- one tile per workgroup cannot see them -- and fail at forced ones:
  msst_bwd.hip:553 request_rows(tile + gridDim.x - 1): the       all 11 tests, every forced geometry: dx - dy up to 9.4 against float64,
    MLP half requests wrong rows for its next tile                dx bits, gradients against the default geometry up to 1.4
  msst_bwd4.hip: fill_seqbase and dma_lse of the next tile        bf16 8 heads (both), 2 heads and the 5 production tests, every forced
    given the current tile                                        geometry: dx - dy up to 1.4, dx bits; the queue runs against the static ones
  msst_fwd3.hip copy_lse: statistics stored at the workgroup's    bf16 8 heads (both) and the 5 production tests, every forced geometry:
    first tile (blockIdx.x)                                       lse bits and bar (rows never written: up to 1e38), dx bits, dx - dy 6e-2
  msst_fwd3.hip: attention-dropout hash with the workgroup's      bf16 8 heads with dropout, every forced geometry: y and x1 bits,
    first tile                                                    increment 0.39, worst gradient 0.33
  msst_api.hip slab_layout: l.grid_mlp without the factor 2       the four bf16 block tests, every forced geometry: "slab of the forced grid
                                                                  not written" (the results stay right -- only the launch check sees it)
  msst_bwd5.hip: rstd of LN1 (MSST_LN1_FROM_XN) read at the       the 5 production tests: dx0 bits at every forced geometry, dx - dy 0.16
    workgroup's first tile                                        and worst gradient 0.20 at g = 1, 2, 3, static and queue
  msst_bwd.hip:420 (tokn from tok + (gridDim.x - 1) * 64)         NOT caught, and cannot be: that whole-tile prefetch (PREF) is compiled only
                                                                  with MSST_MLP2 = 0; the shipped MLP half requests its rows at line 553 (first row)
"""
from contextlib import contextmanager

import pytest
import torch

from util import oracle_cfg, rel_l2, record
from test_gpu_seq_lengths import (BF16_BARS, FP32_BARS, LSE_BARS, DROP, Q, case_cfg, tokens_with_offsets, make_model, block_prefix,
                                  block_inputs, block_reference, block_kernels, block_errors, check_saved_statistics)
from util import saved_lse_rows

pytestmark = pytest.mark.gpu

MIN_TILES = 7                              # grid 2: prologue, middle and epilogue tile; grid 3: 3 / 2 / 2; one drawer wraps the ring of four
SPECTRAL_ALL = [(1, L) for L in (1, 3, 20, 22, 33, 50, 64)]     # TS = 64, 21, 3, 2, 1, 1, 1 sequences per tile
SPATIAL_ALL = [(0, s * s) for s in (1, 3, 5, 7, 8)]
SOME = [(1, 3), (1, 22), (1, 64), (0, 25), (0, 64)]
DROP_CASES = [(1, 3), (1, 22), (1, 50), (0, 9), (0, 49)]
PRODUCTION_CASES = DROP_CASES
TAIL = 4096                                # sentinel floats behind every workspace buffer
SENTINEL = 0x7FC0DEAD                      # a quiet NaN no kernel computes
SNAME = {0: "spatial", 1: "spectral"}
MLP_SLAB, ATTN_SLAB, LN1_SLAB = 64 * 96 + 96 * 64 + 64 + 96 + 96 + 96, 3 * 64 * 96 + 96 * 64, 288    # include/msst.h

# family -> (precision, heads, dropout, saved statistics, bars, cases)
FAMILIES = {
    "bf16_h8": ("bf16", 8, None, True, BF16_BARS[8], SPECTRAL_ALL + SPATIAL_ALL),
    "bf16_h8_drop0.1": ("bf16", 8, DROP, True, BF16_BARS[8], DROP_CASES),
    "bf16_h2": ("bf16", 2, None, False, BF16_BARS["4wave"], SOME),
    "bf16_h3": ("bf16", 3, None, False, BF16_BARS["4wave"], SOME),
    "fp32_h8": ("fp32", 8, None, False, FP32_BARS, SOME),
    "fp32_h3": ("fp32", 3, None, False, FP32_BARS, SOME),
}


def geometry_cfg(mode, L, heads, depth=1):
    """the smallest batch with MIN_TILES attention tiles and MIN_TILES row tiles, the last attention tile partly filled where TS > 1"""
    cfg = case_cfg(mode, L, heads, min_tokens=0, min_tiles=MIN_TILES)
    cfg["depth"] = depth
    return cfg


def shape_of(cfg):
    """(B, S, N) of a case"""
    return cfg["B"], cfg["bands"] // cfg["spectral_patch"], cfg["image_size"] ** 2


def attn_tiles(mode, B, S, N):
    """64-row attention tiles of a block launch: 64 // L whole sequences each (restates msst_block_tiles)"""
    L, nseq = (N, B * S) if mode == 0 else (S, B * N)
    return -(-nseq // (64 // L))


def row_tiles(B, S, N):
    return -(-(B * S * N) // 64)


def geometries(T_a, T_r):
    """name -> (max_grid, attn_chunks, grid_rows); None: the engine's own value"""
    return {"default": None, "g1": (1, 1, 1), "g2": (2, 2, 2), "g3": (3, 3, 3), "all_but_one": (T_a - 1, T_a - 1, T_r - 1)}


def workspace_floats(grid_rows, nchunk, heads, ntok, bf16):
    """msst_block_bwd's caller-owned workspace as include/msst.h documents it, in 4-byte words: dx1 [tokens][96] f32; the d(LN1 out)
    partials heads * tokens * 96 elements (f32, or bf16 for the bf16 kernels); slab grid_rows * (2 MSST_MLP_SLAB + MSST_LN1_SLAB) +
    nchunk * heads * MSST_ATTN_SLAB floats; dab_ws [tokens][96] bf16 (bf16 kernels only)"""
    return dict(dx1=ntok * 96, part=heads * ntok * 96 // (2 if bf16 else 1),
                slab=grid_rows * (2 * MLP_SLAB + LN1_SLAB) + nchunk * heads * ATTN_SLAB, dab=ntok * 48 if bf16 else 0)


def slab_written(grid_rows, nchunk, heads, T_r, T_a, bf16):
    """floats of the slab one msst_block_bwd writes (slab_layout, msst_api.hip): one MLP slab per workgroup of the MLP half (bf16: two
    workgroups per CU), one attention slab per (chunk, head), one LN1 slab per row-wise workgroup -- every grid clamped to its tiles"""
    grid_mlp = min(2 * grid_rows if bf16 else grid_rows, T_r)
    return grid_mlp * MLP_SLAB + min(nchunk, T_a) * heads * ATTN_SLAB + min(grid_rows, T_r) * LN1_SLAB


def sentinel_workspace(grid_rows, nchunk, heads, ntok, bf16):
    """(dx1, part, slab, dab) of the documented sizes, each with TAIL sentinel words behind it; the slab all sentinels"""
    n = workspace_floats(grid_rows, nchunk, heads, ntok, bf16)
    bufs = {}
    for k, words in n.items():
        if k == "dab" and not bf16:
            bufs[k] = None
            continue
        t = torch.full((words + TAIL,), SENTINEL, dtype=torch.int32, device="cuda")
        if k != "slab":
            t[:words] = 0
        bufs[k] = t
    return n, bufs


def workspace_violations(n, bufs, written):
    bad = []
    for k, t in bufs.items():
        if t is not None and not bool((t[n[k]:] == SENTINEL).all()):
            bad.append(("tail overwritten", k))
    slab = bufs["slab"]
    if not bool((slab[:written] != SENTINEL).all()):
        bad.append(("slab of the forced grid not written", int((slab[:written] == SENTINEL).sum())))
    if not bool((slab[written:] == SENTINEL).all()):
        bad.append(("slab written past the forced grid's layout", int((slab[written:n["slab"]] != SENTINEL).sum())))
    return bad


def report(bad):
    """every violation on a line of its own (pytest shortens a long list)"""
    return "%d violations\n" % len(bad) + "\n".join(" ".join(str(v) for v in b) for b in bad)


@contextmanager
def forced(eng, geo, queue=False):
    """the engine's launch geometry for the calls inside; put back on the way out"""
    saved = (eng.max_grid, eng.attn_chunks, eng.grid_rows, eng.tile_queue)
    try:
        if geo is not None:
            eng.max_grid, eng.attn_chunks, eng.grid_rows = geo
        eng.tile_queue = queue
        eng._tpw.clear()     # tiles per workgroup, cached for the stack-launch decision, follow max_grid
        yield
    finally:
        eng.max_grid, eng.attn_chunks, eng.grid_rows, eng.tile_queue = saved
        eng._tpw.clear()


def assert_case_shape(eng, cfg, modes):
    """the properties the file exists for, from the library's own tiling: -> (T_a of modes[0], T_r)"""
    B, S, N = cfg["B"], eng.S, eng.N
    assert (S, N) == shape_of(cfg)[1:]
    T_r = row_tiles(B, S, N)
    assert T_r >= MIN_TILES, (cfg, T_r)
    T = []
    for mode in modes:
        T_a = int(eng.lib.msst_block_tiles(mode, B, S, N))
        assert T_a == attn_tiles(mode, B, S, N) and T_a >= MIN_TILES, (cfg, mode, T_a)
        T.append(T_a)
    L, nseq = (N, B * S) if modes[0] == 0 else (S, B * N)
    assert 64 // L == 1 or nseq % (64 // L), (cfg, "the last attention tile is full")
    return T[0], T_r


def assert_forced(eng, geo, tiles, T_r, B):
    """a forced grid below the tile counts is launched as given (every clamp is min(grid, tiles), and at most the CU count).
    tiles: stack name -> attention tiles of the stacks the geometry is meant for"""
    mg, ac, gr = geo
    assert 1 <= gr < T_r and mg <= eng._cu_count(), (geo, T_r)
    for sname, T in tiles.items():
        assert 1 <= mg < T and 1 <= ac < T, (geo, sname, T)
        assert eng._tiles_per_workgroup(sname, B) == -(-T // mg) > 1


def run_case(family, mode, L):
    """one (family, case): the reference once, the kernels at every geometry -> list of violations"""
    prec, heads, drop, stats, bars, _ = FAMILIES[family]
    bf = prec == "bf16"
    cfg = geometry_cfg(mode, L, heads)
    model, params, eng = make_model(cfg, prec)
    i = 0 if mode == 0 else 1
    B, S, N = cfg["B"], eng.S, eng.N
    T_a, T_r = assert_case_shape(eng, cfg, [mode])
    x, dy = block_inputs(cfg, S, N, i)
    ref = block_reference(params, cfg, S, N, i, x, dy, drop=drop)
    xc, dyc = x.cuda(), dy.cuda().contiguous()
    pre = block_prefix(i)
    flat = {id(p): n for n, p in eng.trainable()}
    names = [flat[id(p)] for pn, p in model.named_parameters() if pn.startswith(pre)]
    bad, base = [], None
    for gname, geo in geometries(T_a, T_r).items():
        if geo is None:    # one tile per workgroup whatever the device: its own values, raised to the tile counts if need be
            run_geo = (0, max(eng.attn_chunks, T_a), max(eng.grid_rows, T_r))
        else:
            run_geo = geo
        with forced(eng, run_geo):
            if geo is not None:
                assert_forced(eng, geo, {SNAME[mode]: T_a}, T_r, B)
            n, bufs = sentinel_workspace(eng.grid_rows, eng.attn_chunks, heads, B * S * N, bf)
            y, x1, dx = block_kernels(eng, cfg, i, prec, xc, dyc, drop=drop, ws=(bufs["dx1"], bufs["part"], bufs["slab"], bufs["dab"]))
            bad += [(gname,) + v for v in workspace_violations(n, bufs, slab_written(eng.grid_rows, eng.attn_chunks, heads, T_r, T_a, bf))]
            r = block_errors(model, eng, i, prec, x, dy, ref, y, dx)
            if stats:
                r["lse_abs_err"], r["rstd_err"] = check_saved_statistics(eng, params, xc, x1, i, mode, B, S, N, cfg["qkv_scale"])
        got = dict(y=y, x1=x1, xn=x1._msst_xn, dx=dx, grad=eng.fp.grad.clone())
        if x1._msst_lse is not None:
            got["lse"], got["rstd"] = saved_lse_rows(x1._msst_lse, heads, N if mode == 0 else S, B * S if mode == 0 else B * N)
        # 1. against float64
        for q in Q:
            if not r[q] < bars[q]:
                bad.append((gname, "bar", q, r[q], bars[q]))
        if stats:
            if not r["lse_abs_err"] < LSE_BARS[cfg["qkv_scale"]]:
                bad.append((gname, "bar", "lse_abs_err", r["lse_abs_err"], LSE_BARS[cfg["qkv_scale"]]))
            if not r["rstd_err"] < 1e-5:
                bad.append((gname, "bar", "rstd_err", r["rstd_err"], 1e-5))
        if base is None:
            base = got
        else:
            # 2., 3. forward outputs, saved rows, statistics and dx: the bits of the default geometry
            for k in ("y", "x1", "xn", "lse", "rstd", "dx"):
                if got.get(k) is not None and not torch.equal(got[k], base[k]):
                    bad.append((gname, "bits differ from the default geometry", k, float((got[k].float() - base[k].float()).abs().max())))
            # 4. parameter gradients: the same sums in another order
            cat = lambda g: torch.cat([eng.fp.view(nm, g).reshape(-1) for nm in names])
            r["grad_vs_default"] = rel_l2(cat(got["grad"]), cat(base["grad"]))
            r["worst_tensor_vs_default"] = max(rel_l2(eng.fp.view(nm, got["grad"]), eng.fp.view(nm, base["grad"])) for nm in names)
            if not r["grad_vs_default"] < 1e-5:
                bad.append((gname, "gradients against the default geometry", r["grad_vs_default"], r["worst_tensor_vs_default"]))
        print(family, SNAME[mode], L, gname, run_geo, r)
        record("launch_geometry_teacher_forced", family=family, mode=mode, L=L, geometry=gname, cfg=cfg, **r)
    return bad


@pytest.mark.parametrize("family", list(FAMILIES))
def test_blocks_at_forced_geometries(family):
    """one block forward (_fwd_block) and backward (block_bwd_single) per case and geometry: the five assertions of the module
    docstring.  bf16_h8: role-split forward with saved statistics + two-head backward on them, every case; with dropout 0.1 the
    (tile, head, row, key) hash of the attention mask; 2 / 3 heads: 4-wave forward, two-head / one-head backward; fp32: the templates"""
    bad = []
    for mode, L in FAMILIES[family][5]:
        b = run_case(family, mode, L)
        bad += [(SNAME[mode], L) + v for v in b]
    assert not bad, report(bad)


def production_run(eng, x0c, dyc, monkeypatch):
    """blocks_fwd (both stacks through msst_block_fwd_stack) + blocks_bwd (chained, LN1 from the saved rows) -> (y, dx0, gradients)"""
    stacked = []
    real_stack = eng._fwd_stack
    eng._fwd_stack = lambda *a: stacked.append(real_stack(*a)) or stacked[-1]
    monkeypatch.setenv("MSST_FWD_STACK", "1")
    try:
        acts, x1s = eng.blocks_fwd(x0c, save=True)
    finally:
        monkeypatch.delenv("MSST_FWD_STACK")
        del eng._fwd_stack
    assert stacked == [True, True], stacked          # both stacks walked (tile, block) steps in one launch each
    eng.fp.grad.zero_()
    dx0 = eng.blocks_bwd(acts, x1s, dyc.clone())
    torch.cuda.synchronize()
    assert eng.last_bwd_ln1_from_xn                  # ... and the backward was the chained one with the fused LN1 + MLP launch
    return acts[-1], dx0, eng.fp.grad.clone()


@pytest.mark.parametrize("mode,L", PRODUCTION_CASES, ids=[f"{SNAME[m]}-{L}" for m, L in PRODUCTION_CASES])
def test_production_path(mode, L, monkeypatch):
    """the forward / backward pair bench.py times on a depth-2 model (two spatial and two spectral blocks) at the forced geometries,
    static partition and tile queue (module docstring)"""
    from oracle import transformer_forward
    cfg = geometry_cfg(mode, L, 8, depth=2)
    model, params, eng = make_model(cfg, "bf16")
    B, S, N = cfg["B"], eng.S, eng.N
    T_a, T_r = assert_case_shape(eng, cfg, [mode, 1 - mode])
    T_as = [int(eng.lib.msst_block_tiles(m, B, S, N)) for m in (0, 1)]
    x0 = tokens_with_offsets(B, S, N, None, seed=3000 + L)
    dy = torch.randn(x0.shape, generator=torch.Generator().manual_seed(4000 + L))
    p64 = {k: v.double().requires_grad_(True) for k, v in params.items() if "spatial_spectral_transformer" in k}
    xs = x0.double().requires_grad_(True)
    y64 = transformer_forward(p64, xs, oracle_cfg(cfg))
    y64.backward(dy.double())
    inc_ref, dxi_ref = y64.detach() - x0.double(), xs.grad - dy.double()
    flat = {id(p): n for n, p in eng.trainable()}
    names = {pn: flat[id(p)] for pn, p in model.named_parameters() if pn in p64}
    x0c, dyc = x0.cuda(), dy.cuda()
    bars = BF16_BARS["production"]
    bad, runs = [], {}

    def against_float64(tag, y, dx0, g):
        ge = {pn: rel_l2(eng.fp.view(nm, g), p64[pn].grad) for pn, nm in names.items()}
        worst = max(ge, key=ge.get)
        r = dict(inc_err=rel_l2(y.double().cpu() - x0.double(), inc_ref), dx=rel_l2(dx0.double().cpu() - dy.double(), dxi_ref),
                 worst_grad=ge[worst], worst_grad_name=worst)
        for q in Q:
            if not r[q] < bars[q]:
                bad.append((tag, "bar", q, r[q], bars[q]))
        return r

    def worst_tensor(g, g_ref):
        return max(rel_l2(eng.fp.view(nm, g), eng.fp.view(nm, g_ref)) for nm in names.values())

    for gname, geo in geometries(T_a, T_r).items():
        if geo is None:
            run_geo = (0, max(eng.attn_chunks, max(T_as)), max(eng.grid_rows, T_r))
        else:
            run_geo = geo
        with forced(eng, run_geo):
            if geo is not None:
                both = gname != "all_but_one"     # (sized for the named stack: the other one may have fewer tiles than that)
                assert_forced(eng, geo, {SNAME[m]: T_as[m] for m in (0, 1) if both or m == mode}, T_r, B)
            y, dx0, g = runs[gname] = production_run(eng, x0c, dyc, monkeypatch)
        r = against_float64(gname, y, dx0, g)
        if gname != "default":
            by, bdx, bg = runs["default"]
            if not torch.equal(y, by):
                bad.append((gname, "stack forward: bits differ from the default geometry"))
            if not torch.equal(dx0, bdx):
                bad.append((gname, "dx0: bits differ from the default geometry", rel_l2(dx0, bdx)))
            cat = lambda t: torch.cat([eng.fp.view(nm, t).reshape(-1) for nm in names.values()])
            r["grad_vs_default"], r["worst_tensor_vs_default"] = rel_l2(cat(g), cat(bg)), worst_tensor(g, bg)
            if not r["grad_vs_default"] < 1e-5:
                bad.append((gname, "gradients against the default geometry", r["grad_vs_default"], r["worst_tensor_vs_default"]))
        print("production", SNAME[mode], L, gname, run_geo, r)
        record("launch_geometry_production", mode=mode, L=L, geometry=gname, queue=False, cfg=cfg, **r)
    # the tile queue: the backward's persistent grids draw their tiles
    for gname in ("g1", "g2", "g3"):
        with forced(eng, geometries(T_a, T_r)[gname], queue=True):
            y, dx0, g = production_run(eng, x0c, dyc, monkeypatch)
        r = against_float64(gname + "_queue", y, dx0, g)
        _, sdx, sg = runs[gname]
        if gname == "g1":     # one drawer per counter: tiles 0, 1, 2, ... -- the static order at that grid
            if not (torch.equal(dx0, sdx) and torch.equal(g, sg)):
                bad.append((gname, "queue with one workgroup: bits differ from the static run", rel_l2(dx0, sdx), worst_tensor(g, sg)))
        else:
            r["input_grad_vs_static"], r["worst_tensor_vs_static"] = rel_l2(dx0, sdx), worst_tensor(g, sg)
            if not (bool(torch.isfinite(dx0).all()) and bool(torch.isfinite(g).all()) and r["input_grad_vs_static"] < 5e-4
                    and r["worst_tensor_vs_static"] < 3.2e-3):
                bad.append((gname, "queue against the static run", r["input_grad_vs_static"], r["worst_tensor_vs_static"]))
        print("production", SNAME[mode], L, gname + "_queue", r)
        record("launch_geometry_production", mode=mode, L=L, geometry=gname, queue=True, cfg=cfg, **r)
    assert not bad, report(bad)
