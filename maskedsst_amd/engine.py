"""Host-side engine: owns the flat parameter buffers, the operand-layout weight copies and the
launch sequence of the HIP kernels (through the C-ABI in ``libmsst.so``) for one model.

PyTorch is used for device memory (``torch.empty``), streams and autograd bookkeeping only; all
arithmetic of the hot path runs in the kernels under ``maskedsst_amd/csrc``.
"""
import collections
import ctypes
import os

import numpy as np
import torch

from . import _lib
from ._lib import (MsstBlockWeights, MsstBlockGrads, MsstPrepJob, PREC_BF16, PREC_F32, MODE_SPATIAL,
                   MODE_SPECTRAL, MLP_SLAB, ATTN_SLAB, LN1_SLAB)
from .flat import FlatParams

D = 96
DH = 64
STACK_MAX_TILES = 12   # msst_block_fwd_stack is used for a stack whose workgroups hold at most this many tiles (crossover measured near 14; batch 256 at the EnMAP shape: 20 / 22)
MLP = 64
_MODE = {"spatial": MODE_SPATIAL, "spectral": MODE_SPECTRAL}   # stack name (Engine._layers) -> block mode

# The three classifier heads.  linear: index of the Linear in mlp_head (the LayerNorm is 0); shape(B, nc, N): the logits; fwd_ws /
# bwd_slab(lib, B, S, N, nc): floats of the forward workspace (None: the kernel takes none) and of the backward slab; assemble: the
# scene assembler that consumes this head's per-window logits.
_Head = collections.namedtuple("_Head", "fwd bwd linear shape fwd_ws bwd_slab assemble")
_HEADS = {
    # default: mean over the S tokens of a position -> LN(96) -> Linear; logits [B, nc, N]
    "cls": _Head("msst_cls_head_fwd", "msst_cls_head_bwd", 1, lambda B, nc, N: (B, nc, N), None,
                 lambda lib, B, S, N, nc: B * (nc * 97 + 192), "msst_scene_assemble"),
    # spectral_mlp_head: the S tokens of a position concatenated -> LN(96 S) -> Linear; logits [B, nc, N]
    "spec": _Head("msst_spec_head_fwd", "msst_spec_head_bwd", 1, lambda B, nc, N: (B, nc, N), None,
                  lambda lib, B, S, N, nc: lib.msst_spec_head_bwd_slab(B, S, N, nc), "msst_scene_assemble"),
    # pixelwise: mean over the S tokens -> LN(96) per position -> flatten -> Linear(96 N); logits [B, nc] (centre pixel)
    "pix": _Head("msst_pix_head_fwd", "msst_pix_head_bwd", 2, lambda B, nc, N: (B, nc),
                 lambda lib, B, S, N, nc: lib.msst_pix_head_fwd_ws(B, N),
                 lambda lib, B, S, N, nc: lib.msst_pix_head_bwd_slab(B, S, N, nc), "msst_scene_centre_assemble"),
}


class Windows:
    """Where the samples of a tokenizer or head call lie -- the one thing the Engine methods, the autograd Functions and the C entry
    points below them are told about it.  kind:
      batch   img [B, C, s, s]: the samples themselves (what a bare tensor means wherever a source is taken);
      tiles   img [B, C, Ht, Wt]: its non-overlapping s x s windows in the reference's stack_image_batch order (src/utils.py:451-474:
              tile, window row, window column; trailing Ht % s rows / Wt % s columns dropped) -- grid = (nr, nq) per tile;
      listed  img [Bs, C, Hs, Ws] and origins int32 [n, 3] = (scene, y0, x0) on its device; csr = scene.origins_csr(origins, ...) opts
              into the scenes' gradient (the windows overlap: it is a fold over that index), sink a SceneGradSink that receives it.
              orient uint8 [n] on its device: window i is read in orientation orient[i] (scene.orient_windows; the _orient entry
              points) -- everything downstream sees the oriented window; no scene gradient through it.
    img is held contiguous and fp32; n: the number of windows."""

    def __init__(self, kind, img, origins=None, csr=None, sink=None, s=None, orient=None):
        self.kind, self.img, self.origins, self.csr, self.sink = kind, img.contiguous().float(), origins, csr, sink
        self.orient = orient
        if orient is not None and (kind != "listed" or csr is not None or sink is not None):
            raise NotImplementedError("orient goes with listed windows only, and without the scenes' gradient")
        if kind == "tiles":
            self.grid = (img.shape[-2] // s, img.shape[-1] // s)
            self.n = img.shape[0] * self.grid[0] * self.grid[1]
        else:
            self.n = origins.shape[0] if kind == "listed" else img.shape[0]


# (kind, token mask given?) -> entry point of Engine.tokenize / tokenize_bwd / tokenize_input_bwd; no key, no entry point
_TOK_FWD = {("batch", False): "msst_tokenize_fwd", ("batch", True): "msst_tokenize_fwd", ("tiles", False): "msst_tokenize_scene_fwd_train",
            ("listed", False): "msst_tokenize_at_fwd", ("listed", True): "msst_tokenize_at_fwd_masked"}
_TOK_BWD = {("batch", False): "msst_tokenize_bwd", ("batch", True): "msst_tokenize_bwd", ("tiles", False): "msst_tokenize_scene_bwd",
            ("listed", False): "msst_tokenize_at_bwd", ("listed", True): "msst_tokenize_at_bwd_masked"}
_TOK_INPUT_BWD = {("batch", False): "msst_tokenize_bwd_input", ("batch", True): "msst_tokenize_bwd_input",
                  ("tiles", False): "msst_tokenize_scene_bwd_input", ("listed", False): "msst_tokenize_at_bwd_input"}


def _tok_entry(table, method, src, masked, emb_drop=(0.0, 0)):
    """(entry point, its dropout arguments) of `method` on src; the masked listed entry points take no embedding dropout; oriented
    listed windows run their namesake's _orient entry point (the forward and the parameter backward have one)"""
    name = table.get((src.kind, masked))
    if name is not None and src.orient is not None:
        name = name + "_orient" if table is not _TOK_INPUT_BWD else None
    if name is None:
        raise NotImplementedError(f"{method}: no entry point for {'oriented ' if src.orient is not None else ''}{src.kind} windows "
                                  f"{'with' if masked else 'without'} a token mask")
    if masked and src.kind == "listed":
        if emb_drop[0] > 0:
            raise NotImplementedError(f"{method}: no entry point for listed windows with a token mask and embedding dropout")
        return name, ()
    return name, tuple(emb_drop)


def _prec_of(name):
    name = (name or os.environ.get("MSST_PRECISION", "bf16")).lower()
    if name in ("fp32", "f32", "32-true", "float32"):
        return PREC_F32
    if name in ("bf16", "bf16-mixed", "bfloat16"):
        return PREC_BF16
    raise ValueError(f"unknown precision {name!r} (use 'bf16' or 'fp32')")


def _kernel_flags():
    """MSST_KERNEL_* selection flags (include/msst.h), read from the environment on the HOST side per call: the
    library itself never reads the environment.  MSST_DBG=16 selects the generic template kernels, 64 the 4-wave
    forward, 128 the one-head attention backward; 0 (default) the tuned kernels.  Only those selection bits pass (plus 8 and
    the wave-select bits 0x300 of the -DMSST_STAMPS kernel-study builds): MSST_X1_BF16 / MSST_BWD_DEFER_REDUCE share the
    field and are set by the engine's own logic, never from the environment."""
    v = int(os.environ.get("MSST_DBG", "0"))
    allowed = 16 | 64 | 128
    if v & 8:
        allowed |= 8 | 0x300
    return (v & allowed) << 8


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def recon_fwd(y, img, mask_u8, w_pix, b_pix, per_block, blend, S, N, P, stats=True, lib=None):
    """msst_recon_fwd (include/msst.h) on tensors: y [B, S N, 96] fp32, img with B S P N elements in the cube layout [B, S P, N]
    (a [B, C, H, W] cube as it lies), mask_u8 [B, S N] uint8, w_pix / b_pix the to_pixels tables ([S or 1, P, 96] / [S or 1, P]
    tensors, or device pointers) -> (recon [B, S P, N], band_err [B, S P] float64, band_cnt [B, S P] int32); stats=False: null
    statistics pointers, (recon, None, None).  The current stream."""
    lib = lib or _lib.load()
    for t in (y, img, mask_u8):
        if not t.is_cuda:
            raise RuntimeError("maskedsst_amd runs on an MI355X only (tensor is on %s); there is no CPU fallback" % t.device)
    B = y.shape[0]
    if (y.dtype, img.dtype, mask_u8.dtype) != (torch.float32, torch.float32, torch.uint8):
        raise ValueError("recon_fwd takes fp32 y and img and a uint8 mask")
    if tuple(y.shape) != (B, S * N, D) or img.numel() != B * S * P * N or mask_u8.numel() != B * S * N:
        raise ValueError(f"recon_fwd: y {tuple(y.shape)}, img {tuple(img.shape)}, mask {tuple(mask_u8.shape)} do not fit "
                         f"B = {B}, S = {S}, N = {N}, P = {P}")
    y, img, mask_u8 = y.contiguous(), img.contiguous(), mask_u8.contiguous()
    tables = []
    for t, n in ((w_pix, P * D), (b_pix, P)):
        if torch.is_tensor(t):
            if not t.is_cuda or t.dtype != torch.float32 or t.numel() != (S if per_block else 1) * n:
                raise ValueError("recon_fwd: to_pixels tables must be fp32 cuda tensors [S or 1, P, 96] and [S or 1, P]")
            t = t.contiguous()
        tables.append(t)
    recon = torch.empty(B, S * P, N, dtype=torch.float32, device=y.device)
    err = torch.empty(B, S * P, dtype=torch.float64, device=y.device) if stats else None
    cnt = torch.empty(B, S * P, dtype=torch.int32, device=y.device) if stats else None
    wp, bp = (_p(t) if torch.is_tensor(t) else t for t in tables)
    _lib.check(lib.msst_recon_fwd(_p(y), _p(img), _p(mask_u8), wp, bp, int(bool(per_block)), int(bool(blend)), _p(recon), _p(err),
                                  _p(cnt), B, S, N, P, _stream()), "msst_recon_fwd")
    return recon, err, cnt


class Engine:
    def __init__(self, encoder, mim):
        self.enc = encoder
        self.mim = mim
        self.lib = _lib.load()
        self.fp = FlatParams(encoder, mim)
        self.prec = _prec_of(getattr(encoder, "precision", None))
        self.max_grid = int(os.environ.get("MSST_MAX_GRID", "0"))
        # persistent grids of the backward: one row-wise workgroup per CU; tile chunks of the attention backward so that its
        # (chunks x heads or head pairs) grid fills every CU slot exactly once (64 x 4 two-head workgroups on 256 CUs)
        self.grid_rows = int(os.environ.get("MSST_BWD_GRID", "0")) or (self._cu_count() if torch.cuda.is_available() else 256)
        self.attn_chunks = int(os.environ.get("MSST_ATTN_CHUNKS", "0")) or \
            (self.default_attn_chunks() if torch.cuda.is_available() else 64)
        self.tok_chunks = int(os.environ.get("MSST_TOK_CHUNKS", "64"))
        self.bucket_hook = None  # callable(bucket_name, start, end) fired when a gradient bucket is complete
        self.tile_queue = False  # data parallel: the backward's persistent grids draw tiles from a queue (no static partition)
        self._tpw = {}   # (mode, batch) -> tiles per workgroup of a block forward
        self._wbuf = None
        self._jobs = None
        self._bw = None
        self._zero_mask = None

    # ------------------------------------------------------------------ setup
    @property
    def S(self):
        return self.enc.num_spectral_patches

    @property
    def N(self):
        return self.enc.num_spatial_patches

    @property
    def P(self):
        return self.enc.pixels_per_patch

    def _cu_count(self):
        try:
            return int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)
        except Exception:
            return 256

    def _attn_wgs_per_chunk_and_cu(self):
        """(workgroups per tile chunk, workgroups per CU) of the bf16 attention backward this engine selects: the two-head
        kernel (even head count) launches H/2 workgroups of 512 threads per chunk, one per CU (156 KB of LDS); the one-head
        kernels H workgroups of 256 threads, two per CU."""
        H = max(1, int(self.enc.heads))
        return (H // 2, 1) if H % 2 == 0 else (H, 2)

    def default_attn_chunks(self, free_cus=0):
        per_chunk, per_cu = self._attn_wgs_per_chunk_and_cu()
        return max(1, (per_cu * max(8, self._cu_count() - free_cus)) // per_chunk)

    def reserve_cus(self, n):
        """Leave ``n`` of the chip's CUs free of backward workgroups (data parallel: RCCL's channels).  The persistent grids are
        derived from the device's CU count and from how many workgroups of the selected attention backward fit a CU;
        explicit MSST_ATTN_CHUNKS / MSST_BWD_GRID settings win."""
        total = self._cu_count()
        n = max(0, min(int(n), total - 8))
        if "MSST_ATTN_CHUNKS" not in os.environ:
            self.attn_chunks = self.default_attn_chunks(n)
        if "MSST_BWD_GRID" not in os.environ:
            self.grid_rows = total - n

    def queue_capable(self):
        """Will blocks_bwd run the kernels that can DRAW their tiles (msst_block_bwd_chain with a tile queue: the two-head attention
        backward + the fused LN1 / MLP launch)?  The static part of blocks_bwd's `chain` predicate: bf16 tuned kernels, no kernel
        selection flags, an even head count with at most four head pairs, chaining not switched off.  (fp32, odd or more than
        eight heads, MSST_DBG flags, MSST_BWD_CHAIN=0 fall back to msst_block_bwd: full static grids.)"""
        H = int(self.enc.heads)
        return (self.prec == PREC_BF16 and _kernel_flags() == 0 and H % 2 == 0 and H // 2 <= 4
                and os.environ.get("MSST_BWD_CHAIN", "1") != "0")

    def set_precision(self, name):
        prec = _prec_of(name)
        if prec != self.prec:
            self.prec = prec
            self._wbuf = None

    def _require_cuda(self, t):
        if not t.is_cuda:
            raise RuntimeError(
                "maskedsst_amd runs on an MI355X only (tensor is on %s); there is no CPU fallback" % t.device)

    def ensure(self):
        """flat buffers + operand-layout weight storage + prep job table (rebuilt if params moved)"""
        if self.fp.stale():
            self.fp.flatten()
            self._wbuf = None
        if self._wbuf is None:
            self._build_weight_storage()

    def _layers(self):
        """[(stack name, layer index)] in forward order"""
        L = self.enc.depth
        return [("spatial", l) for l in range(L)] + [("spectral", l) for l in range(L)]

    def _build_weight_storage(self):
        dev = self.fp.flat.device
        self._require_cuda(self.fp.flat)
        H = self.enc.heads
        inner = H * DH
        esz = 4 if self.prec == PREC_F32 else 2
        mats = [("wqkv", 3 * inner, D), ("wout", D, inner), ("w1", MLP, D), ("w2", D, MLP)]
        # bf16: three more copies in the 32-row x 16-k fragment packing of the round-3 attention backward (32x32x16 MFMAs)
        # (name, rows, cols, transpose, field, scale_rows): pack = 1; wqkvT32 carries dim_head^-0.5 in its q and k blocks
        mats32 = [("wqkv", 3 * inner, D, 0, "wqkv32", 0), ("wout", D, inner, 1, "woutT32", 0), ("wqkv", 3 * inner, D, 1, "wqkvT32", 2 * inner)] \
            if self.prec != PREC_F32 else []
        # bf16: and the four forward matrices once more as IEEE half (MSST_FWD_HALF: the fp16-operand forward), same fragment packing
        mats_h = [(name, r, c, name + "_h") for name, r, c in mats] if self.prec != PREC_F32 else []
        per_layer = sum(2 * r * c for _, r, c in mats) + sum(r * c for _, r, c, _, _, _ in mats32) + sum(r * c for _, r, c, _ in mats_h)
        layers = self._layers()
        self._wbuf = torch.empty(per_layer * len(layers) * esz, dtype=torch.uint8, device=dev)
        base = self._wbuf.data_ptr()
        jobs = (MsstPrepJob * ((8 + len(mats32) + len(mats_h)) * len(layers)))()
        self._bw = []
        self._bg = []
        off = 0
        j = 0
        maxel = 0
        for sname, l in layers:
            bw = MsstBlockWeights()
            bw.struct_bytes = ctypes.sizeof(MsstBlockWeights)
            for name, r, c in mats:
                src = self.fp.ptr(f"{sname}.{l}.{name}")
                for tr in (0, 1):
                    dst = base + off * esz
                    jobs[j].src, jobs[j].dst, jobs[j].rows, jobs[j].cols, jobs[j].transpose = src, dst, r, c, tr
                    setattr(bw, name + ("T" if tr else ""), dst)
                    off += r * c
                    j += 1
                    maxel = max(maxel, r * c)
            for name, r, c, tr, field, scale_rows in mats32:
                dst = base + off * esz
                jobs[j].src, jobs[j].dst, jobs[j].rows, jobs[j].cols = self.fp.ptr(f"{sname}.{l}.{name}"), dst, r, c
                jobs[j].transpose, jobs[j].pack = tr, 1
                jobs[j].scale_rows, jobs[j].scale = scale_rows, float(DH) ** -0.5
                dr, dk = (c, r) if tr else (r, c)   # destination rows x contraction length: whole 32 x 16 fragments only
                assert dr % 32 == 0 and dk % 16 == 0, (name, r, c, tr)
                setattr(bw, field, dst)
                off += r * c
                j += 1
            for name, r, c, field in mats_h:
                dst = base + off * esz
                jobs[j].src, jobs[j].dst, jobs[j].rows, jobs[j].cols = self.fp.ptr(f"{sname}.{l}.{name}"), dst, r, c
                jobs[j].transpose, jobs[j].pack = 0, _lib.PREP_HALF
                setattr(bw, field, dst)
                off += r * c
                j += 1
            for name in ("ln1_g", "ln1_b", "bo", "ln2_g", "ln2_b", "b1", "b2"):
                setattr(bw, name, self.fp.ptr(f"{sname}.{l}.{name}"))
            self._bw.append(bw)
            bg = MsstBlockGrads()
            for name in ("ln1_g", "ln1_b", "wqkv", "wout", "bo", "ln2_g", "ln2_b", "w1", "b1", "w2", "b2"):
                setattr(bg, name, self.fp.ptr(f"{sname}.{l}.{name}", self.fp.grad))
            self._bg.append(bg)
        raw = bytes(jobs)
        self._jobs = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
        self._njobs = j
        self._maxel = maxel

    def prep_weights(self):
        """fp32 master weights -> operand layout (one launch); call after every parameter update"""
        self.ensure()
        first = getattr(self, "_prep_flag", None) is None or self._prep_flag.device != self._jobs.device
        if first:
            self._prep_flag = torch.zeros(1, dtype=torch.int32, device=self._jobs.device)
            self._prep_checked = None
        _lib.check(self.lib.msst_prep_weights(_p(self._jobs), self._njobs, ctypes.sizeof(MsstPrepJob), self._maxel, self.prec,
                                              _p(self._prep_flag), _stream()), "msst_prep_weights")
        if self._prep_checked is not self._jobs:   # once per job table: did the kernel skip a malformed job? (one sync at setup)
            bad = int(self._prep_flag.item())
            if bad:
                raise _lib.MsstError(f"msst_prep_weights skipped malformed jobs (flags {bad}): operand copies are incomplete")
            self._prep_checked = self._jobs
        if self.prec == PREC_BF16:
            self._ln1_guard_launch()

    # ------------------------------------------------------------------ parameter guards of MSST_LN1_FROM_XN and MSST_FWD_HALF
    LN1_XN_MAX_RATIO = 12.0   # max |ln1_b / ln1_g|: xhat = (row - b) / g amplifies the bf16 rounding of the saved rows by 1 + |b / g| / |xhat|
    HALF_MAX_BOUND = 3.0e4    # bound on |q|, |k|, |v|, |attention output| and the MLP's hidden pre-activation (half's largest finite value: 65504)

    def _ln1_guard_launch(self):
        """Two numbers over every block, computed on the device from the flat parameter buffer (a [blocks, floats per block] view: the
        blocks' parameters lie a constant stride apart) and copied to pinned host memory WITHOUT a synchronisation -- read some steps later
        (parameters move by <= lr per step; both thresholds are orders of magnitude, not margins):
          * max |ln1_b / ln1_g| (inf when a gamma is 0): MSST_LN1_FROM_XN divides by gamma;
          * a bound on every half operand the forward produces (MSST_FWD_HALF): |W x| <= max_row ||W_row||_1 * max |x|, with
            |LayerNorm row| <= max |gamma| * sqrt(96) + max |beta| -- q / k / v (and the attention output, a convex combination of v
            rows) from Wqkv and LN1, the hidden pre-activation (>= |GELU output|) from W1, b1 and LN2."""
        if getattr(self, "_ln1_idx_key", None) is not self._jobs:
            blocks = [f"{s_}.{l}" for s_, l in self._layers()]
            names = ["ln1_g", "ln1_b", "wqkv", "ln2_g", "ln2_b", "w1", "b1"]
            seg0 = [self.fp.segments[f"{blocks[0]}.{n}"] for n in names]
            start = min(s[0] for s in seg0)
            span = max(s[0] + s[1] for s in seg0) - start
            d = self.fp.block_stride(blocks, names)   # block 0 -> block 1 of the forward order: negative in FlatParams' own layout
            # rows of the view: the blocks in memory order, from the lowest; they must not overlap (a single block has no stride: no view)
            self._guard_view = (min(start, start + d * (len(blocks) - 1)), abs(d), len(blocks),
                                {n: s[0] - start for n, s in zip(names, seg0)}, span) if d is not None and abs(d) >= span else None
            self._ln1_idx_key = self._jobs
            self._ln1_host = torch.empty(2, dtype=torch.float32, pin_memory=True)
            self._ln1_ev = None
            self._ln1_ratio = None
            self._half_bound = None
            self._ln1_calls = 0
        if self._guard_view is None:
            return                                                     # (not our own flat layout: both switches stay off)
        self._ln1_calls += 1
        if self._ln1_ev is not None and self._ln1_ev.query():      # the copy launched some parameter updates ago has landed: adopt its values
            self._ln1_ratio, self._half_bound = float(self._ln1_host[0]), float(self._ln1_host[1])
            self._ln1_ev = None
        # fresh values every 8th parameter update are enough; the very first call synchronises once
        if self._ln1_ratio is not None and (self._ln1_ev is not None or self._ln1_calls % 8 != 1):
            return
        lo, stride, n, rel, span = self._guard_view
        H = self.enc.heads
        base = self.fp.flat[lo:]
        m = base.as_strided((n, span), (stride, 1), base.storage_offset())

        def t(name, *shape):
            k = int(np.prod(shape))
            return m[:, rel[name]:rel[name] + k].reshape((n,) + shape)
        g1, b1_, g2, b2_ = t("ln1_g", 96).abs(), t("ln1_b", 96).abs(), t("ln2_g", 96).abs(), t("ln2_b", 96).abs()
        ratio = (b1_ / g1).nan_to_num(nan=float("inf")).max()
        ln1_max = g1.amax(1) * (96 ** 0.5) + b1_.amax(1)
        ln2_max = g2.amax(1) * (96 ** 0.5) + b2_.amax(1)
        qkv = t("wqkv", 3 * H * DH, 96).abs().sum(-1).amax(1) * ln1_max
        hid = t("w1", MLP, 96).abs().sum(-1).amax(1) * ln2_max + t("b1", MLP).abs().amax(1)
        bound = torch.maximum(qkv, hid).nan_to_num(nan=float("inf")).max()
        self._ln1_host.copy_(torch.stack((ratio, bound)), non_blocking=True)
        self._ln1_ev = torch.cuda.Event()
        self._ln1_ev.record()
        if self._ln1_ratio is None:
            self._ln1_ev.synchronize()
            self._ln1_ratio, self._half_bound = float(self._ln1_host[0]), float(self._ln1_host[1])
            self._ln1_ev = None

    def ln1_xn_ok(self):
        r = getattr(self, "_ln1_ratio", None)
        return r is not None and r <= self.LN1_XN_MAX_RATIO

    def half_ok(self):
        """may the forward's GEMM operands be IEEE half?  (every one of them provably below HALF_MAX_BOUND; unknown -> no)"""
        b = getattr(self, "_half_bound", None)
        return b is not None and b <= self.HALF_MAX_BOUND

    # ------------------------------------------------------------------ forward pieces
    def _pos_tables(self, buf=None):
        """(split, a, b): the position tables the tokenizer kernels read, or with buf = the gradient buffer write -- spectral_pos_embed:
        pos_embed | channel_embed, split after pos_embed's width; else the one pos_embedding table (split 0, no b)"""
        fp = self.fp
        if self.enc.spectral_pos_embed:
            return self.enc.pos_embed.shape[-1], fp.ptr("pos_embed", buf), fp.ptr("channel_embed", buf)
        return 0, fp.ptr("pos_embedding", buf), 0

    def _zero_mask_for(self, n, device):
        """an all-zero token mask of at least n bytes on `device` (nothing masked), grown or moved when needed"""
        if self._zero_mask is None or self._zero_mask.numel() < n or self._zero_mask.device != torch.device(device):
            self._zero_mask = torch.zeros(n, dtype=torch.uint8, device=device)
        return self._zero_mask

    def _tok_params(self, grad=False):
        """the tokenizer's parameters as every tokenizer entry point takes them (pre_g, pre_b, w_emb, b_emb, post_g, post_b), or with
        grad=True their places in the gradient buffer"""
        buf = self.fp.grad if grad else None
        return tuple(ctypes.c_void_p(self.fp.ptr(k, buf)) for k in ("pre_g", "pre_b", "embed.w.0", "embed.b.0", "post_g", "post_b"))

    def _tok_bwd_slab(self, nsamples, device):
        """(nchunk, slab) of a tokenizer backward over nsamples samples: nchunk partial-gradient slabs per spectral block, then the
        [S][N][96] position-gradient staging"""
        S, N, P = self.S, self.N, self.P
        nchunk = max(1, min(nsamples, self.tok_chunks))
        ss = N * 96 + 96 * P + 96 * 4 + 32
        return nchunk, torch.empty(S * nchunk * ss + S * N * 96, dtype=torch.float32, device=device)

    # the generic tokenizer kernels run one grid row per window; the fp32-MFMA ones (P = 10, 8 x 8 windows) walk any number
    TILE_WINDOWS_PER_LAUNCH = 65535

    def _launch_chunk(self, src, emb_drop):
        """windows of src per tokenizer launch: all of them for the fp32-MFMA kernels, else TILE_WINDOWS_PER_LAUNCH at most -- and then
        without embedding dropout (a dropout element is addressed by its place in one launch's output: launches in turn would repeat
        the first one's masks)"""
        total = src.n
        chunk = total if (self.P == 10 and self.enc.num_spatial_patches_sqrt == 8) else min(total, self.TILE_WINDOWS_PER_LAUNCH)
        if chunk < total and emb_drop[0] > 0:
            raise NotImplementedError(f"embedding dropout over {total} windows in one step needs more than one launch of the generic "
                                      f"tokenizer ({self.TILE_WINDOWS_PER_LAUNCH} windows each): "
                                      f"{'use fewer tiles' if src.kind == 'tiles' else 'list fewer windows'} per step")
        return chunk

    def _src(self, src):
        return src if isinstance(src, Windows) else Windows("batch", src)

    def _src_args(self, src, win0, n):
        """what a tokenizer entry point is told of windows win0 .. win0 + n - 1 of src: (its leading pointers, its shape integers)"""
        S, P = self.S, self.P
        if src.kind == "batch":
            return (_p(src.img),), (n, S, self.N, P)
        Bs, _, Hs, Ws = src.img.shape
        s = self.enc.num_spatial_patches_sqrt
        if src.kind == "tiles":
            return (_p(src.img),), (Bs, Hs, Ws, s, s, win0, n, S, P)
        lead = (_p(src.img), _p(src.origins[win0:] if win0 else src.origins))
        if src.orient is not None:   # the _orient entry points: the orientation table follows the origins
            lead += (_p(src.orient[win0:] if win0 else src.orient),)
        return lead, (Bs, Hs, Ws, s, n, S, P)

    def tokenize(self, src, mask_u8=None, with_pos=True, emb_drop=(0.0, 0)):
        """tokens [n, T, 96] (position added, embedding dropout) of the n windows of src, a Windows or a bare batch img [B, C, H, W] fp32
        cuda; with mask_u8 [n, T] the mask token substituted.  Tiles and listed windows are read where they lie, bit for bit what the
        stacked copy gives.  One launch, or for tiles / unmasked listed windows under the generic kernels several (_launch_chunk)."""
        src = self._src(src)
        self._require_cuda(src.img)
        self.ensure()
        masked = mask_u8 is not None
        name, drop_args = _tok_entry(_TOK_FWD, "tokenize", src, masked, emb_drop)
        S, N, total = self.S, self.N, src.n
        T = S * N
        dev = src.img.device
        out = torch.empty(total, T, D, dtype=torch.float32, device=dev)
        fp, V = self.fp, ctypes.c_void_p
        if not with_pos:
            if getattr(self, "_zero_pos", None) is None or self._zero_pos.numel() < T * D:
                self._zero_pos = torch.zeros(T * D, dtype=torch.float32, device=dev)
            split, pos_a, pos_b = 0, self._zero_pos.data_ptr(), 0
        else:
            split, pos_a, pos_b = self._pos_tables()
        mask_args, chunk = (), total
        if src.kind == "batch" or masked:   # these entry points take the mask token and a mask (nothing masked: the zero mask), one launch
            mask_args = (V(fp.ptr("mask_token") if self.mim is not None else fp.ptr("post_b")),
                         _p(mask_u8 if masked else self._zero_mask_for(total * T, dev)))
        else:
            chunk = self._launch_chunk(src, emb_drop)
        fn, par, st = getattr(self.lib, name), self._tok_params(), _stream()
        for win0 in (range(0, total, chunk) if chunk < total else (0,)):
            lead, dims = self._src_args(src, win0, min(chunk, total - win0))
            _lib.check(fn(*lead, *par, V(pos_a), V(pos_b), split, *mask_args, _p(out[win0:] if win0 else out), *dims, *drop_args, st), name)
        return out

    def blocks_fwd(self, x0, save=True, drop=(0.0, 0)):
        """run the 2*depth fused blocks; returns (list of activations [x0 .. x_2L], list of x1)"""
        acts = [x0]
        x1s = []
        flags = _kernel_flags()
        role_split = self._role_split(flags)
        # bf16 x1 rows (MSST_X1_BF16): only the role-split forward writes them; MSST_X1_BF16=0 keeps fp32 rows.  The x1 tensor's
        # dtype tells the backward which kind it holds.
        x1_bf16 = save and role_split and os.environ.get("MSST_X1_BF16", "1") != "0"
        want_lse = save and role_split and os.environ.get("MSST_LSE", "1") != "0"
        # MSST_FWD_HALF (round 6): the role-split forward multiplies IEEE-half operands (11 significant bits, same MFMA rate) instead of
        # bf16 ones -- the bf16 forward's loss error against the fp32 reference is owned by the rounding of the weights
        # (tools/bf16_error_table.py: 2.7e-4 -> 7e-6 on the Houston-shape anchor).  MSST_FWD_HALF=0: bf16 operands.
        # (decided per launch by _half_flag)
        layers = self._layers()
        # Round 5: a whole stack (its blocks never mix tiles) as ONE launch of the role-split forward -- msst_block_fwd_stack; same
        # arithmetic, bit-identical outputs, no prologue + pipeline fill / drain per block.  MSST_FWD_STACK=0: one launch per block.
        # Measured (tools/fwd_ab.py): ahead when a workgroup holds few tiles (batch 64: -5.5 % forward time, Houston shape: -7.3 %),
        # behind when it holds many (batch 256, EnMAP shape: +1.3 %) -- MSST_FWD_STACK=1 / 0 force it on / off, otherwise by tiles per workgroup.
        want_stack = os.environ.get("MSST_FWD_STACK", "auto")
        stacked = role_split and want_stack != "0"
        i0 = 0
        self.fwd_launch_blocks = []   # blocks carried by each block-forward launch of this call (bench.py normalises per-launch numbers with it)
        while i0 < len(layers):
            i1 = i0
            while i1 < len(layers) and layers[i1][0] == layers[i0][0] and i1 - i0 < 16:
                i1 += 1
            use = stacked and (want_stack == "1" or self._tiles_per_workgroup(layers[i0][0], x0.shape[0]) <= STACK_MAX_TILES)
            if use and self._fwd_stack(acts, x1s, i0, i1, save, drop, x1_bf16, want_lse):
                self.fwd_launch_blocks.append(i1 - i0)
            else:
                for i in range(i0, i1):
                    self._fwd_block(acts, x1s, i, save, drop, x1_bf16, want_lse, flags)
                self.fwd_launch_blocks += [1] * (i1 - i0)
            i0 = i1
        return acts, x1s

    def blocks_fwd_pingpong(self, x0, drop=(0.0, 0), other=None, n=None, stream=None):
        """the 2*depth fused blocks with nothing kept for a backward, on two token buffers in turn (x0 and `other`, one more of its
        shape; x0 is overwritten): returns the last block's output.  One msst_block_fwd per block with the kernels, precision flags and
        dropout arguments of blocks_fwd(save=False) -- the same bits -- but one residual stream of scratch instead of 2*depth.
        n: the batch, when the buffers hold more rows than are in use (scene_forward's last chunk)."""
        B = x0.shape[0] if n is None else n
        S, N, H = self.S, self.N, self.enc.heads
        flags = _kernel_flags()
        prec = self.prec | flags | self._half_flag(flags)
        x, y = x0, torch.empty_like(x0) if other is None else other
        wrote = ctypes.c_int(0)
        st = _stream() if stream is None else stream
        for i, (sname, _) in enumerate(self._layers()):
            _lib.check(self.lib.msst_block_fwd(ctypes.byref(self._bw[i]), _p(x), _p(y), None, _MODE[sname], B, S, N, H, prec, self.max_grid,
                                               drop[0], drop[1], i, None, None, ctypes.byref(wrote), st), "msst_block_fwd")
            x, y = y, x
        return x

    def _tiles_per_workgroup(self, sname, B):
        """64-row tiles the busiest workgroup of a block forward walks (the library's own tiling: msst_block_lse_floats counts tiles x heads x 64)"""
        mode = _MODE[sname]
        key = (mode, B)
        hit = self._tpw.get(key)
        if hit is None:
            tiles = int(self.lib.msst_block_tiles(mode, B, self.S, self.N))
            grid = max(1, min(tiles, self._cu_count(), self.max_grid if self.max_grid > 0 else tiles))
            hit = self._tpw[key] = -(-tiles // grid)
        return hit

    def _role_split(self, flags):
        """may the role-split forward run?  bf16, 8 heads, no kernel-selection flags -- the one kernel that writes bf16 x1 rows and
        softmax statistics, takes IEEE-half operands and has the one-launch stack form"""
        return self.prec == PREC_BF16 and self.enc.heads == 8 and flags == 0

    def _half_flag(self, flags):
        """MSST_FWD_HALF for a forward launch: the role-split kernel, unless MSST_FWD_HALF=0"""
        self.fwd_half = self._role_split(flags) and os.environ.get("MSST_FWD_HALF", "1") != "0" and self.half_ok()
        return _lib.FWD_HALF if self.fwd_half else 0

    def _attach_saved(self, x1, wrote, xn, lse):
        """what a block forward saved beside x1 (its `saved` word) rides on the x1 tensor object, so that every caller keeps its
        (acts, x1s) pair: the LN1 rows, the softmax statistics, whether LN1's rstd is in their tail, whether they are those of
        half-operand scores (the backward then renormalises: MSST_LSE_RENORM)"""
        x1._msst_xn = xn if (wrote & _lib.SAVED_XN) else None
        x1._msst_lse = lse if (lse is not None and (wrote & _lib.SAVED_LSE)) else None
        x1._msst_rstd = bool(wrote & _lib.SAVED_RSTD) and x1._msst_lse is not None
        x1._msst_half = bool(self.fwd_half)

    def _fwd_block(self, acts, x1s, i, save, drop, x1_bf16, want_lse, flags):
        """block i as its own launch (msst_block_fwd): appends its output to acts, its saved mid residual to x1s"""
        x = acts[-1]
        B = x.shape[0]
        S, N, H = self.S, self.N, self.enc.heads
        sname, l = self._layers()[i]
        y = torch.empty_like(x)
        x1 = (torch.empty(x.shape, dtype=torch.bfloat16, device=x.device) if x1_bf16 else torch.empty_like(x)) if save else None
        # bf16: the block also saves LN1(x) as it used it (bf16 rows), if the selected kernel can; the attention backward
        # then skips its own LN1.
        xn = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device) if (save and self.prec != PREC_F32) else None
        mode = _MODE[sname]
        # ... and (role-split kernel) the softmax statistics of every (tile, head, row): MSST_LSE=0 keeps the backward's own softmax
        lse = None
        if xn is not None and want_lse:
            lse = torch.empty(int(self.lib.msst_block_lse_floats(mode, B, S, N, H)), dtype=torch.float32, device=x.device)
        wrote = ctypes.c_int(0)
        _lib.check(self.lib.msst_block_fwd(ctypes.byref(self._bw[i]), _p(x), _p(y), _p(x1), mode, B, S, N, H,
                                           self.prec | flags | (_lib.X1_BF16 if x1_bf16 else 0) | self._half_flag(flags), self.max_grid, drop[0], drop[1], i, _p(xn), _p(lse),
                                           ctypes.byref(wrote), _stream()),
                   "msst_block_fwd")
        if x1 is not None:
            self._attach_saved(x1, wrote.value, xn, lse)
        acts.append(y)
        x1s.append(x1)

    def _fwd_stack(self, acts, x1s, i0, i1, save, drop, x1_bf16, want_lse):
        """blocks i0 .. i1 - 1 (one stack) through msst_block_fwd_stack, one launch; False when the library refuses the call (too many
        (tile, block) steps per workgroup for its step table, or per-block operands that are not a constant stride apart): the caller
        then launches block by block"""
        x0 = acts[-1]
        B = x0.shape[0]
        S, N, H = self.S, self.N, self.enc.heads
        dev = x0.device
        n = i1 - i0
        mode = _MODE[self._layers()[i0][0]]
        # one allocation per kind, block j its j-th slice: the kernel addresses block j's operands as block 0's + j x a byte stride
        # (the weight copies and the flat parameters are laid out that way by _build_weight_storage / FlatParams)
        def slices(dtype, shape=None):
            t = torch.empty((n,) + tuple(shape if shape is not None else x0.shape), dtype=dtype, device=dev)
            return [t[j] for j in range(n)]
        ys = slices(x0.dtype)
        x1 = slices(torch.bfloat16 if x1_bf16 else torch.float32) if save else None
        xn = slices(torch.bfloat16) if save else None
        lse = slices(torch.float32, (int(self.lib.msst_block_lse_floats(mode, B, S, N, H)),)) if (save and want_lse) else None
        wv = (ctypes.POINTER(MsstBlockWeights) * n)(*[ctypes.pointer(self._bw[i0 + j]) for j in range(n)])
        VP = ctypes.c_void_p * n

        def arr(ts):
            return VP(*[t.data_ptr() for t in ts]) if ts is not None else None
        wrote = ctypes.c_int(0)
        rc = self.lib.msst_block_fwd_stack(wv, n, _p(x0), arr(ys), arr(x1), arr(xn), arr(lse), mode, B, S, N, H,
                                           self.prec | (_lib.X1_BF16 if x1_bf16 else 0) | self._half_flag(0), self.max_grid, drop[0], drop[1], i0,
                                           ctypes.byref(wrote), _stream())
        if rc == -2:   # MSST_ERR_UNSUPPORTED: nothing was launched
            return False
        _lib.check(rc, "msst_block_fwd_stack")
        for j in range(n):
            acts.append(ys[j])
            if save:
                self._attach_saved(x1[j], wrote.value, xn[j], lse[j] if lse is not None else None)
                x1s.append(x1[j])
            else:
                x1s.append(None)
        return True

    def head_fwd(self, y, src, idx32, want_pred=False):
        """the masked-L1 head over y [B, T, 96] -> (loss, dpred, pred); the targets come from src: a batch img [B, C, s, s], or listed
        windows, read where they lie in their scenes (msst_head_at_fwd; oriented: msst_head_at_fwd_orient): the same bits"""
        src = self._src(src)
        if src.kind == "tiles":
            raise NotImplementedError("head_fwd: no entry point for tiles windows")
        B, T, _ = y.shape
        K = idx32.shape[1]
        dev = y.device
        dpred = torch.empty(B, K, self.P, dtype=torch.float32, device=dev)
        pred = torch.empty(B, K, self.P, dtype=torch.float32, device=dev) if want_pred else None
        partial = torch.empty(B * ((K + 63) // 64), dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        per_block = 1 if hasattr(self.mim.to_pixels, "layers") else 0
        V = ctypes.c_void_p
        name = "msst_head_fwd" if src.kind != "listed" else "msst_head_at_fwd" if src.orient is None else "msst_head_at_fwd_orient"
        lead, dims = self._src_args(src, 0, B)
        _lib.check(getattr(self.lib, name)(
            _p(y), *lead, _p(idx32), V(self.fp.ptr("to_pixels.w.0")), V(self.fp.ptr("to_pixels.b.0")), per_block,
            _p(dpred), _p(pred), _p(partial), _p(loss), *dims, K, _stream()), name)
        return loss, dpred, pred

    def recon_fwd(self, y, img, mask_u8, blend=True, stats=True):
        """to_pixels over every token of y [B, T, 96] -> (recon [B, S P, N], band_err [B, S P] float64, band_cnt [B, S P] int32; the
        last two None without stats): module-level recon_fwd on this model's to_pixels tables"""
        per_block = 1 if hasattr(self.mim.to_pixels, "layers") else 0
        V = ctypes.c_void_p
        return recon_fwd(y, img, mask_u8, V(self.fp.ptr("to_pixels.w.0")), V(self.fp.ptr("to_pixels.b.0")), per_block, blend,
                         self.S, self.N, self.P, stats=stats, lib=self.lib)

    def reconstruct(self, img, mask_u8, blend=True):
        """Eval forward of the SimMIM model down to pixels: img [B, C, H, W] fp32 cuda, mask_u8 [B, T] uint8 cuda (1 = masked) ->
        (recon [B, S P, N] fp32, band_err [B, S P] float64, band_cnt [B, S P] int32).  The encoder path of simmim_loss in eval
        mode (prep_weights, tokenize with the mask token, the blocks with nothing saved and no dropout, at the model's
        precision), then msst_recon_fwd instead of the gather head.  No autograd; the current stream."""
        self._require_cuda(img)
        if self.mim is None:
            raise RuntimeError("reconstruct needs the SimMIM wrapper's mask token and to_pixels (a bare encoder has neither)")
        img = img.contiguous().float()
        with torch.no_grad():
            self.prep_weights()
            x0 = self.tokenize(img, mask_u8)
            acts, _ = self.blocks_fwd(x0, save=False)
            return self.recon_fwd(acts[-1], img, mask_u8, blend)

    def tokenize_scene_masked(self, scene, scene_mask_u8, stride, win0, nwin, out=None):
        """msst_tokenize_scene_fwd_masked: the tokens of windows win0 .. win0 + nwin - 1 of scene [Bs, C, Hs, Ws] (fp32 cuda, contiguous)
        with the tokens that scene_mask_u8 [Bs, S, Hs, Ws] (uint8, non-zero = masked) marks replaced by the mask token -> out
        [>= nwin, T, 96]; bit for bit what tokenize gives for the copied windows and their copied masks"""
        self._require_cuda(scene)
        self._require_cuda(scene_mask_u8)
        if self.mim is None:
            raise RuntimeError("tokenize_scene_masked needs the SimMIM wrapper's mask token (a bare encoder has none)")
        self.ensure()
        Bs, _, Hs, Ws = scene.shape
        S, N, P = self.S, self.N, self.P
        w = self.enc.num_spatial_patches_sqrt
        if scene.dtype != torch.float32 or not scene.is_contiguous() or scene_mask_u8.dtype != torch.uint8 or \
                not scene_mask_u8.is_contiguous() or tuple(scene_mask_u8.shape) != (Bs, S, Hs, Ws):
            raise ValueError(f"tokenize_scene_masked takes a contiguous fp32 scene and a contiguous uint8 mask [{Bs}, {S}, {Hs}, {Ws}]")
        if out is None:
            out = torch.empty(nwin, S * N, D, dtype=torch.float32, device=scene.device)
        fp = self.fp
        split, pos_a, pos_b = self._pos_tables()
        V = ctypes.c_void_p
        _lib.check(self.lib.msst_tokenize_scene_fwd_masked(
            _p(scene), *self._tok_params(), V(pos_a), V(pos_b), split, V(fp.ptr("mask_token")), _p(scene_mask_u8), _p(out),
            Bs, Hs, Ws, w, stride, win0, nwin, S, P, _stream()), "msst_tokenize_scene_fwd_masked")
        return out

    def reconstruct_scene(self, scene, scene_mask_u8, stride, blend=True, max_windows=2048):
        """Eval forward of the SimMIM model down to pixels over every window of scene [Bs, C, Hs, Ws] (window = image_size, origins 0,
        stride, 2 stride, ...) with scene_mask_u8 [Bs, S, Hs, Ws] (uint8 cuda, non-zero = masked) -> (cube [Bs, C, Hs, Ws] fp32,
        band_err [Bs, C] float64, band_cnt [Bs, C] int32, cover [Bs, Hs, Ws] int32).  The loop of scene_forward: chunks of at most
        max_windows windows; the masked scene tokenizer reads a chunk's windows out of the scene, the blocks run on two token buffers
        in turn, msst_recon_fwd (no blend, no statistics) writes per-window predictions and msst_scene_recon_assemble adds them into
        the cube, finalizing on the last chunk (mean over the covering windows, blend, per-band masked error, cover).  No dropout,
        nothing saved, no autograd; the current stream; the model's precision."""
        self._require_cuda(scene)
        self._require_cuda(scene_mask_u8)
        if self.mim is None:
            raise RuntimeError("reconstruct_scene needs the SimMIM wrapper's mask token and to_pixels (a bare encoder has neither)")
        with torch.no_grad():
            scene = scene.contiguous().float()
            scene_mask_u8 = scene_mask_u8.contiguous()
            Bs, C, Hs, Ws = scene.shape
            S, N, P = self.S, self.N, self.P
            w = self.enc.num_spatial_patches_sqrt
            total, chunk = self._scene_chunking(scene, stride, max_windows)
            dev = scene.device
            # msst_recon_fwd reads a cube and a token mask whatever blend is: with blend = 0 and no statistics neither reaches its output
            no_img = torch.zeros(chunk, S * P, N, dtype=torch.float32, device=dev)
            no_mask = self._zero_mask_for(chunk * S * N, dev)
            win_recon = torch.empty(chunk, S * P, N, dtype=torch.float32, device=dev)
            cube = torch.empty(Bs, C, Hs, Ws, dtype=torch.float32, device=dev)
            err = torch.empty(Bs, C, dtype=torch.float64, device=dev)
            cnt = torch.empty(Bs, C, dtype=torch.int32, device=dev)
            cover = torch.empty(Bs, Hs, Ws, dtype=torch.int32, device=dev)
            per_block = 1 if hasattr(self.mim.to_pixels, "layers") else 0
            V = ctypes.c_void_p
            st = _stream()
            for win0, n, y in self._scene_encoder_chunks(scene, stride, total, chunk, st, scene_mask_u8):
                _lib.check(self.lib.msst_recon_fwd(_p(y), _p(no_img), _p(no_mask), V(self.fp.ptr("to_pixels.w.0")),
                                                   V(self.fp.ptr("to_pixels.b.0")), per_block, 0, _p(win_recon), None, None, n, S, N, P, st),
                           "msst_recon_fwd")
                _lib.check(self.lib.msst_scene_recon_assemble(_p(win_recon), win0, n, _p(scene), _p(scene_mask_u8), _p(cube), _p(err),
                                                              _p(cnt), _p(cover), Bs, S, P, Hs, Ws, w, stride, int(win0 + n == total),
                                                              int(bool(blend)), st), "msst_scene_recon_assemble")
            return cube, err, cnt, cover

    # ------------------------------------------------------------------ backward pieces
    def _fire(self, bucket):
        if self.bucket_hook is not None:
            for name, start, end in self.fp.buckets:
                if name == bucket:
                    self.bucket_hook(name, start, end)

    def head_bwd(self, y, dpred, csr_ptr, csr_pos, gout=None):
        """-> dy [B, T, 96]; to_pixels grads land in the flat grad buffer"""
        B, T, _ = y.shape
        S, N, P = self.S, self.N, self.P
        K = dpred.shape[1]
        dev = y.device
        nchunk = max(1, min(B, int(os.environ.get("MSST_HEAD_CHUNKS", "0")) or 512 // max(S, 1)))
        dy = torch.empty_like(y)
        slab = torch.empty(S * nchunk * (P * 96 + P), dtype=torch.float32, device=dev)
        per_block = 1 if hasattr(self.mim.to_pixels, "layers") else 0
        gscale = 1.0 / (B * K * P) / K
        V = ctypes.c_void_p
        g = self.fp.grad
        _lib.check(self.lib.msst_head_bwd(
            _p(y), _p(dpred), _p(csr_ptr), _p(csr_pos), V(self.fp.ptr("to_pixels.w.0")), per_block, gscale, _p(gout),
            _p(dy), _p(slab), nchunk, V(self.fp.ptr("to_pixels.w.0", g)), V(self.fp.ptr("to_pixels.b.0", g)),
            B, S, N, P, K, _stream()), "msst_head_bwd")
        self._fire("head")
        return dy

    def _grad_stride(self, nlayers):
        """floats between the gradient tensors of consecutive backward calls (block i -> block i - 1), or None when the blocks'
        gradients are not laid out a constant, 16-byte-aligned stride apart (msst_block_bwd_reduce needs that)"""
        blocks = [f"{sname}.{l}" for sname, l in self._layers()[:nlayers]]
        d = self.fp.block_stride(blocks, [n for n, _ in MsstBlockGrads._fields_])   # forward order: the backward walks it in reverse
        return -d if d is not None and d < 0 and d % 4 == 0 else None

    def _bwd_workspace(self, B, device):
        """(dx1, part, slab, dab): the scratch of one block backward at batch B, shared by every block of a backward pass"""
        H = self.enc.heads
        ntok = B * self.S * self.N
        esz = 4 if self.prec == PREC_F32 else 2
        dx1 = torch.empty(ntok * 96, dtype=torch.float32, device=device)
        part = torch.empty(H * ntok * 96 * esz, dtype=torch.uint8, device=device)
        # the bf16 MLP backward runs two workgroups per CU: up to 2 * grid_rows MLP slabs (msst_block_bwd lays the parts out);
        # the chained form adds one MLP slab per workgroup of the fused LN1 + MLP launch
        slab = torch.empty(self.grid_rows * (3 * MLP_SLAB + LN1_SLAB) + self.attn_chunks * H * ATTN_SLAB, dtype=torch.float32, device=device)
        dab = torch.empty(ntok * 96, dtype=torch.bfloat16, device=device) if self.prec != PREC_F32 else None
        return dx1, part, slab, dab

    def blocks_bwd(self, acts, x1s, dy, drop=(0.0, 0)):
        """backward through the 2*depth blocks (reverse order); returns dx0"""
        H = self.enc.heads
        ntok = dy.shape[0] * self.S * self.N
        ws = self._bwd_workspace(dy.shape[0], dy.device)
        x1_bf16 = len(x1s) > 0 and all(t.dtype == torch.bfloat16 for t in x1s)
        if not x1_bf16 and any(t.dtype != torch.float32 for t in x1s):
            raise ValueError("saved x1 rows of mixed dtypes")
        # Chained backward (msst_block_bwd_chain): the LN1 backward of block i and the MLP-half backward of block i - 1 are
        # one launch, dx of block i stays on chip.  bf16 tuned kernels with saved LN1 rows only; at most four d(LN1 out)
        # partials (one per head pair for an even head count, else one per head).
        nparts = H // 2 if H % 2 == 0 else H
        chain = (self.prec == PREC_BF16 and _kernel_flags() == 0 and all(getattr(t, "_msst_xn", None) is not None for t in x1s)
                 and nparts <= 4 and os.environ.get("MSST_BWD_CHAIN", "1") != "0" and self.enc.depth > 0
                 and ntok * 384 < 2 ** 31 - 16 and nparts * ntok * 192 < 2 ** 31 - 16)   # 32-bit buffer offsets in the fused launch
        # MSST_LN1_FROM_XN (round 6): the fused LN1 + MLP launch rebuilds xhat of LN1 from the saved bf16 LN1 rows and the saved rstd
        # instead of re-reading the fp32 block input (192 of 2304 bytes per token less) -- when the forward saved both for every block,
        # and the LN1 parameters allow the division by gamma (ln1_xn_ok: max |beta / gamma| <= 12, checked on the device a step behind)
        ln1_from_xn = (chain and x1_bf16 and os.environ.get("MSST_LN1_XN", "1") != "0"
                       and all(getattr(t, "_msst_rstd", False) for t in x1s) and self.ln1_xn_ok())
        self.last_bwd_ln1_from_xn = bool(ln1_from_xn)
        if chain:
            return self._blocks_bwd_chained(acts, x1s, dy, drop, ws,
                                            (_lib.X1_BF16 if x1_bf16 else 0) | (_lib.LN1_FROM_XN if ln1_from_xn else 0))
        return self._blocks_bwd_unchained(acts, x1s, dy, drop, ws)

    def _blocks_bwd_chained(self, acts, x1s, dy, drop, ws, x1flags):
        """blocks_bwd through msst_block_bwd_chain, one call per block; x1flags: MSST_X1_BF16 / MSST_LN1_FROM_XN as blocks_bwd decided"""
        B = dy.shape[0]
        S, N, H = self.S, self.N, self.enc.heads
        dev = dy.device
        dx1, part, slab, dab = ws
        layers = self._layers()
        # dynamic tile queues (attach_data_parallel sets self.tile_queue; MSST_TILE_QUEUE=1 forces them): see include/msst.h
        queue = None
        if self.tile_queue or os.environ.get("MSST_TILE_QUEUE", "0") == "1":
            if getattr(self, "_queue_ws", None) is None or self._queue_ws.device != dev:
                self._queue_ws = torch.zeros(64, dtype=torch.int32, device=dev)
            queue = self._queue_ws
        last = len(layers) - 1
        dx0 = torch.empty_like(dy)
        null_w = ctypes.POINTER(MsstBlockWeights)()
        null_g = ctypes.POINTER(MsstBlockGrads)()
        # Deferred slab reduction (msst_block_bwd_reduce, opt-in with MSST_BWD_DEFER=1): every call of a run of same-mode blocks
        # keeps its own slab set and ONE launch reduces the run -- 2 block reductions per step instead of 2 * depth.  Bit-identical
        # gradients; measured (LABNOTES round 4): the reductions drop from 566 to 400 us per EnMAP step, but the producers pay it
        # back -- their slab epilogues now write 1.5 GB of cold memory per step instead of the same 62 MB that the reduction just
        # read (attention backward +6 us per launch) -- so the per-call reduction stays the default.
        gstride = self._grad_stride(len(layers))
        defer = gstride is not None and os.environ.get("MSST_BWD_DEFER", "0") == "1"
        nslab_r = (slab.numel() + 3) // 4 * 4
        if defer:
            slab = torch.empty(nslab_r * len(layers), dtype=torch.float32, device=dev)
        run_start = last
        for i in reversed(range(len(layers))):
            sname, l = layers[i]
            prev = i > 0
            x1 = x1s[i]
            slab_i = slab[(last - i) * nslab_r:] if defer else slab
            _lib.check(self.lib.msst_block_bwd_chain(
                ctypes.byref(self._bw[i]), ctypes.byref(self._bg[i]),
                ctypes.byref(self._bw[i - 1]) if prev else null_w, ctypes.byref(self._bg[i - 1]) if prev else null_g,
                _p(acts[i]), _p(x1), _p(x1s[i - 1]) if prev else _p(None), _p(dy) if i == last else _p(None),
                _p(None) if prev else _p(dx0), _p(dx1), _p(part), _p(slab_i), self.grid_rows, self.attn_chunks, _MODE[sname],
                B, S, N, H, self.prec | x1flags | (_lib.LSE_RENORM if getattr(x1, "_msst_half", False) else 0) |
                (_lib.BWD_DEFER_REDUCE if defer else 0), drop[0], drop[1], i, _p(x1._msst_xn), _p(getattr(x1, "_msst_lse", None)), _p(dab),
                1 if i == last else 0, _p(queue), _stream()),
                "msst_block_bwd_chain")
            if not defer:
                self._fire(f"{sname}.{l}")
            elif i == 0 or layers[i - 1][0] != sname:   # the run of this stack ends here: reduce it, then announce its blocks
                count = run_start - i + 1
                _lib.check(self.lib.msst_block_bwd_reduce(
                    ctypes.byref(self._bg[run_start]), ctypes.byref(self._bg[run_start - 1]) if run_start > 0 else null_g,
                    _p(slab[(last - run_start) * nslab_r:]), nslab_r, gstride, count, count if i > 0 else count - 1,
                    1 if run_start == last else 0, self.grid_rows, self.attn_chunks, _MODE[sname], B, S, N, H, self.prec, _stream()),
                    "msst_block_bwd_reduce")
                for j in range(run_start, i - 1, -1):
                    self._fire(f"{layers[j][0]}.{layers[j][1]}")
                run_start = i - 1
        return dx0

    def _blocks_bwd_unchained(self, acts, x1s, dy, drop, ws):
        """blocks_bwd block by block (block_bwd_single) on two gradient buffers in turn: dy and one more"""
        layers = self._layers()
        g, other = dy, torch.empty_like(dy)
        for i in reversed(range(len(layers))):
            self.block_bwd_single(i, acts[i], x1s[i], g, other, drop=drop, ws=ws)
            g, other = other, g
            self._fire(f"{layers[i][0]}.{layers[i][1]}")
        return g

    def block_bwd_single(self, i, x, x1, dy, dx=None, drop=(0.0, 0), ws=None):
        """Backward of block i alone (msst_block_bwd: MLP half, attention half, LN1 backward, slab reduction): x = the block's input,
        x1 = its saved mid residual (with the LN1 rows / statistics its forward attached), dy = the gradient at its output -> dx;
        the block's parameter gradients land in the flat gradient buffer.  The unchained loop of blocks_bwd runs on it; the parity tests
        call it block by block with the ORACLE's activations and gradients (no error carried from block to block)."""
        dx1, part, slab, dab = ws if ws is not None else self._bwd_workspace(dy.shape[0], dy.device)
        if dx is None:
            dx = torch.empty_like(dy)
        if x1.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("saved x1 rows must be fp32 or bf16")
        x1flag = _lib.X1_BF16 if x1.dtype == torch.bfloat16 else 0
        _lib.check(self.lib.msst_block_bwd(
            ctypes.byref(self._bw[i]), ctypes.byref(self._bg[i]), _p(x), _p(x1), _p(dy), _p(dx),
            _p(dx1), _p(part), _p(slab), self.grid_rows, self.attn_chunks, _MODE[self._layers()[i][0]], dy.shape[0], self.S, self.N, self.enc.heads,
            self.prec | _kernel_flags() | x1flag | (_lib.LSE_RENORM if getattr(x1, "_msst_half", False) else 0),
            drop[0], drop[1], i, _p(getattr(x1, "_msst_xn", None)), _p(getattr(x1, "_msst_lse", None)), _p(dab), _stream()), "msst_block_bwd")
        return dx

    def tokenize_bwd(self, src, mask_u8, dx0, emb_drop=(0.0, 0), with_pos=True):
        """backward of tokenize(src, mask_u8, with_pos, emb_drop): dx0 [n, T, 96] -> the tokenizer's gradients, the position tables' and
        (a SimMIM model's batch, or any masked source) the mask token's in the flat buffer.  One launch over all windows, with the nchunk
        a batch of as many samples takes: the same bits.  with_pos=False: gradients of the embedding / its two LayerNorms only (the
        position table and the mask token were applied outside the kernel, by the caller's own autograd ops)"""
        src = self._src(src)
        masked = mask_u8 is not None
        name, drop_args = _tok_entry(_TOK_BWD, "tokenize_bwd", src, masked, emb_drop)
        total, dev = src.n, src.img.device
        nchunk, slab = self._tok_bwd_slab(total, dev)
        g, V = self.fp.grad, ctypes.c_void_p
        split, dpa, dpb = self._pos_tables(g) if with_pos else (0, 0, 0)
        mask_args = dmt_args = ()
        if src.kind == "batch" or masked:   # these entry points take a mask (nothing masked: the zero mask) and the mask token's gradient
            mask_args = (_p(mask_u8 if masked else self._zero_mask_for(total * self.S * self.N, dev)),)
            dmt_args = (V(self.fp.ptr("mask_token", g) if (self.mim is not None and with_pos) else 0),)
        lead, dims = self._src_args(src, 0, total)
        _lib.check(getattr(self.lib, name)(
            *lead, *self._tok_params(), *mask_args, _p(dx0), _p(slab), nchunk, *self._tok_params(grad=True), V(dpa), V(dpb), split,
            *dmt_args, *dims, *drop_args, _stream()), name)
        if with_pos:
            self._fire("tokenizer")

    # ------------------------------------------------------------------ input gradient (msst_input_grad.hip)
    def tokenize_input_bwd(self, src, mask_u8, dx0, dtarget=None, emb_drop=(0.0, 0)):
        """d(loss)/d(src.img) through the tokenizer: dx0 [n, T, 96] the gradient at its output.  Reads only; the parameter gradients are
        tokenize_bwd's business.
        batch: mask_u8 [B, T] or None, dtarget [B, S P, N] (head_bwd_target) added before the store -> a new tensor, written whole.
        tiles: the same over the windows read in place, zeros in the trailing rows and columns that belong to no window.
        listed (with src.csr): the windows overlap -- one msst_tokenize_at_bwd_input writes the per-window gradients dwin [n, C, N], one
        msst_scene_fold_at sums them per pixel in its fixed order into a new tensor written whole (zeros where no window lies), or
        into src.sink's running map: the sink's first fold writes it whole, the later ones accumulate."""
        src = self._src(src)
        img = src.img
        self._require_cuda(img)
        name, drop_args = _tok_entry(_TOK_INPUT_BWD, "tokenize_input_bwd", src, mask_u8 is not None, emb_drop)
        if dtarget is not None and src.kind != "batch":
            raise NotImplementedError(f"tokenize_input_bwd: no entry point for {src.kind} windows with a target gradient")
        lead, dims = self._src_args(src, 0, src.n)
        fn, par, st = getattr(self.lib, name), self._tok_params(), _stream()
        if src.kind != "listed":
            dimg = torch.empty(img.shape, dtype=torch.float32, device=img.device)
            mask_args = (_p(mask_u8),) if src.kind == "batch" else ()
            target_args = (_p(dtarget),) if src.kind == "batch" else ()
            _lib.check(fn(*lead, *par, *mask_args, _p(dx0), *target_args, _p(dimg), *dims, *drop_args, st), name)
            return dimg
        if src.csr is None:
            raise NotImplementedError("no input gradient through windows at listed origins unless the forward opted in "
                                      "(forward_at(..., scene_grad=True)): they overlap, so d(scene) is an accumulating fold")
        sink = src.sink
        if sink is None:
            out = torch.empty(img.shape, dtype=torch.float32, device=img.device)
        else:
            out = sink.out
            if tuple(out.shape) != tuple(img.shape) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != img.device:
                raise ValueError(f"out must be a contiguous fp32 tensor {tuple(img.shape)} on the scene's device")
        Bs, C, Hs, Ws = img.shape
        dwin = torch.empty(src.n, C, self.N, dtype=torch.float32, device=img.device)
        _lib.check(fn(*lead, *par, _p(dx0), _p(dwin), *dims, *drop_args, st), name)
        _lib.check(self.lib.msst_scene_fold_at(_p(dwin), _p(src.csr[0]), _p(src.csr[1]), _p(out), Bs, C, Hs, Ws, self.enc.num_spatial_patches_sqrt, src.n, self.P,
                                               int(bool(sink and sink.started)), st), "msst_scene_fold_at")
        if sink:
            sink.started = True
        return out

    def head_bwd_target(self, dpred, csr_ptr, csr_pos, gout=None):
        """the SimMIM loss's direct dependence on the input (msst_head_bwd_target): dpred [B, K, P] of head_fwd and the inverse CSR
        head_bwd takes -> dtarget [B, S P, N], the gradient of the loss through its target (the raw pixels of the masked patches)"""
        B, K, P = dpred.shape
        dtarget = torch.empty(B, self.S * P, self.N, dtype=torch.float32, device=dpred.device)
        _lib.check(self.lib.msst_head_bwd_target(_p(dpred), _p(csr_ptr), _p(csr_pos), _p(gout), _p(dtarget), B, self.S, self.N, P, K,
                                                 _stream()), "msst_head_bwd_target")
        return dtarget

    # ------------------------------------------------------------------ autograd entry (SimMIM loss)
    def trainable(self):
        """[(flat name, parameter)] of everything that receives a gradient in pre-training"""
        if self.fp.flat is None or getattr(self, "_trainable_key", None) != self.fp.version:
            groups, _ = self.fp._ordered()
            self._trainable = [(n, p) for _, g in groups for n, p in g]
            self._trainable_key = self.fp.version if self.fp.flat is not None else None
        return self._trainable

    def dropout_state(self):
        """(p, seed) for this forward: p = transformer dropout when the encoder is in training mode (the
        reference's nn.Dropout sites, vit_spatial_spectral.py:38,40,57,62), else 0.  A fresh 32-bit seed is
        drawn from the torch CPU generator per forward (reproducible under torch.manual_seed); the masks are a
        stateless function of (seed, layer, site, element) that the backward regenerates."""
        p = float(self.enc.dropout_p) if self.enc.training else 0.0
        if p <= 0.0:
            return 0.0, 0
        if not 0.0 < p < 1.0:
            raise ValueError(f"dropout probability {p} outside (0, 1)")
        seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
        # data parallel: every rank draws the same seed from identically seeded generators; mix the rank in so that
        # the ranks' dropout masks are independent (as they are for the reference's per-process RNG streams)
        rank = int(getattr(self.mim, "dp_rank", 0)) if self.mim is not None else 0
        if rank:
            seed = (seed ^ (rank * 0x9E3779B1)) & 0x7FFFFFFF
        return p, seed

    def _upload(self, dev, *arrays):
        """Host arrays of one step -> device, without stalling the launch queue.

        A ``.to(device)`` from pageable memory is stream ordered AND host blocking: the host sat until the
        previous step had drained, and the GPU then idled while the next step's launches were issued (measured:
        2 ms per 41 ms step).  Going through pinned staging buffers keeps the copies asynchronous: they queue on
        the compute stream behind the previous step and the host keeps launching.  Two pinned sets alternate; a
        set is rewritten only after the copy that last read it has run (host waits on its event, i.e. the host
        runs at most two steps ahead).  The DEVICE tensors are fresh per call (caching allocator, stream ordered):
        the autograd path stashes them for its backward, and any number of further forwards (eval / no_grad ones
        included) may run between a forward and its backward without touching them."""
        if getattr(self, "_up", None) is None:
            self._up = {"sets": [None, None], "k": 0}
        up = self._up
        k = up["k"]
        up["k"] = 1 - k
        cur = up["sets"][k]
        sig = tuple((a.shape, a.dtype) for a in arrays)
        if cur is None or cur["sig"] != sig:
            cur = {"sig": sig,
                   "pin": [torch.empty(a.shape, dtype=torch.from_numpy(a).dtype, pin_memory=True) for a in arrays],
                   "ev": torch.cuda.Event()}
            up["sets"][k] = cur
        else:
            cur["ev"].synchronize()
        out = []
        for pin, a in zip(cur["pin"], arrays):
            pin.numpy()[...] = a
            d = torch.empty(pin.shape, dtype=pin.dtype, device=dev)
            d.copy_(pin, non_blocking=True)
            out.append(d)
        cur["ev"].record(torch.cuda.current_stream(dev))
        return out

    def simmim_loss(self, src, bool_mask, idx=None):
        """scalar loss attached to autograd (reference SimMIMSpatialSpectral.forward :203-340) of src: a batch img [B, C, s, s], or the
        windows listed in a Windows' origins of resident tiles, read where they lie: no stacked copy.  bool_mask / idx: one row per
        window; or bool_mask a ``DeviceMasks`` alone (masks drawn on the device: its four tensors reach the kernels as they lie).
        Listed windows give the loss and, through autograd, every parameter gradient the bits of the stacked batch; the tiles get
        no gradient (SimMIMSpatialSpectral.forward_at refuses tiles that ask for one)"""
        src = self._src(src)
        img = src.img
        self._require_cuda(img)
        self.ensure()
        T = self.S * self.N
        from . import masking
        if isinstance(bool_mask, masking.DeviceMasks):
            # drawn on the device (msst_draw_masks): the four tensors reach the kernels as they lie -- no numpy, no inverse_csr, no upload
            dm = bool_mask
            if idx is not None:
                raise ValueError("a DeviceMasks carries its own indices: pass it alone")
            masking.check_device_masks(dm, src.n, T, dm.idx.shape[1] if torch.is_tensor(dm.idx) and dm.idx.dim() == 2 else 0)
            if dm.bool_mask.device != img.device:
                raise ValueError(f"DeviceMasks on {dm.bool_mask.device}, input on {img.device}")
            mask_u8, idx32, csr_ptr, csr_pos = dm.bool_mask.view(torch.uint8), dm.idx, dm.csr_ptr, dm.csr_pos
        else:
            bm = bool_mask.cpu().numpy() if torch.is_tensor(bool_mask) else np.asarray(bool_mask)
            ix = idx.cpu().numpy() if torch.is_tensor(idx) else np.asarray(idx)
            ptr, pos = masking.inverse_csr(ix, T)   # (looked up on the module at call time)
            mask_u8, idx32, csr_ptr, csr_pos = self._upload(img.device, bm.astype(np.uint8), ix.astype(np.int32), ptr, pos)
        names = [n for n, _ in self.trainable()]
        params = [p for _, p in self.trainable()]
        want_img = src.kind == "batch" and img.requires_grad
        if not torch.is_grad_enabled() or not (want_img or any(p.requires_grad for p in params)):
            self.prep_weights()
            x0 = self.tokenize(src, mask_u8)
            acts, _ = self.blocks_fwd(x0, save=False, drop=self.dropout_state())
            loss, _, _ = self.head_fwd(acts[-1], src, idx32)
            return loss
        return _SimMIMLossFn.apply(self, names, self.dropout_state(), src, img, mask_u8, idx32, csr_ptr, csr_pos, *params)

    # ------------------------------------------------------------------ encoder-level API (inference)
    def _block_param_names(self):
        return [n for n, _ in self.trainable() if n.startswith(("spatial.", "spectral."))]

    def _embed_param_names(self):
        return [n for n, _ in self.trainable() if n.startswith(("embed.", "pre_", "post_"))]

    def transformer(self, tokens):
        """ViTSpatialSpectral.transformer_forward (reference :495-499): both stacks on [B, T, 96] tokens.  Attached to
        autograd when gradients are enabled, so a caller that keeps the reference's own SimMIMSpatialSpectral
        (vit_simmim_original.py:298) and swaps only the encoder trains through the HIP blocks: d(tokens) flows on to
        whatever produced them, the block parameters receive views of the flat gradient buffer."""
        self._require_cuda(tokens)
        self.ensure()
        drop = self.dropout_state()
        tokens = tokens.contiguous().float()
        by_name = dict(self.trainable())
        names = self._block_param_names()
        params = [by_name[n] for n in names]
        if torch.is_grad_enabled() and (tokens.requires_grad or any(p.requires_grad for p in params)):
            return _TransformerFn.apply(self, names, drop, tokens, *params)
        self.prep_weights()
        acts, _ = self.blocks_fwd(tokens, save=False, drop=drop)
        return acts[-1]

    def embed_patches(self, patches):
        """BlockwisePatchEmbedding.embed on patches [B, S, N, P] (no position / mask terms; reference :210-222),
        attached to autograd for the embedding parameters when gradients are enabled."""
        self._require_cuda(patches)
        self.ensure()
        B, S, N, P = patches.shape
        want_input = torch.is_grad_enabled() and patches.requires_grad
        # patches that require a gradient stay attached: the permute into the cube layout is a torch op, so d(patches) comes back
        # in the [B, S, N, P] layout it was given
        img = (patches if want_input else patches.detach()).permute(0, 1, 3, 2).reshape(B, S * P, N).contiguous().float()
        by_name = dict(self.trainable())
        names = self._embed_param_names()
        params = [by_name[n] for n in names]
        if torch.is_grad_enabled() and (want_input or any(p.requires_grad for p in params)):
            return _EmbedFn.apply(self, names, img, *params)
        return self.tokenize(img, None, with_pos=False)

    def features(self, img):
        """forward_features (reference :518-534): tokenize + pos (+ embedding dropout in training mode) -> transformer.

        Differentiable like the reference's: when gradients are enabled and any encoder parameter or the input requires one, the result is
        composed of the two autograd entry points (``embed_patches`` and ``transformer``) with the position add and the
        embedding dropout as ordinary torch ops in between -- exactly what the reference's own SimMIM wrapper does with this
        encoder -- so a custom head trained on these features trains the encoder too.  Otherwise (eval / no_grad) one fused
        tokenizer launch does embed + position + dropout."""
        enc = self.enc
        params = [q for _, q in self.trainable()]
        if torch.is_grad_enabled() and (img.requires_grad or any(q.requires_grad for q in params)):
            self._require_cuda(img)
            patches = enc.to_patch_embedding.to_patch(img.contiguous().float())
            tokens = self.embed_patches(patches).reshape(img.shape[0], -1, D)
            pos = enc.get_pos_embeddings() if enc.spectral_pos_embed else enc.pos_embedding[:, :tokens.shape[1]]
            tokens = tokens + pos
            if enc.training and float(enc.emb_dropout_p) > 0:
                tokens = torch.nn.functional.dropout(tokens, p=float(enc.emb_dropout_p), training=True)
            return self.transformer(tokens)
        pe = float(enc.emb_dropout_p) if enc.training else 0.0
        emb_drop = (pe, int(torch.randint(0, 2 ** 31 - 1, (1,)).item())) if pe > 0 else (0.0, 0)
        x0 = self.tokenize(img, None, with_pos=True, emb_drop=emb_drop)
        with torch.no_grad():
            return self.transformer(x0)

    # ------------------------------------------------------------------ classification (row a17 / finetune.py)
    def _head_kind(self):
        """key into _HEADS of the classifier head the encoder was built with"""
        return "pix" if self.enc.pixelwise else "spec" if self.enc.spectral_mlp_head else "cls"

    def _head_params(self, head, buf=None):
        """the head's LayerNorm weight, bias and Linear weight, bias in the flat buffer (or in buf: the gradient buffer)"""
        return [ctypes.c_void_p(self.fp.ptr(f"mlp_head.{i}.{wb}", buf)) for i in (0, head.linear) for wb in ("weight", "bias")]

    def _head_fwd(self, kind, y, B=None, logits=None, stream=None):
        """logits of head `kind` over tokens y [>= B, T, 96]; the kernel writes every element of `logits` (head.shape(B, nc, N)),
        whatever it held.  B: the batch, when y and logits hold more rows than are in use (scene_forward's last chunk)."""
        head = _HEADS[kind]
        B = y.shape[0] if B is None else B
        nc = self.enc.num_classes
        if logits is None:
            logits = torch.empty(head.shape(B, nc, self.N), dtype=torch.float32, device=y.device)
        ws = None if head.fwd_ws is None else torch.empty(int(head.fwd_ws(self.lib, B, self.S, self.N, nc)), dtype=torch.float32, device=y.device)
        _lib.check(getattr(self.lib, head.fwd)(
            _p(y), *self._head_params(head), _p(logits), *([] if ws is None else [_p(ws)]), B, self.S, self.N, nc,
            _stream() if stream is None else stream), head.fwd)
        return logits

    def _head_bwd(self, kind, y, dlogits, dy=None, want_dy=True):
        """-> dy [B, T, 96], written whole (None with want_dy=False, a frozen body: the kernel variant without dy runs, null dy); the
        four head gradients are written (not accumulated) into the flat gradient buffer, the same bits either way"""
        head = _HEADS[kind]
        B = y.shape[0]
        nc = self.enc.num_classes
        if dy is None and want_dy:
            dy = torch.empty_like(y)
        slab = torch.empty(int(head.bwd_slab(self.lib, B, self.S, self.N, nc)), dtype=torch.float32, device=y.device)
        g = self._head_params(head, self.fp.grad)
        _lib.check(getattr(self.lib, head.bwd)(
            _p(y), _p(dlogits), *self._head_params(head)[:3], _p(dy), _p(slab), *g, B, self.S, self.N, nc, _stream()), head.bwd)
        self._fire("cls_head")
        return dy

    # the six public names run their own head's kernels on this model's mlp_head parameters, whatever head the encoder has
    def cls_head_fwd(self, y, logits=None):
        return self._head_fwd("cls", y, logits=logits)

    def cls_head_bwd(self, y, dlogits, dy=None, want_dy=True):
        return self._head_bwd("cls", y, dlogits, dy, want_dy)

    def spec_head_fwd(self, y, logits=None):
        return self._head_fwd("spec", y, logits=logits)

    def spec_head_bwd(self, y, dlogits, dy=None, want_dy=True):
        return self._head_bwd("spec", y, dlogits, dy, want_dy)

    def pix_head_fwd(self, y, logits=None):
        return self._head_fwd("pix", y, logits=logits)

    def pix_head_bwd(self, y, dlogits, dy=None, want_dy=True):
        return self._head_bwd("pix", y, dlogits, dy, want_dy)

    def head_logits(self, y):
        """the classifier head the encoder was built with: logits [B, nc, N] ([B, nc] for the pixelwise head)"""
        return self._head_fwd(self._head_kind(), y)

    def head_logits_bwd(self, y, dlogits, want_dy=True):
        return self._head_bwd(self._head_kind(), y, dlogits, want_dy=want_dy)

    def _classify_view(self, logits, B):
        """the reference's output layout: [B, nc, H, W]; pixelwise: [B, nc, 1, 1].squeeze() -- [B, nc], or [nc] when B = 1"""
        if self._head_kind() == "pix":
            return logits.view(B, -1, 1, 1).squeeze()
        H = W = self.enc.num_spatial_patches_sqrt
        return logits.view(B, -1, H, W)

    def classify(self, img):
        """ViTSpatialSpectral.forward: logits [B, num_classes, H, W] (reference :536-564); pixelwise: [B, num_classes] ([num_classes]
        for B = 1, the reference's squeeze)."""
        self._require_cuda(img)
        self.ensure()
        return self._classify(Windows("batch", img))

    def classify_tiles(self, tiles):
        """classify(stack_image_batch(tiles)) without the stacked copy: logits of every non-overlapping s x s window of tiles
        [B, C, Ht, Wt] (s = the model's image size; trailing Ht % s rows and Wt % s columns dropped), windows numbered (tile, window
        row, window column) -- the reference's shifting_window training batch (src/utils.py:608-613, :451-474).  [B nr nq, num_classes,
        s, s]; pixelwise: [B nr nq, num_classes].  The three regimes of classify, the same seeds drawn in the same order (equal
        torch.manual_seed: equal bits), and what is kept for the backward is the tiles.
        Limit: windows other than 8 x 8 of 10-band patches (a pixelwise model's 7 x 7) run the generic tokenizer, 65535 windows per
        launch; more windows than that in one call are tokenized in several launches, but with embedding dropout on the call raises
        NotImplementedError (a dropout element is addressed by its place in one launch's output)."""
        self._require_cuda(tiles)
        self.ensure()
        s = self.enc.num_spatial_patches_sqrt
        src = Windows("tiles", tiles, s=s)
        if min(src.grid) < 1:
            raise ValueError(f"tiles of {tuple(tiles.shape[-2:])} hold no {s} x {s} window")
        return self._classify(src)

    def classify_at(self, src):
        """classify(the stacked s x s windows of the scenes src.img [Bs, C, Hs, Ws] at src.origins [n, 3] = (scene, y0, x0)) without the
        stacked copy: both tokenizer passes read the listed windows in place (msst_tokenize_at_fwd / _bwd).  origins: int32, contiguous,
        on the scene's device, every row inside the scene (ViTSpatialSpectral.forward_at checks).  Shapes, regimes, seeds and limits of
        classify_tiles; n = 0 is refused."""
        self._require_cuda(src.img)
        self.ensure()
        if src.n < 1:
            raise ValueError("origins lists no window")
        return self._classify(src)

    def window_alignment(self):
        """A: a window's logits and gradients keep their bits when its place in the batch moves by a multiple of A windows.  The block
        kernels pack whole sequences of several windows into 64-row tiles (TileMap, msst_dev.h: 64 // S spectral sequences, 64 // N
        spatial ones), and a sequence's slot in its tile decides how its few non-zero terms fall into the MFMAs' partial sums -- the
        last bit of a window's result (1e-7 relative in fp32) depends on its place in the batch modulo A.  saliency.scene_saliency
        cuts its chunks so that every window keeps its place modulo A."""
        from math import gcd
        a = b = 1
        if 0 < self.S <= 64:
            ts = 64 // self.S
            a = ts // gcd(self.N, ts)
        if 0 < self.N <= 64:
            ts = 64 // self.N
            b = ts // gcd(self.S, ts)
        return a * b // gcd(a, b)

    def _classify(self, src):
        """classify / classify_tiles / classify_at on their source"""
        img, B = src.img, src.n
        p = float(self.enc.dropout_p) if self.enc.training else 0.0
        pe = float(self.enc.emb_dropout_p) if self.enc.training else 0.0
        seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item()) if (p > 0 or pe > 0) else 0
        drop, emb_drop = (p, seed), (pe, seed ^ 0x5bd1e995)
        named = self.trainable()
        want = torch.is_grad_enabled() and (img.requires_grad or any(q.requires_grad for _, q in named))
        if self.mim is not None and want:
            raise NotImplementedError("train the classifier through a bare ViTSpatialSpectral (as finetune.py "
                                      "does), not through an encoder wrapped in SimMIMSpatialSpectral")
        if want and (img.requires_grad or any(q.requires_grad for n, q in named if not n.startswith("mlp_head."))):
            out = _ClassifyFn.apply(self, [n for n, _ in named], drop, emb_drop, src, img, *[q for _, q in named])
            return self._classify_view(out, B)
        self.prep_weights()
        x0 = self.tokenize(src, None, emb_drop=emb_drop)
        if not want:
            acts, _ = self.blocks_fwd(x0, save=False, drop=drop)
            return self._classify_view(self.head_logits(acts[-1]), B)
        # linear evaluation (reference finetune.py:110-136: only mlp_head trains): the body runs as in a no-gradient forward --
        # module still in training mode, so its dropout stays on -- with nothing saved, and only the head has a backward.  (An
        # input that requires a gradient needs the full body backward: that call takes the full path above.)
        y = self.blocks_fwd_pingpong(x0, drop=drop)
        head = [(n, q) for n, q in named if n.startswith("mlp_head.")]
        out = _HeadOnlyFn.apply(self, [n for n, _ in head], y, *[q for _, q in head])
        return self._classify_view(out, B)

    # ------------------------------------------------------------------ scene inference (maskedsst_amd/scene.py, msst_scene_assemble)
    def scene_forward(self, scene, stride, max_windows):
        """Eval forward of every window of scene [Bs, C, Hs, Ws] (window = image_size, origins 0, stride, 2 stride, ...): returns
        (logits [Bs, num_classes, Hs, Ws] = mean over the windows covering a pixel, classes [Bs, Hs, Ws] int64, -1 where uncovered).
        Windows run in chunks of at most max_windows: one tokenizer launch reads a chunk's windows out of the scene, the blocks
        run on two token buffers in turn (msst_block_fwd, the kernels and precision flags of blocks_fwd; its one-launch stack
        variant computes the same bits but keeps every block's output), the head writes per-window logits and msst_scene_assemble
        adds them into the scene map.  A pixelwise model's window logits go to the window's centre pixel instead
        (msst_scene_centre_assemble): logits 0 and class -1 on every pixel that is no window's centre.  No dropout, nothing saved
        for a backward."""
        self._require_cuda(scene)
        scene = scene.contiguous().float()
        Bs, _, Hs, Ws = scene.shape
        w, nc, N = self.enc.num_spatial_patches_sqrt, self.enc.num_classes, self.N
        total, chunk = self._scene_chunking(scene, stride, max_windows)
        dev = scene.device
        kind = self._head_kind()
        head = _HEADS[kind]
        win_logits = torch.empty(head.shape(chunk, nc, N), dtype=torch.float32, device=dev)
        logits = torch.empty(Bs, nc, Hs, Ws, dtype=torch.float32, device=dev)
        classes = torch.empty(Bs, Hs, Ws, dtype=torch.int64, device=dev)
        st = _stream()
        for win0, n, x in self._scene_encoder_chunks(scene, stride, total, chunk, st):
            self._head_fwd(kind, x, n, win_logits, st)
            _lib.check(getattr(self.lib, head.assemble)(_p(win_logits), win0, n, _p(logits), _p(classes), Bs, nc, Hs, Ws, w, stride,
                                                        int(win0 + n == total), st), head.assemble)
        return logits, classes

    def _scene_chunking(self, scene, stride, max_windows):
        """(total, chunk): the windows of scene [Bs, C, Hs, Ws] at this stride and how many of them run at a time"""
        Bs, _, Hs, Ws = scene.shape
        w = self.enc.num_spatial_patches_sqrt
        nr, nq = (Hs - w) // stride + 1, (Ws - w) // stride + 1
        total = Bs * nr * nq
        return total, max(1, min(int(max_windows), total, 65535))   # 65535: the generic tokenizer runs one grid row per window

    def _scene_encoder_chunks(self, scene, stride, total, chunk, st, scene_mask_u8=None):
        """the front of scene_forward, encode_scene and reconstruct_scene: for every chunk of windows of scene (contiguous fp32) yields
        (win0, n, y), y the encoder output [>= n, T, 96] of windows win0 .. win0 + n - 1 -- one msst_tokenize_scene_fwd launch (with
        scene_mask_u8 [Bs, S, Hs, Ws]: tokenize_scene_masked) reads them out of the scene, the blocks run on two token buffers in turn.
        y is one of the two buffers: the next chunk overwrites it."""
        self.ensure()
        Bs, _, Hs, Ws = scene.shape
        S, N, P = self.S, self.N, self.P
        w = self.enc.num_spatial_patches_sqrt
        self.prep_weights()
        split, pos_a, pos_b = self._pos_tables()
        bufs = [torch.empty(chunk, S * N, D, dtype=torch.float32, device=scene.device) for _ in range(2)]
        V = ctypes.c_void_p
        for win0 in range(0, total, chunk):
            n = min(chunk, total - win0)
            if scene_mask_u8 is not None:
                self.tokenize_scene_masked(scene, scene_mask_u8, stride, win0, n, out=bufs[0])
            else:
                _lib.check(self.lib.msst_tokenize_scene_fwd(
                    _p(scene), *self._tok_params(), V(pos_a), V(pos_b), split, _p(bufs[0]), Bs, Hs, Ws, w, stride, win0, n, S, P, st),
                    "msst_tokenize_scene_fwd")
            yield win0, n, self.blocks_fwd_pingpong(bufs[0], other=bufs[1], n=n, stream=st)

    # ------------------------------------------------------------------ scene embedding maps (msst_scene_embed.hip)
    def encode_scene(self, scene, stride, normalize=False, max_windows=2048):
        """Eval forward of the encoder over every window of scene [Bs, C, Hs, Ws] (window = image_size, origins 0, stride, 2 stride, ...)
        -> (features [Bs, 96, Hs, Ws] fp32, cover [Bs, Hs, Ws] int32).  The chunk loop of scene_forward with another tail: no head;
        msst_pool_spectral_fwd averages a window's encoder output over the spectral axis into [n, 96, N] and msst_scene_embed_assemble
        adds that into the map, finalizing on the last chunk (mean over the covering windows, with normalize the division by the
        pixel's L2 norm, NaN where no window covers a pixel, cover).  No dropout, nothing saved, no autograd; the current stream; the
        model's precision."""
        self._require_cuda(scene)
        with torch.no_grad():
            scene = scene.contiguous().float()
            Bs, _, Hs, Ws = scene.shape
            S, N = self.S, self.N
            w = self.enc.num_spatial_patches_sqrt
            total, chunk = self._scene_chunking(scene, stride, max_windows)
            dev = scene.device
            win_feat = torch.empty(chunk, D, N, dtype=torch.float32, device=dev)
            feat = torch.empty(Bs, D, Hs, Ws, dtype=torch.float32, device=dev)
            cover = torch.empty(Bs, Hs, Ws, dtype=torch.int32, device=dev)
            st = _stream()
            for win0, n, y in self._scene_encoder_chunks(scene, stride, total, chunk, st):
                _lib.check(self.lib.msst_pool_spectral_fwd(_p(y), _p(win_feat), n, S, N, st), "msst_pool_spectral_fwd")
                _lib.check(self.lib.msst_scene_embed_assemble(_p(win_feat), win0, n, _p(feat), _p(cover), Bs, D, Hs, Ws, w, stride,
                                                              int(win0 + n == total), int(bool(normalize)), st),
                           "msst_scene_embed_assemble")
            return feat, cover

    # ------------------------------------------------------------------ attention maps (msst_attn_maps.hip)
    def attn_maps_block(self, i, x, out, reduce):
        """msst_attn_maps of block i (index into _layers()) on its input x [B, T, 96] fp32: the fp32 softmax(q k^T / 8) of every
        sequence and head, written into out -- a tensor (or a view of one) whose dim 0 is the sample and whose remaining dims are
        one sample's maps, contiguous: [G, heads, L, L] (reduce = ATTN_PER_SEQ) or [heads, L, L] (ATTN_MEAN_SEQ); out.stride(0) is
        the call's sample_stride.  Reads the block's ln1_g / ln1_b and the fp32 master to_qkv.weight in the flat parameter buffer: no
        operand copy, so it is independent of prep_weights and of the precision.  The current stream."""
        self.ensure()
        sname, l = self._layers()[i]
        B = x.shape[0]
        V = ctypes.c_void_p
        fp = self.fp
        _lib.check(self.lib.msst_attn_maps(_p(x), V(fp.ptr(f"{sname}.{l}.ln1_g")), V(fp.ptr(f"{sname}.{l}.ln1_b")),
                                           V(fp.ptr(f"{sname}.{l}.wqkv")), _p(out), out.stride(0) if B > 1 else out[0].numel(),
                                           _MODE[sname], B, self.S, self.N, self.enc.heads, reduce, _stream()), "msst_attn_maps")
        return out

    def _maps_storage(self, B, nblk, tail, device):
        """the result [B, nblk, *tail] fp32 of one stack.  Every (sample, block) slice must start on 16 bytes (msst_attn_maps stores
        into it in place): when one block's maps are not a multiple of 4 floats (odd toy shapes; never with 8 heads) the slices lie
        a padded stride apart and the result is a strided view of that storage."""
        per = int(np.prod(tail))
        pad = (per + 3) // 4 * 4
        flat = torch.empty(B * nblk * pad, dtype=torch.float32, device=device)
        strides, s = [], 1
        for d in reversed(tail):
            strides.insert(0, s)
            s *= d
        return torch.as_strided(flat, (B, nblk) + tuple(tail), (nblk * pad, pad) + tuple(strides))

    def attention_maps_tokens(self, x0, stacks, blocks, reduce):
        """attention_maps on tokens x0 [B, T, 96] (overwritten): the loop of blocks_fwd_pingpong, with msst_attn_maps on the input
        of every wanted block after that block's launch and before the next block overwrites the buffer."""
        B = x0.shape[0]
        S, N, H = self.S, self.N, self.enc.heads
        out = {}
        for sname in stacks:
            L, G = (N, S) if sname == "spatial" else (S, N)
            tail = (H, L, L) if reduce == _lib.ATTN_MEAN_SEQ else (G, H, L, L)
            out[sname] = self._maps_storage(B, len(blocks), tail, x0.device)
        flags = _kernel_flags()
        prec = self.prec | flags | self._half_flag(flags)
        x, y = x0, torch.empty_like(x0)
        wrote = ctypes.c_int(0)
        st = _stream()
        layers = self._layers()
        last = max((i for i, (sname, l) in enumerate(layers) if sname in out and l in blocks), default=-1)
        for i, (sname, l) in enumerate(layers):
            if i > last:
                break   # nothing wanted reads a later block's input
            _lib.check(self.lib.msst_block_fwd(ctypes.byref(self._bw[i]), _p(x), _p(y), None, _MODE[sname], B, S, N, H, prec, self.max_grid,
                                               0.0, 0, i, None, None, ctypes.byref(wrote), st), "msst_block_fwd")
            if sname in out and l in blocks:
                self.attn_maps_block(i, x, out[sname][:, blocks.index(l)], reduce)
            x, y = y, x
        return out.get("spatial"), out.get("spectral")

    def attention_maps(self, img, mask_u8, stacks, blocks, reduce):
        """Eval forward of the encoder (encode_scene's / reconstruct's: prep_weights, tokenizer -- with the mask token where mask_u8
        [B, T] uint8 marks a token, None: nothing masked --, the blocks on two token buffers with no dropout and nothing saved, at the
        model's precision, the current stream) that hands out the attention probabilities of the wanted blocks.
        stacks: names out of ("spatial", "spectral"); blocks: layer indices within a stack; reduce: _lib.ATTN_PER_SEQ / ATTN_MEAN_SEQ.
        -> (spatial, spectral), fp32 [B, len(blocks), heads, L, L] or [B, len(blocks), G, heads, L, L]; None for a stack not asked for."""
        self._require_cuda(img)
        with torch.no_grad():
            self.prep_weights()
            x0 = self.tokenize(img.contiguous().float(), mask_u8)
            return self.attention_maps_tokens(x0, tuple(stacks), list(blocks), reduce)

    # ------------------------------------------------------------------ staged forward (tests / debugging)
    def simmim_forward_stages(self, img, bool_mask, idx, drop=(0.0, 0)):
        """Forward only, returning the intermediates the golden fixtures pin."""
        self._require_cuda(img)
        self.prep_weights()
        dev = img.device
        img = img.contiguous().float()
        mask_u8 = bool_mask.to(device=dev, dtype=torch.uint8).contiguous()
        idx32 = idx.to(device=dev, dtype=torch.int32).contiguous()
        tok_embed = self.tokenize(img, None, with_pos=False)
        x0 = self.tokenize(img, mask_u8)
        acts, x1s = self.blocks_fwd(x0, drop=drop)
        loss, dpred, pred = self.head_fwd(acts[-1], img, idx32, want_pred=True)
        L = self.enc.depth
        return dict(loss=loss, tok_embed=tok_embed, tok_masked=x0, after_spatial=acts[L], enc_out=acts[-1],
                    pred=pred, dpred=dpred, acts=acts, x1s=x1s)


class _SimMIMLossFn(torch.autograd.Function):
    """loss = SimMIM(the windows of src); gradients of every parameter come from the HIP backward kernels and are handed to autograd as
    views of the flat gradient buffer.  img = src.img, for autograd: a batch receives its gradient, tiles read through listed windows
    none."""

    @staticmethod
    def forward(ctx, eng, names, drop, src, img, mask_u8, idx32, csr_ptr, csr_pos, *params):
        eng.prep_weights()
        x0 = eng.tokenize(src, mask_u8)
        acts, x1s = eng.blocks_fwd(x0, save=True, drop=drop)
        ctx.drop = drop
        loss, dpred, _ = eng.head_fwd(acts[-1], src, idx32)
        ctx.eng = eng
        ctx.names = names
        ctx.stash = (src, mask_u8, csr_ptr, csr_pos, acts, x1s, dpred)
        return loss

    @staticmethod
    def backward(ctx, gout):
        eng = ctx.eng
        src, mask_u8, csr_ptr, csr_pos, acts, x1s, dpred = ctx.stash
        ctx.stash = None
        needs = ctx.needs_input_grad[9:]
        _refuse_accumulation(eng, ctx.names, needs)
        gout = gout.contiguous().float()
        dy = eng.head_bwd(acts[-1], dpred, csr_ptr, csr_pos, gout)
        dx0 = eng.blocks_bwd(acts, x1s, dy, drop=ctx.drop)
        dimg = None
        if ctx.needs_input_grad[4] and src.kind == "batch":   # the input asked for its gradient: two more launches that only read
            dimg = eng.tokenize_input_bwd(src, mask_u8, dx0, eng.head_bwd_target(dpred, csr_ptr, csr_pos, gout))
        if any(needs):   # (a fully frozen model: the tokenizer backward writes parameter gradients only, nobody reads them)
            eng.tokenize_bwd(src, mask_u8, dx0)
        return (None,) * 4 + (dimg,) + (None,) * 4 + _grad_views(eng, ctx.names, needs)


def _refuse_accumulation(eng, names, needs=None):
    """called by every backward before it writes gradients: none of the parameters it returns gradients for (flat names; needs: which of
    them, ctx.needs_input_grad of their slots -- a frozen parameter receives None) may still hold the view of the flat gradient
    buffer that an earlier backward handed out"""
    by_name = dict(eng.trainable())
    lo, hi = eng.fp.grad.data_ptr(), eng.fp.grad.data_ptr() + 4 * eng.fp.grad.numel()
    for i, n in enumerate(names):
        if needs is not None and not needs[i]:
            continue
        p = by_name[n]
        if p.grad is not None and lo <= p.grad.data_ptr() < hi:
            raise RuntimeError(
                "maskedsst_amd hands autograd views of its flat gradient buffer: drop the previous gradients "
                "with optimizer.zero_grad(set_to_none=True) (the torch default) before the next backward; "
                "in-place gradient accumulation across backward calls is not supported")


def _grad_views(eng, names, needs=None):
    """the gradients a backward returns to autograd: views of the flat gradient buffer the kernels have just written; None for the
    parameters that do not require one (needs: ctx.needs_input_grad of their slots)"""
    return tuple(eng.fp.view(n, eng.fp.grad) if needs is None or needs[i] else None for i, n in enumerate(names))


class _TransformerFn(torch.autograd.Function):
    """y = transformer_forward(tokens): the 2 * depth fused blocks with their HIP backward."""

    @staticmethod
    def forward(ctx, eng, names, drop, tokens, *params):
        eng.prep_weights()
        acts, x1s = eng.blocks_fwd(tokens, save=True, drop=drop)
        ctx.eng, ctx.names, ctx.drop = eng, names, drop
        ctx.stash = (acts[:-1], x1s)   # block inputs only: the output itself is not needed by the backward
        return acts[-1]

    @staticmethod
    def backward(ctx, dy):
        eng = ctx.eng
        acts, x1s = ctx.stash
        ctx.stash = None
        needs = ctx.needs_input_grad[4:]
        _refuse_accumulation(eng, ctx.names, needs)
        dx0 = eng.blocks_bwd(acts, x1s, dy.contiguous().float().clone(), drop=ctx.drop)
        return (None, None, None, dx0) + _grad_views(eng, ctx.names, needs)


class _EmbedFn(torch.autograd.Function):
    """tokens = BlockwisePatchEmbedding.embed(patches) (no position / mask terms) with its HIP backward."""

    @staticmethod
    def forward(ctx, eng, names, img, *params):
        ctx.eng, ctx.names = eng, names
        ctx.stash = (img,)
        return eng.tokenize(img, None, with_pos=False)

    @staticmethod
    def backward(ctx, dtok):
        eng = ctx.eng
        (img,) = ctx.stash
        ctx.stash = None
        needs = ctx.needs_input_grad[3:]
        _refuse_accumulation(eng, ctx.names, needs)
        dtok = dtok.contiguous().float()
        dimg = eng.tokenize_input_bwd(img, None, dtok) if ctx.needs_input_grad[2] else None
        if any(needs):
            eng.tokenize_bwd(img, None, dtok, with_pos=False)
        return (None, None, dimg) + _grad_views(eng, ctx.names, needs)


class SceneGradSink:
    """a running scene gradient map (saliency.scene_saliency): every backward of a forward_at(..., scene_grad=sink) folds its windows
    into `out` [Bs, C, Hs, Ws] fp32 -- the first one writes it whole, the later ones accumulate (msst_scene_fold_at) -- and autograd
    gets no gradient for the scene"""

    def __init__(self, out):
        self.out, self.started = out, False


class _ClassifyFn(torch.autograd.Function):
    """logits = encoder(the windows of src) for the classification path; backward through the same HIP kernels.  Both tokenizer passes
    read tiles and listed windows in place: the stash holds the source, not the windows.  img = src.img, for autograd."""

    @staticmethod
    def forward(ctx, eng, names, drop, emb_drop, src, img, *params):
        eng.prep_weights()
        x0 = eng.tokenize(src, None, emb_drop=emb_drop)
        acts, x1s = eng.blocks_fwd(x0, save=True, drop=drop)
        logits = eng.head_logits(acts[-1])
        ctx.eng, ctx.names, ctx.drop, ctx.emb_drop = eng, names, drop, emb_drop
        ctx.stash = (src, acts, x1s)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        eng = ctx.eng
        src, acts, x1s = ctx.stash
        ctx.stash = None
        needs = ctx.needs_input_grad[6:]
        _refuse_accumulation(eng, ctx.names, needs)
        dy = eng.head_logits_bwd(acts[-1], dlogits.contiguous().float())
        dx0 = eng.blocks_bwd(acts, x1s, dy, drop=ctx.drop)
        dimg = None
        if ctx.needs_input_grad[5]:   # the input asked for its gradient: launches that only read (listed windows refuse unless opted in)
            dimg = eng.tokenize_input_bwd(src, None, dx0, emb_drop=ctx.emb_drop)
            if src.sink is not None:   # the sink holds the fold: autograd gets no gradient for the scene
                dimg = None
        if any(needs):   # (a fully frozen model: the tokenizer backward writes parameter gradients only, nobody reads them)
            eng.tokenize_bwd(src, None, dx0, emb_drop=ctx.emb_drop)
        return (None,) * 5 + (dimg,) + _grad_views(eng, ctx.names, needs)


class _HeadOnlyFn(torch.autograd.Function):
    """logits = head(y) over the output y of a frozen body (linear evaluation): the stash is y alone, the backward is the head
    backward without dy (nobody consumes it) and returns gradients for the head parameters only."""

    @staticmethod
    def forward(ctx, eng, names, y, *params):
        ctx.eng, ctx.names = eng, names
        ctx.stash = (y,)
        return eng.head_logits(y)

    @staticmethod
    def backward(ctx, dlogits):
        eng = ctx.eng
        (y,) = ctx.stash
        ctx.stash = None
        needs = ctx.needs_input_grad[3:]
        _refuse_accumulation(eng, ctx.names, needs)
        eng.head_logits_bwd(y, dlogits.contiguous().float(), want_dy=False)
        return (None, None, None) + _grad_views(eng, ctx.names, needs)
