"""The operand layouts of ``msst_prep_weights`` restated on the CPU (numpy / torch), written from the contract -- include/msst.h
(MsstPrepJob), DESIGN.md "Operand copies" and the readers (``PBF16::ld_w`` in msst_dev.h, ``ld_w32`` in msst_bwd3.hip): the reference
of tests/test_gpu_prep_weights.py, itself checked in tests/test_prep_weights_host.py.

A job turns an fp32 source [rows][cols] into the logical destination [R][K] = [rows][cols], or [cols][rows] when transposed.
  * the first ``scale_rows`` SOURCE rows are multiplied by ``scale`` in fp32, then every value is rounded ONCE, to nearest even, to the
    destination type (torch's CPU ``.to(torch.bfloat16)`` / ``.to(torch.float16)``; fp32: no rounding);
  * fp32 destinations are plain row-major [R][K];
  * 2-byte destinations (bf16, IEEE half) are 1-KB fragments of 512 elements, fragment after fragment:
      pack 0: f = (r / 16) (K / 32) + k / 32, lane l = (k % 32 / 8) 16 + r % 16 holds the 8 consecutive k from 8 (k % 32 / 8)
      pack 1: f = (r / 32) (K / 16) + k / 16, lane l = (k % 16 / 8) 32 + r % 32
    element (r, k) at (f 64 + l) 8 + k % 8.  Only whole fragments exist: R % 16 == 0 and K % 32 == 0 (pack 0), R % 32 == 0 and
    K % 16 == 0 (pack 1).
"""
import numpy as np
import torch

ELEMS = {"f32": (torch.float32, np.int32), "bf16": (torch.bfloat16, np.int16), "f16": (torch.float16, np.int16)}
FRAG = 512   # elements of one 1-KB fragment

# (rows, cols, transpose) of the SOURCE: the smallest shapes at which each mechanism exists (one fragment, two fragment columns, three
# of each with R != K, more fragment rows than columns; a transposed single fragment and a transposed R != K) ...
SHAPES_PACK0 = [(16, 32, 0), (32, 64, 0), (48, 96, 0), (96, 64, 0), (32, 16, 1), (64, 96, 1)]
SHAPES_PACK1 = [(32, 16, 0), (64, 48, 0), (16, 32, 1), (96, 64, 1)]
# ... to_qkv at 2 and 8 heads (147456 elements: more than the 64 workgroups of one launch cover in one pass), every pack and orientation
SHAPES_REAL = [(rows, 96, tr, pk) for rows in (384, 1536) for tr in (0, 1) for pk in (0, 1)]
SHAPES_F32 = [(1, 1), (5, 7), (96, 64)]
# 2-byte destinations with pack 0 that are not whole 16 x 32 fragments: refused (flag 2), nothing written
SHAPES_PARTIAL0 = [(8, 32, 0), (17, 32, 0), (16, 8, 0), (16, 36, 0), (16, 40, 0), (20, 7, 0), (32, 8, 1)]


def logical_shape(rows, cols, transpose):
    return (cols, rows) if transpose else (rows, cols)


def whole_fragments(R, K, pack):
    RB, KB = (32, 16) if pack else (16, 32)
    return R > 0 and K > 0 and R % RB == 0 and K % KB == 0


def frag_index(R, K, pack):
    """int64 [R, K]: the position of logical element (r, k) in a fragment-packed destination"""
    if not whole_fragments(R, K, pack):
        raise ValueError(f"[{R}][{K}] is not whole fragments of pack {pack}")
    RB, KB = (32, 16) if pack else (16, 32)
    r, k = np.arange(R, dtype=np.int64)[:, None], np.arange(K, dtype=np.int64)[None, :]
    f = (r // RB) * (K // KB) + k // KB
    lane = (k % KB // 8) * RB + r % RB
    return (f * 64 + lane) * 8 + k % 8


def scaled(src, scale_rows, scale):
    """src [rows, cols] fp32 with its first scale_rows rows multiplied by fp32(scale), the product in fp32"""
    assert src.dtype == torch.float32 and src.dim() == 2
    v = src.clone()
    n = max(0, min(int(scale_rows), v.shape[0]))
    if n:
        v[:n] = v[:n] * torch.tensor(float(scale), dtype=torch.float32)
    return v


def pack(src, transpose, pack, scale_rows, scale, elem):
    """the expected destination of one job as bits: int16 [rows cols] (elem "bf16" / "f16") or int32 [rows cols] ("f32")"""
    tdt, ndt = ELEMS[elem]
    v = scaled(src, scale_rows, scale)
    logical = (v.t() if transpose else v).contiguous()
    R, K = logical.shape
    if elem == "f32":
        return logical.view(torch.int32).numpy().reshape(-1).copy()
    bits = logical.to(tdt).view(torch.int16).numpy()
    out = np.empty(R * K, dtype=ndt)
    out[frag_index(R, K, pack & 1).reshape(-1)] = bits.reshape(-1)
    return out


def unpack(dst, rows, cols, transpose, pack, elem):
    """inverse of pack(): destination bits -> fp32 [rows, cols] in the SOURCE orientation (the values as stored: scaled and rounded)"""
    tdt, ndt = ELEMS[elem]
    R, K = logical_shape(rows, cols, transpose)
    dst = np.asarray(dst)
    assert dst.dtype == ndt and dst.shape == (R * K,)
    if elem == "f32":
        logical = torch.from_numpy(dst.copy()).view(torch.float32).reshape(R, K)
    else:
        bits = dst[frag_index(R, K, pack & 1)]
        logical = torch.from_numpy(np.ascontiguousarray(bits)).view(tdt).float()
    return (logical.t() if transpose else logical).contiguous()


# ---- an independent round-to-nearest-even on the fp32 bit pattern, in Python integers ----
def rne_bits(u, mbits):
    """fp32 bit pattern u -> the bit pattern of the nearest value (ties to even) of the 16-bit format with `mbits` mantissa bits
    (7: bf16, 8 exponent bits; 10: IEEE half, 5 exponent bits).  NaN -> a quiet NaN of the same sign."""
    ebits = 15 - mbits
    bias = (1 << (ebits - 1)) - 1
    inf = ((1 << ebits) - 1) << mbits
    s, e, m = (u >> 31) & 1, (u >> 23) & 0xFF, u & 0x7FFFFF
    if e == 255:
        return (s << 15) | inf | ((1 << (mbits - 1)) if m else 0)
    sig, ex = (m, -149) if e == 0 else (m | 0x800000, e - 150)        # |value| = sig 2^ex
    if sig == 0:
        return s << 15
    E = max(ex + sig.bit_length() - 1, 1 - bias)                       # exponent of the value, held at the smallest normal one
    shift = (E - mbits) - ex                                           # the target's ulp is 2^(E - mbits): >= 1 bit of fp32 goes
    q, rem, tie = sig >> shift, sig & ((1 << shift) - 1), 1 << (shift - 1)
    if rem > tie or (rem == tie and (q & 1)):
        q += 1
    # q < 2^mbits: subnormal (E is the smallest normal exponent, the exponent field is 0); a carry walks into the exponent by itself
    out = ((E + bias - 1) << mbits) + q
    return (s << 15) | min(out, inf)


def is_nan16(bits, elem):
    mb = 7 if elem == "bf16" else 10
    b = np.asarray(bits).astype(np.int64) & 0x7FFF
    inf = ((1 << (15 - mb)) - 1) << mb
    return b > inf


def is_nan32(bits):
    return (np.asarray(bits).astype(np.int64) & 0x7FFFFFFF) > 0x7F800000


# ---- fills ----
def _from_bits(u):
    return torch.from_numpy(np.asarray(u, dtype=np.uint32).view(np.int32).copy()).view(torch.float32)


# exponent ranges of the distinct fill: normal in the destination type, and still normal (so still exact) after a scale of 2^-3
_DISTINCT = {"bf16": (7, -100, 100), "f16": (10, -11, 15)}


def fill_distinct(rows, cols, elem):
    """fp32 [rows, cols] of values that are exact in the destination type and pairwise distinct: element i = r cols + c takes the i-th
    of the type's values (mantissa fastest, then the exponent over the range above, then the sign).  M values of one sign: 25727
    (bf16) / 27647 (half), so up to 2 M = 51454 / 55294 elements are pairwise distinct -- every shape but (1536, 96), whose 147456
    elements outnumber the finite values of a 16-bit type: there a value returns after 2 M elements, an odd count times two, which is
    no multiple of a row (96, 1536), a lane (8) or a fragment (512).  fp32: distinct normal values 4099 ulps apart."""
    i = np.arange(rows * cols, dtype=np.int64)
    if elem == "f32":
        return _from_bits((0x30000000 + i * 4099).astype(np.uint32) | ((i & 1) << 31).astype(np.uint32)).reshape(rows, cols)
    mb, e0, e1 = _DISTINCT[elem]
    M = (e1 - e0 + 1) * (1 << mb) - 1
    j = i % M
    mant, exp = j % (1 << mb), j // (1 << mb) + e0
    sign = (i // M) % 2
    u = (sign << 31) | ((exp + 127) << 23) | (mant << (23 - mb))
    return _from_bits(u.astype(np.uint32)).reshape(rows, cols)


def fill_random(rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    return 0.05 * torch.randn(rows, cols, generator=g)


def _both_signs(bits):
    return [b for u in bits for b in (u, u | 0x80000000)]


def _f(x):
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


# fp32 bit patterns, no fp32 denormals among them (those are DENORMALS): zeros, infinities, NaNs of two payloads ...
SPECIAL_COMMON = _both_signs([0x00000000, 0x7F800000, 0x7FC00000, 0x7F800001, _f(1.0), _f(3.0)])
SPECIAL = {
    # ... exact ties of bf16 in both directions (1 + 2^-8 -> 1, 1 + 3 2^-8 -> 1 + 2^-6), one ulp of fp32 either side of a tie, the
    # largest fp32 values: FLT_MAX and the tie 0x7F7F8000 round to bf16 inf, 0x7F7F7FFF is the last that stays finite; the smallest
    # normal fp32 value (2^-126)
    "bf16": SPECIAL_COMMON + _both_signs([_f(1 + 2.0 ** -8), _f(1 + 3 * 2.0 ** -8), _f(1 + 2.0 ** -8) + 1, _f(1 + 2.0 ** -8) - 1,
                                          _f(1 + 3 * 2.0 ** -8) + 1, _f(1 + 3 * 2.0 ** -8) - 1, 0x7F7FFFFF, 0x7F7F8000, 0x7F7F7FFF, 0x00800000]),
    # ... exact ties of half (1 + 2^-11 -> 1, 1 + 3 2^-11 -> 1 + 2^-9) and their fp32 neighbours; 65504 (largest half), 65519.996 (the
    # last value below the tie: stays 65504), 65520 (tie -> inf), 1e6; subnormal results 1e-6, 6e-8, 2^-24 (smallest), 3 2^-25 (tie
    # -> 2^-23), 2^-25 (tie -> 0), the value after it (-> 2^-24), 2^-14 (smallest normal half) and the value before it, FLT_MAX
    "f16": SPECIAL_COMMON + _both_signs([_f(1 + 2.0 ** -11), _f(1 + 3 * 2.0 ** -11), _f(1 + 2.0 ** -11) + 1, _f(1 + 2.0 ** -11) - 1,
                                         _f(1 + 3 * 2.0 ** -11) + 1, _f(1 + 3 * 2.0 ** -11) - 1, _f(65504.0), _f(65520.0) - 1, _f(65520.0),
                                         _f(1e6), _f(1e-6), _f(6e-8), _f(2.0 ** -24), _f(3 * 2.0 ** -25), _f(2.0 ** -25), _f(2.0 ** -25) + 1,
                                         _f(2.0 ** -14), _f(2.0 ** -14) - 1, 0x7F7FFFFF]),
}
SPECIAL["f32"] = sorted(set(SPECIAL["bf16"] + SPECIAL["f16"]))
# fp32 DENORMAL inputs: 2^-127 .. 2^-130 and odd patterns between (a bf16 result keeps a non-zero subnormal even after a scale of 0.5;
# a half result is a zero either way), the largest and the smallest denormal
DENORMALS = _both_signs([0x00400000, 0x007FFFFF, 0x00200000, 0x00123456, 0x00080000, 0x00654321, 0x00000001])


def fill_cycle(bits, rows, cols):
    """fp32 [rows, cols]: the given bit patterns over and over, so that every one of them meets several lanes and positions (a list
    whose length shares a factor with the row length gets 0.5s appended until it does not: each pattern then walks through all k)"""
    n = rows * cols
    bits = list(bits)
    while np.gcd(len(bits), cols) != 1:
        bits.append(_f(0.5))
    assert n >= len(bits)
    return _from_bits(np.resize(np.asarray(bits, dtype=np.uint32), n)).reshape(rows, cols)
