// What the kernels on frozen per-pixel features share (msst_knn.hip, msst_probe.hip, msst_kmeans.hip, msst_pca.hip, msst_gauss.hip): rows x [M][96] fp32, or an
// encode_scene map [Bs][96][plane] read in place, walked in tiles of 64 rows by workgroups of 256 threads = 4 waves, with one score per
// (row, class) on v_mfma_f32_16x16x4_f32.  Every rule that these files must agree on to keep their bits lives here, once:
//   zero rows   a row past the end of the walk is loaded as zeros (never as garbage) and masked by index by the caller.
//   tile        rows layout: piece e = tid + 256 i of the tile's 64 x 24 16-byte pieces, row e / 24, channels 4 (e % 24) ..; one 16-byte
//               global load per piece, held in registers (f32x4 pre[6]) so that a tile is fetched while the one before is computed on.
//               Map layout: thread = (row tid & 63, channels 4 i + (tid >> 6)), the 64 lanes of a wave on 64 adjacent pixels of one
//               channel plane; the same 24 registers.  The LDS pitch is the caller's: 98 (= 2 mod 32: the 32 lanes of a one-dword operand
//               read on 32 banks; rows start on 8 bytes, stored as two float2) or a multiple of 4 (16-byte rows, one f32x4 store).
//   centre      c = x - centre in fp32 on the registers of a prefetched tile, and the flags of a stored tile (a channel that is not finite;
//               past the end), four threads per row: msst_pca.hip and msst_gauss.hip.
//   scores      wave w owns rows 16 w .. 16 w + 15: A = x[16 w + (l & 15)][4 ks + (l >> 4)], B = w[16 jt + (l & 15)][4 ks + (l >> 4)], 24
//               k-steps ascending, so a score is the fp32 fmaf chain over d = 0 .. 95 in order behind the accumulator's start value;
//               lane l then holds rows 4 (l >> 4) + r, classes 16 jt + (l & 15).
//   order       ONE total order: value descending, then index ascending.
//   pairs       the NCT x 6 (class tile, channel tile) accumulators of a [class][channel] product are dealt round-robin to the 4 waves.
//   partition   rows over workgroups of whole tiles, from the row count alone.
// What differs between them (kNN's query fragments and top-k lists, the probe's LayerNorm and softmax, the accumulation loops, the
// centring and the 21 symmetric pairs of msst_pca.hip) stays in its own file.  No helper takes a flag that says which caller it serves.  No inline assembly.
#pragma once
#include "msst_dev.h"

#include <atomic>
#include <type_traits>

namespace msst {

constexpr int FEAT_D = 96;             // the feature width
constexpr int FEAT_TILE = 64;          // rows per tile
constexpr int FEAT_THREADS = 256;      // 4 waves
constexpr int FEAT_MAX_WGS = 512;      // 256 CUs x 2: every CU busy with two workgroups, and a slab of per-workgroup partials stays small

// ---- tile loader, rows layout [M][96]: rows r0 .. r0 + 63, zero from rend on
__device__ __forceinline__ void feat_rows_prefetch(f32x4 (&pre)[6], const float* x, long r0, long rend, int tid) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const int e = tid + FEAT_THREADS * i;
        const int row = e / 24, c4 = e - row * 24;
        const long r = r0 + row;
        pre[i] = r < rend ? *reinterpret_cast<const f32x4*>(x + r * FEAT_D + 4 * c4) : zero4();
    }
}

template <int PITCH>
__device__ __forceinline__ void feat_rows_store(float* xs, const f32x4 (&pre)[6], int tid) {
    static_assert(PITCH % 2 == 0, "LDS rows start on 8 bytes at least");
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const int e = tid + FEAT_THREADS * i;
        const int row = e / 24, c4 = e - row * 24;
        float* d = xs + row * PITCH + 4 * c4;
        if constexpr (PITCH % 4 == 0) {
            *reinterpret_cast<f32x4*>(d) = pre[i];
        } else {
            *reinterpret_cast<float2*>(d) = make_float2(pre[i][0], pre[i][1]);
            *reinterpret_cast<float2*>(d + 2) = make_float2(pre[i][2], pre[i][3]);
        }
    }
}

// ---- tile loader, map layout [Bs][96][plane]: row q = b plane + p reads (b 96 + d) plane + p
__device__ __forceinline__ void feat_map_prefetch(f32x4 (&pre)[6], const float* x, long plane, long r0, long rend, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    const long q = r0 + lane;
    const bool in = q < rend;
    const long b = in ? q / plane : 0, p = in ? q - b * plane : 0;
    const float* src = x + b * FEAT_D * plane + p;
#pragma unroll
    for (int i = 0; i < 24; ++i) pre[i >> 2][i & 3] = in ? src[(long)(4 * i + wave) * plane] : 0.f;
}

template <int PITCH>
__device__ __forceinline__ void feat_map_store(float* xs, const f32x4 (&pre)[6], int tid) {
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int i = 0; i < 24; ++i) xs[lane * PITCH + 4 * i + wave] = pre[i >> 2][i & 3];
}

// ---- c = x - centre on the registers of a prefetched tile (scen: [96] in LDS, 16-byte aligned), formed in fp32 before any product
__device__ __forceinline__ void feat_centre_rows(f32x4 (&pre)[6], const float* scen, int tid) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const int e = tid + FEAT_THREADS * i;
        const int c4 = e - (e / 24) * 24;
        pre[i] -= *reinterpret_cast<const f32x4*>(scen + 4 * c4);
    }
}

__device__ __forceinline__ void feat_centre_map(f32x4 (&pre)[6], const float* scen, int tid) {
    const int wave = tid >> 6;
#pragma unroll
    for (int i = 0; i < 24; ++i) pre[i >> 2][i & 3] -= scen[4 * i + wave];
}

// ---- four threads per row of a stored tile: flag 0 = counted, 1 = a channel is not finite, 2 = at or past rend; a flagged row is zeroed
template <int PITCH>
__device__ __forceinline__ void feat_flag_rows(float* xs, int* sflag, long r0, long rend, int tid) {
    float* xr = xs + (tid >> 2) * PITCH + (tid & 3);
    int bad = 0;
#pragma unroll
    for (int i = 0; i < 24; ++i) bad |= !(fabsf(xr[4 * i]) <= 3.4028234e38f) ? 1 : 0;
    bad |= __shfl_xor(bad, 1);
    bad |= __shfl_xor(bad, 2);
    const int flag = r0 + (tid >> 2) >= rend ? 2 : bad;
    if (flag) {
#pragma unroll
        for (int i = 0; i < 24; ++i) xr[4 * i] = 0.f;
    }
    if ((tid & 3) == 0) sflag[tid >> 2] = flag;
}

// ---- scores of the wave's 16 rows x 16 NCT classes, added to c as the caller initialised it
template <int NCT, int XP, int WP>
__device__ __forceinline__ void feat_scores(const float* xs, const float* ws, int wave, int cc, int cg, f32x4 (&c)[NCT]) {
    const float* xa = xs + (16 * wave + cc) * XP + cg;
    const float* wb = ws + cc * WP + cg;
#pragma unroll
    for (int ks = 0; ks < 24; ++ks) {
        const float a = xa[4 * ks];
#pragma unroll
        for (int jt = 0; jt < NCT; ++jt) c[jt] = PF32::mma(a, wb[16 * jt * WP + 4 * ks], c[jt]);
    }
}

// ---- the total order: (s, i) ranks before (es, ei)
__device__ __forceinline__ bool feat_ahead(float s, int i, float es, int ei) { return s > es || (s == es && i < ei); }

// the first (value, index) under the order over the 16 lanes of a group (xor 1, 2, 4, 8)
__device__ __forceinline__ void feat_group_argmax(float& bv, int& bi) {
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) {
        const float ov = __shfl_xor(bv, m);
        const int oi = __shfl_xor(bi, m);
        if (feat_ahead(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
}

__device__ __forceinline__ float feat_group_sum(float v) {
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 8);
    return v;
}

// ---- (class tile, channel tile) pairs: pair p = wave + 4 i is (p / 6, p % 6)
__host__ __device__ constexpr int feat_pairs_per_wave(int nct) { return (nct * 6 + 3) / 4; }

template <int NCT>
__device__ __forceinline__ bool feat_wave_pair(int wave, int i, int& it, int& jt) {   // false: the wave has no i-th pair
    const int p = wave + 4 * i;
    it = p / 6;
    jt = p - it * 6;
    return p < NCT * 6;
}

// a wave's accumulators (lane l holds classes 16 it + 4 (l >> 4) + r, channel 16 jt + (l & 15)) to a table [class][channel]; classes
// from nrows on are not stored
template <int NCT, int PITCH>
__device__ __forceinline__ void feat_store_pairs(float* tab, const f32x4 (&acc)[feat_pairs_per_wave(NCT)], int nrows, int wave, int cc, int cg) {
#pragma unroll
    for (int i = 0; i < feat_pairs_per_wave(NCT); ++i) {
        int it, jt;
        if (feat_wave_pair<NCT>(wave, i, it, jt)) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int cls = 16 * it + 4 * cg + r;
                if (cls < nrows) tab[cls * PITCH + 16 * jt + cc] = acc[i][r];
            }
        }
    }
}

// ---- an LDS table [64][pitch] of the workgroup's rows q0 .. q0 + nq - 1 by all NT threads: as rows [Q][nc] (layout 0, consecutive
// threads on consecutive floats) or as a map [Bs][nc][plane] (layout 1, thread = (row tid & 63, classes (tid >> 6) + (NT / 64) i))
template <int NT>
__device__ __forceinline__ void feat_store_table(const float* tab, int pitch, float* out, int layout, long q0, long nq, int nc, long plane,
                                                 int tid) {
    if (layout == 0) {
        for (long e = tid; e < nq * nc; e += NT) {
            const int ql = (int)(e / nc), cl = (int)(e - (long)ql * nc);
            out[q0 * nc + e] = tab[ql * pitch + cl];
        }
    } else {
        const int row = tid & 63;
        if (row < nq) {
            const long q = q0 + row;
            const long b = q / plane, p = q - b * plane;
            for (int cl = tid >> 6; cl < nc; cl += NT / 64) out[(b * nc + cl) * plane + p] = tab[row * pitch + cl];
        }
    }
}

// ---- host side
// rows over workgroups of whole tiles; depends on the row count only, so every launch over the same rows agrees on it
inline void feat_partition(long rows, long* tiles_per_wg, int* nwg) {
    const long tiles = (rows + FEAT_TILE - 1) / FEAT_TILE;
    const long per = (tiles + FEAT_MAX_WGS - 1) / FEAT_MAX_WGS;
    *tiles_per_wg = per;
    *nwg = (int)((tiles + per - 1) / per);
}

// class (or cluster) tiles of 16 a kernel is instantiated for: n rounded up to 16, 32, 64 or 128
inline int feat_nct(int n) { return n <= 16 ? 1 : n <= 32 ? 2 : n <= 64 ? 4 : 8; }

// f(std::integral_constant<int, NCT>) for the NCT of n
template <class F>
int feat_dispatch_nct(int n, F&& f) {
    switch (feat_nct(n)) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 4: return f(std::integral_constant<int, 4>{});
        default: return f(std::integral_constant<int, 8>{});
    }
}

// allow a kernel `bytes` of dynamic LDS, once per kernel: 0 or the HIP error
template <auto Kernel>
int feat_allow_lds(size_t bytes) {
    static std::atomic<bool> done{false};
    if (!done) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return (int)e;
        done = true;
    }
    return 0;
}

}  // namespace msst
