// SLIC superpixels of an encode_scene feature map and object-based class maps (msst_slic_assign, msst_slic_update, msst_slic_pool,
// msst_slic_pool_finish, msst_slic_broadcast; maskedsst_amd/superpixel.py): the grid form of SLIC (gSLICr) on a map [Bs][96][Hs][Ws] read
// in place, and the per-superpixel means of any map [Bs][C][Hs][Ws], C <= 128.  fp32, no inline assembly, no float atomics: every output
// has the same bits in every call, and a fixed point (an iteration that moves no pixel) reproduces itself bit for bit.
//
// From msst_feat.h: the feature width, the `scores` rule (a dot is the fp32 fmaf chain over d = 0 .. 95 on v_mfma_f32_16x16x4_f32, operands
// at LDS pitch 98), feat_map_store and feat_flag_rows on the registers and the LDS rows of a 64-row tile, and the one total order
// (feat_ahead, feat_group_argmax).  The 64 rows of a tile are the 8 x 8 pixels of a BLOCK aligned to 8, row = 8 ly + lx; the loader that
// fetches a block of each channel plane (eight 32-byte segments per channel per wave) is this file's.
//
// Grid: step S in {4, 8, 16}; cell (i, j) owns rows [i S, (i + 1) S) and columns [j S, (j + 1) S) of its scene; superpixel id = i gx + j,
// gy = ceil(Hs / S), gx = ceil(Ws / S).  A block lies in one cell (S = 8, 16) or touches 2 x 2 cells (S = 4); the union of its pixels'
// 3 x 3 candidate cells is the WINDOW of the block: NW x NW cells from (8 by / S - 1, 8 bx / S - 1), NW = 3 (S = 8, 16) or 4 (S = 4), at
// most 16 SLOTS, slot = si NW + sj.  Slot order is id order, so the total order over slots is the total order over ids.
//
// slic_assign    one workgroup of 256 threads = 4 waves per block.  LDS: the window's centroids [16][98] (a slot outside the grid: a zero
//                row) | the block's features [64][98] | [ly, lx, 1, 0 ..] [64][16] | flags, slots.
//   live         in the scene, the 96 features finite (feat_flag_rows zeroes the others: 0 x NaN would poison the sums), cover null or > 0.
//   scores       feat_scores<1>: wave w owns rows 16 w .., lane l holds rows 4 (l >> 4) + r against slot l & 15.  Per lane the slot's
//                bias, offset and count; dy = (float)(y - ci S) - off_y (the integer is the cell difference times S plus the pixel's place
//                in its cell: small, exact), dx alike; s = fmaf(-hl, fmaf(dy, dy, dx dx), dot + bias).  A slot that is outside the grid,
//                has count 0 or lies outside the pixel's own 3 x 3 cells is masked; feat_group_argmax over the 16 lanes of the group.
//   home         (centroids == null: iteration 0) every live pixel takes its own cell; no scores.
//   best         (best != null) the winning score of a labelled pixel, NaN for label -1 and in the home mode.
//   moved        pixels whose label differs from prev_labels (which may be the labels buffer itself: a pixel reads its own entry before
//                it writes it): one integer atomic per wave.
//   sums         (slab != null) onehot^T [x | ly, lx, 1] on the same MFMA: A = (slot[row 4 ks + (l >> 4)] == l & 15) ? 1 : 0, B = the
//                row's channel; the 6 + 1 column tiles dealt round-robin to the 4 waves; the block's [16][99] partials go to its slab row
//                (every entry is written, zeros included).
// slic_update    one workgroup per centre, thread = column: the slab entries of the blocks whose window holds the centre's cell (4 at
//                S = 4, 9 at S = 8, 36 at S = 16, fewer at a border), by ascending, then bx ascending -- an order that depends on (Hs, Ws,
//                S) alone.  The offset columns are whole numbers (a block's sum of ly plus its count times the block's row offset from
//                the cell's origin), exact in fp32.  count > 0: centroid = sum / count, offset = sum / count (one IEEE division each),
//                bias = -0.5 x the fmaf chain of c[d]^2 from zero.  count == 0: count 0, everything else kept; `empty` counts these.
// slic_pool      one workgroup per block: the block of every channel plane to LDS [64][C | 1]; thread = (channel, half of the block):
//                acc[half][slot][c] += v in pixel order -- a selection, never a product with 0, so that a -inf score pools to -inf and
//                stays in its own superpixel; the block's partial is acc[0] + acc[1].  A label outside the block's window (no fit gives
//                one) contributes to no sum.
// slic_pool_finish  as slic_update: table = sum / count, NaN for count 0; region class = the first largest entry above -inf, else -1.
// slic_broadcast classes[p] = region_classes[label[p]], -1 for a label outside [0, n_sp).
#include "../../include/msst.h"
#include "msst_feat.h"
#include "msst_kernels.h"

namespace msst {

namespace {

constexpr int SL_P = 98;                       // LDS pitch of a feature row and of a centroid row
constexpr int SL_AUX = 16;                     // [ly, lx, 1, 0 ..]: the 7th column tile
constexpr int SL_COLS = FEAT_D + 3;            // a slab row of the fit: 96 feature sums | sum ly | sum lx | count
constexpr int SL_NONE = 0x7fffffff;

struct SlicGeo {
    int Bs, Hs, Ws, S, gy, gx, nby, nbx, NW;
    __host__ __device__ long plane() const { return (long)Hs * Ws; }
    __host__ __device__ int nsp() const { return gy * gx; }
    __host__ __device__ long blocks() const { return (long)Bs * nby * nbx; }
};

SlicGeo slic_geo(int Bs, int Hs, int Ws, int S) {
    SlicGeo g;
    g.Bs = Bs; g.Hs = Hs; g.Ws = Ws; g.S = S;
    g.gy = (Hs + S - 1) / S; g.gx = (Ws + S - 1) / S;
    g.nby = (Hs + 7) / 8; g.nbx = (Ws + 7) / 8;
    g.NW = S == 4 ? 4 : 3;
    return g;
}

// f(block index within the scene, slot) over the blocks whose window holds cell (i, j): by ascending, then bx ascending
template <class F>
__device__ __forceinline__ void slic_for_blocks(const SlicGeo& g, int i, int j, F&& f) {
    const int S = g.S, NW = g.NW;
    const int by_lo = max(0, ((i - NW + 2) * S + 7) / 8 - 1), by_hi = min(g.nby - 1, ((i + 2) * S - 1) / 8);
    const int bx_lo = max(0, ((j - NW + 2) * S + 7) / 8 - 1), bx_hi = min(g.nbx - 1, ((j + 2) * S - 1) / 8);
    for (int by = by_lo; by <= by_hi; ++by) {
        const int si = i - (8 * by / S - 1);
        if (si < 0 || si >= NW) continue;
        for (int bx = bx_lo; bx <= bx_hi; ++bx) {
            const int sj = j - (8 * bx / S - 1);
            if (sj < 0 || sj >= NW) continue;
            f(by, bx, si * NW + sj);
        }
    }
}

struct SlicBlock {
    int b, by, bx, y0, x0, ci0, cj0;
};

__device__ __forceinline__ SlicBlock slic_block(const SlicGeo& g) {
    SlicBlock k;
    int t = blockIdx.x;
    k.bx = t % g.nbx;
    t /= g.nbx;
    k.by = t % g.nby;
    k.b = t / g.nby;
    k.y0 = 8 * k.by; k.x0 = 8 * k.bx;
    k.ci0 = k.y0 / g.S - 1; k.cj0 = k.x0 / g.S - 1;
    return k;
}

struct SlicAssignArgs {
    const float* feat;
    const int32_t* cover;
    const float* cent;        // null: home mode
    const float* off;
    const float* bias;
    const int32_t* counts;
    int64_t* labels;
    const int64_t* prev;
    int32_t* moved;
    float* best;
    float* slab;
    SlicGeo g;
    float hl;
};

__global__ __launch_bounds__(256) void slic_assign_kernel(SlicAssignArgs a) {
    __shared__ __attribute__((aligned(16))) float sc[16 * SL_P];
    __shared__ __attribute__((aligned(16))) float xs[64 * SL_P];
    __shared__ float saux[64 * SL_AUX];
    __shared__ int sflag[64];
    __shared__ int sslot[64];
    const SlicGeo& g = a.g;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cg = lane >> 4, cc = lane & 15;
    const SlicBlock k = slic_block(g);
    const int S = g.S, NW = g.NW, nsp = g.nsp();
    const long plane = g.plane();
    const bool home = a.cent == nullptr;

    // ---- the window's centroids; [ly, lx, 1, 0 ..]
    if (!home) {
        for (int e = tid; e < 16 * FEAT_D; e += 256) {
            const int slot = e / FEAT_D, d = e - slot * FEAT_D;
            const int ci = k.ci0 + slot / NW, cj = k.cj0 + slot % NW;
            const bool ok = slot < NW * NW && ci >= 0 && ci < g.gy && cj >= 0 && cj < g.gx;
            sc[slot * SL_P + d] = ok ? a.cent[((long)k.b * nsp + ci * g.gx + cj) * FEAT_D + d] : 0.f;
        }
    }
    for (int e = tid; e < 64 * SL_AUX; e += 256) {
        const int row = e >> 4, col = e & 15;
        saux[e] = col == 0 ? (float)(row >> 3) : col == 1 ? (float)(row & 7) : col == 2 ? 1.0f : 0.f;
    }
    // ---- the block of every channel plane: lane = pixel (lane >> 3, lane & 7), channels 4 i + wave; outside the scene: zeros
    {
        const int y = k.y0 + (lane >> 3), x = k.x0 + (lane & 7);
        const bool in = y < g.Hs && x < g.Ws;
        const float* src = a.feat + (long)k.b * FEAT_D * plane + (in ? (long)y * g.Ws + x : 0);
        f32x4 pre[6];
#pragma unroll
        for (int i = 0; i < 24; ++i) pre[i >> 2][i & 3] = in ? src[(long)(4 * i + wave) * plane] : 0.f;
        feat_map_store<SL_P>(xs, pre, tid);
    }
    __syncthreads();
    feat_flag_rows<SL_P>(xs, sflag, 0, 64, tid);
    __syncthreads();

    f32x4 c[1] = {zero4()};
    if (!home) feat_scores<1, SL_P, SL_P>(xs, sc, wave, cc, cg, c);

    // ---- the lane's slot
    const int ci = k.ci0 + cc / NW, cj = k.cj0 + cc % NW;
    bool slot_ok = false;
    float oy = 0.f, ox = 0.f, bs = 0.f;
    if (!home && cc < NW * NW && ci >= 0 && ci < g.gy && cj >= 0 && cj < g.gx) {
        const long id = (long)k.b * nsp + ci * g.gx + cj;
        slot_ok = a.counts[id] > 0;
        oy = a.off[2 * id];
        ox = a.off[2 * id + 1];
        bs = a.bias[id];
    }
    int nmoved = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int rl = 16 * wave + 4 * cg + r;
        const int y = k.y0 + (rl >> 3), x = k.x0 + (rl & 7);
        const bool in = y < g.Hs && x < g.Ws;
        const long p = (long)k.b * plane + (long)y * g.Ws + x;
        bool live = in && sflag[rl] == 0;
        if (live && a.cover) live = a.cover[p] > 0;
        const int pi = y / S, pj = x / S;
        float bv = -__builtin_inff();
        int bi = SL_NONE;
        if (home) {
            bi = (pi - k.ci0) * NW + (pj - k.cj0);
        } else {
            const int di = ci - pi, dj = cj - pj;
            if (slot_ok && di >= -1 && di <= 1 && dj >= -1 && dj <= 1) {
                const float dy = (float)(y - ci * S) - oy, dx = (float)(x - cj * S) - ox;
                bv = fmaf(-a.hl, fmaf(dy, dy, dx * dx), c[0][r] + bs);
                bi = cc;
            }
            feat_group_argmax(bv, bi);
        }
        const int slot = live && bi != SL_NONE ? bi : -1;
        if (cc == 0) {
            if (in) {
                const int64_t label = slot < 0 ? -1 : (int64_t)(k.ci0 + slot / NW) * g.gx + (k.cj0 + slot % NW);
                if (a.prev && a.prev[p] != label) ++nmoved;
                a.labels[p] = label;
                if (a.best) a.best[p] = slot < 0 || home ? __builtin_nanf("") : bv;
            }
            sslot[rl] = slot;
        }
    }
    if (a.moved) {   // uniform
        nmoved += __shfl_xor(nmoved, 16);
        nmoved += __shfl_xor(nmoved, 32);
        if (lane == 0 && nmoved) atomicAdd(a.moved, nmoved);
    }
    if (!a.slab) return;   // uniform
    __syncthreads();

    // ---- the block's partial sums: onehot^T [x | ly, lx, 1]; column tile p = wave + 4 i of 7
    f32x4 acc[2] = {zero4(), zero4()};
#pragma unroll 4
    for (int ks = 0; ks < 16; ++ks) {
        const int row = 4 * ks + cg;
        const float one = sslot[row] == cc ? 1.0f : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int p = wave + 4 * i;
            if (p < 7) acc[i] = PF32::mma(one, p < 6 ? xs[row * SL_P + 16 * p + cc] : saux[row * SL_AUX + cc], acc[i]);
        }
    }
    float* out = a.slab + (long)blockIdx.x * (16 * SL_COLS);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int col = 16 * (wave + 4 * i) + cc;
        if (col < SL_COLS) {
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(4 * cg + r) * SL_COLS + col] = acc[i][r];
        }
    }
}

struct SlicUpdateArgs {
    const float* __restrict__ slab;
    float* cent;
    float* off;
    float* bias;
    int32_t* counts;
    int32_t* empty;
    SlicGeo g;
};

__global__ __launch_bounds__(128) void slic_update_kernel(SlicUpdateArgs a) {
    __shared__ float ssum[SL_COLS];
    __shared__ float snew[FEAT_D];
    const SlicGeo& g = a.g;
    const int tid = threadIdx.x;
    const int nsp = g.nsp();
    const int b = blockIdx.x / nsp, kk = blockIdx.x - b * nsp;
    const int i = kk / g.gx, j = kk - i * g.gx;
    if (tid < SL_COLS) {
        float s = 0.f;
        slic_for_blocks(g, i, j, [&](int by, int bx, int slot) {
            const float* row = a.slab + ((((long)b * g.nby + by) * g.nbx + bx) * 16 + slot) * SL_COLS;
            float v = row[tid];
            if (tid == FEAT_D) v += row[FEAT_D + 2] * (float)(8 * by - i * g.S);        // whole numbers below 2^24: exact
            if (tid == FEAT_D + 1) v += row[FEAT_D + 2] * (float)(8 * bx - j * g.S);
            s += v;
        });
        ssum[tid] = s;
    }
    __syncthreads();
    const float n = ssum[FEAT_D + 2];
    const long id = (long)b * nsp + kk;
    if (!(n > 0.f)) {   // uniform: an empty centre keeps its centroid, offset and bias
        if (tid == 0) {
            a.counts[id] = 0;
            if (a.empty) atomicAdd(a.empty, 1);
        }
        return;
    }
    if (tid < FEAT_D) {
        const float v = ssum[tid] / n;
        snew[tid] = v;
        a.cent[id * FEAT_D + tid] = v;
    } else if (tid < FEAT_D + 2) {
        a.off[2 * id + (tid - FEAT_D)] = ssum[tid] / n;
    }
    __syncthreads();
    if (tid == 0) {
        float c2 = 0.f;
        for (int d = 0; d < FEAT_D; ++d) c2 = fmaf(snew[d], snew[d], c2);
        a.bias[id] = -0.5f * c2;
        a.counts[id] = (int32_t)n;
    }
}

constexpr int SL_MAXC = 128;

struct SlicPoolArgs {
    const float* map;
    const int64_t* labels;
    float* slab;
    SlicGeo g;
    int C;
};

__global__ __launch_bounds__(256) void slic_pool_kernel(SlicPoolArgs a) {
    __shared__ float tile[64 * (SL_MAXC + 1)];
    __shared__ float sacc[2 * 16 * SL_MAXC];
    __shared__ int sslot[64];
    const SlicGeo& g = a.g;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SlicBlock k = slic_block(g);
    const int C = a.C, CP = C | 1, NW = g.NW;
    const long plane = g.plane();
    const int y = k.y0 + (lane >> 3), x = k.x0 + (lane & 7);
    const bool in = y < g.Hs && x < g.Ws;
    const long p = in ? (long)y * g.Ws + x : 0;
    const float* src = a.map + (long)k.b * C * plane + p;
    for (int c = wave; c < C; c += 4) tile[lane * CP + c] = in ? src[(long)c * plane] : 0.f;
    if (tid < 64) {
        int slot = -1;
        if (in) {
            const int64_t lab = a.labels[(long)k.b * plane + p];
            if (lab >= 0 && lab < g.nsp()) {
                const int si = (int)lab / g.gx - k.ci0, sj = (int)lab % g.gx - k.cj0;
                if (si >= 0 && si < NW && sj >= 0 && sj < NW) slot = si * NW + sj;
            }
        }
        sslot[tid] = slot;
    }
    for (int e = tid; e < 2 * 16 * C; e += 256) sacc[e] = 0.f;
    __syncthreads();
    if (tid < 2 * C) {
        const int h = tid / C, c = tid - h * C;
        float* acc = sacc + h * 16 * C + c;
        for (int q = 32 * h; q < 32 * h + 32; ++q) {
            const int s = sslot[q];
            if (s >= 0) acc[s * C] += tile[q * CP + c];
        }
    }
    __syncthreads();
    float* out = a.slab + (long)blockIdx.x * 16 * (C + 1);
    for (int e = tid; e < 16 * C; e += 256) {
        const int s = e / C, c = e - s * C;
        out[s * (C + 1) + c] = sacc[e] + sacc[16 * C + e];
    }
    if (tid < 16) {
        int n = 0;
        for (int q = 0; q < 64; ++q) n += sslot[q] == tid ? 1 : 0;
        out[tid * (C + 1) + C] = (float)n;
    }
}

struct SlicFinishArgs {
    const float* __restrict__ slab;
    float* table;
    int64_t* region;
    SlicGeo g;
    int C;
};

__global__ __launch_bounds__(128) void slic_pool_finish_kernel(SlicFinishArgs a) {
    __shared__ float sval[SL_MAXC];
    const SlicGeo& g = a.g;
    const int tid = threadIdx.x, C = a.C;
    const int nsp = g.nsp();
    const int b = blockIdx.x / nsp, kk = blockIdx.x - b * nsp;
    const int i = kk / g.gx, j = kk - i * g.gx;
    const long id = (long)b * nsp + kk;
    if (tid < C) {
        float s = 0.f, n = 0.f;
        slic_for_blocks(g, i, j, [&](int by, int bx, int slot) {
            const float* row = a.slab + ((((long)b * g.nby + by) * g.nbx + bx) * 16 + slot) * (C + 1);
            s += row[tid];
            n += row[C];
        });
        const float v = n > 0.f ? s / n : __builtin_nanf("");
        sval[tid] = v;
        a.table[id * C + tid] = v;
    }
    __syncthreads();
    if (tid == 0 && a.region) {
        float bv = -__builtin_inff();
        int bi = -1;
        for (int c = 0; c < C; ++c) {
            if (sval[c] > bv) { bv = sval[c]; bi = c; }
        }
        a.region[id] = bi;
    }
}

__global__ __launch_bounds__(256) void slic_broadcast_kernel(const int64_t* labels, const int64_t* region, int64_t* classes, long plane, long total,
                                                             int nsp) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int64_t lab = labels[e];
    classes[e] = lab >= 0 && lab < nsp ? region[(e / plane) * nsp + lab] : -1;
}

}  // namespace

long slic_blocks(int Bs, int Hs, int Ws) { return (long)Bs * ((Hs + 7) / 8) * ((Ws + 7) / 8); }

long slic_scratch_floats(int Bs, int Hs, int Ws, int C) { return slic_blocks(Bs, Hs, Ws) * 16 * (C + 1); }

int launch_slic_assign(const float* feat, const int32_t* cover, int Bs, int Hs, int Ws, int step, float hl, const float* centroids,
                       const float* offsets, const float* bias, const int32_t* counts, int64_t* labels, const int64_t* prev_labels, int32_t* moved,
                       float* best, float* slab, hipStream_t st) {
    SlicAssignArgs a;
    a.feat = feat; a.cover = cover; a.cent = centroids; a.off = offsets; a.bias = bias; a.counts = counts; a.labels = labels;
    a.prev = prev_labels; a.moved = moved; a.best = best; a.slab = slab; a.g = slic_geo(Bs, Hs, Ws, step); a.hl = hl;
    hipLaunchKernelGGL(slic_assign_kernel, dim3((unsigned)a.g.blocks()), dim3(256), 0, st, a);
    return (int)hipGetLastError();
}

int launch_slic_update(const float* slab, int Bs, int Hs, int Ws, int step, float* centroids, float* offsets, float* bias, int32_t* counts,
                       int32_t* empty, hipStream_t st) {
    SlicUpdateArgs a;
    a.slab = slab; a.cent = centroids; a.off = offsets; a.bias = bias; a.counts = counts; a.empty = empty; a.g = slic_geo(Bs, Hs, Ws, step);
    hipLaunchKernelGGL(slic_update_kernel, dim3((unsigned)((long)Bs * a.g.nsp())), dim3(128), 0, st, a);
    return (int)hipGetLastError();
}

int launch_slic_pool(const float* map, const int64_t* labels, int Bs, int C, int Hs, int Ws, int step, float* slab, hipStream_t st) {
    SlicPoolArgs a;
    a.map = map; a.labels = labels; a.slab = slab; a.g = slic_geo(Bs, Hs, Ws, step); a.C = C;
    hipLaunchKernelGGL(slic_pool_kernel, dim3((unsigned)a.g.blocks()), dim3(256), 0, st, a);
    return (int)hipGetLastError();
}

int launch_slic_pool_finish(const float* slab, int Bs, int C, int Hs, int Ws, int step, float* table, int64_t* region_classes, hipStream_t st) {
    SlicFinishArgs a;
    a.slab = slab; a.table = table; a.region = region_classes; a.g = slic_geo(Bs, Hs, Ws, step); a.C = C;
    hipLaunchKernelGGL(slic_pool_finish_kernel, dim3((unsigned)((long)Bs * a.g.nsp())), dim3(128), 0, st, a);
    return (int)hipGetLastError();
}

int launch_slic_broadcast(const int64_t* labels, const int64_t* region_classes, int Bs, int Hs, int Ws, int step, int64_t* classes, hipStream_t st) {
    const SlicGeo g = slic_geo(Bs, Hs, Ws, step);
    const long total = (long)Bs * g.plane();
    hipLaunchKernelGGL(slic_broadcast_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, labels, region_classes, classes, g.plane(),
                       total, g.nsp());
    return (int)hipGetLastError();
}

}  // namespace msst
