// k-means clustering of frozen per-pixel features (msst_kmeans_assign, msst_kmeans_update, msst_kmeans_pick; maskedsst_amd/cluster.py):
// Lloyd's iteration as two launches and the k-means++ seeding as one small launch per centre, on rows x [M][96] or an encode_scene map
// [Bs][96][plane] read in place.  1 <= k <= 128, fp32.  No atomics; every output has the same bits in every call, and a fixed point
// (an iteration that moves no row) reproduces itself bit for bit.
//
// Every row gets one score per centroid, s_c = x . c + bias_c: the dot product is the fp32 fmaf chain over d = 0 .. 95 in order from a
// zero accumulator (msst_feat.h: scores), the bias is added behind it.  cosine: bias 0 and
// unit centroids; euclidean: bias = -0.5 |c|^2, so that argmax_c s_c = argmin_c |x - c|^2.  ONE total order: score descending, then
// cluster index ascending.  distance = max(0, 2 (1 - s)) (cosine) or max(0, |x|^2 - 2 s) (euclidean).  A row whose |x|^2 is not finite
// (a NaN channel) gets assignment -1 and distance NaN and contributes to no sum.
//
// The tile loaders of both layouts, the scores loop, the order, the pairs and the partition are msst_feat.h's.
// kmeans_assign  grid = workgroups of whole 64-row tiles (feat_partition), 256 threads = 4 waves, LDS (kp = k rounded up to 16, 32, 64 or
//             128, KmAssignLds): centroids [kp][98] | x tile [64][98] | bias [kp] | |x|^2 [64] | assignment [64] | 16 x 2 row sums: 75 KB
//             at kp = 128, two workgroups per CU.  The cluster-tile count and the layout are template parameters.
//   tile      one tile ahead in registers, stored at pitch 98.  Rows past the end are zero rows, masked by index.
//   |x|^2     four threads per row, channels 4 i + q by fmaf, then (q0 + q1) + (q2 + q3); a row that is not finite is zeroed in LDS (0 x NaN
//             would poison the sums below) and flagged by a NaN in the |x|^2 table.
//   scores    the best (score, index) of a row: over the lane's own clusters ascending, then over the 16 lanes of the group.
//   sums      (fit mode: slab != null) one more product onehot^T x on the same MFMA: each wave accumulates its (cluster tile, channel
//             tile) pairs over ALL tiles of the workgroup in registers: A = (assignment[row 4 ks + (l >> 4)] == cluster) ? 1 : 0, B = x[row 4 ks + (l >> 4)][channel]; the k-step loop
//             is outermost, so a wave's up to 12 accumulators are independent and one assignment read serves all its pairs.  fma(0, x, acc)
//             = acc, so a cluster's sum is the fmaf chain of its member rows in row order.  Counts: thread c counts the tile's rows of
//             cluster c, in integers.
//   partials  the workgroup writes [sums k x 96 | counts k | distance sum | rows whose assignment changed] to its slab row.
// kmeans_update  one workgroup per cluster, 384 threads = 96 channels x 4 slab slices: the slices summed in a fixed order, ((p0 + p1) +
//             (p2 + p3)); euclidean: sum / count (IEEE division); cosine: sum / |sum|; count 0 or |sum| = 0 keeps the centroid.  Writes
//             the new centroid, its bias, its count and its displacement (L2); workgroup 0 also sums the distance and moved partials in
//             workgroup order.  The two history entries that span clusters (empty, shift = the largest displacement) are folded on the
//             host from the k counts and displacements: a cross-workgroup maximum inside one launch would need an atomic.
// kmeans_pick  one workgroup: the D^2 draw of k-means++ from the dist array and the per-workgroup distance sums that kmeans_assign left.
//             total = the sums in workgroup order; t = u total, u = (h >> 8) 2^-24, h = the counter hash of (seed, j); the first workgroup
//             block whose inclusive prefix exceeds t, then inside it the first row whose inclusive prefix (continued from the blocks
//             before, rows ascending) exceeds t.  Rows chosen before never count (their distance is 0 up to rounding).  Rounding can leave
//             no such row in the block: then the block's last row of positive distance.  total == 0: the lowest row not chosen yet.
//             Centre 0: row (h >> 8) M >> 24 = floor(u M).
// No inline assembly.
#include "../../include/msst.h"
#include "msst_feat.h"
#include "msst_kernels.h"

namespace msst {

namespace {

constexpr int KM_P = 98;               // LDS pitch of a centroid row and of a feature row

// the LDS of kmeans_assign_kernel<NCT, .>, offsets in floats
template <int NCT>
struct KmAssignLds {
    static constexpr int cent = 0;                       // [16 NCT][KM_P]
    static constexpr int x = cent + 16 * NCT * KM_P;     // [64][KM_P]
    static constexpr int bias = x + 64 * KM_P;           // [16 NCT]
    static constexpr int x2 = bias + 16 * NCT;           // [64]  NaN: the row is not finite
    static constexpr int asg = x2 + 64;                  // [64] int
    static constexpr int red = asg + 64;                 // [16][2]
    static constexpr size_t bytes = (size_t)4 * (red + 32);
};

__device__ __forceinline__ unsigned km_mix(unsigned x) {   // the finaliser of msst_mask.hip
    x *= 0x9E3779B1U; x ^= x >> 15;
    x *= 0x85EBCA6BU; x ^= x >> 13;
    x *= 0xC2B2AE35U; x ^= x >> 16;
    return x;
}
__device__ __forceinline__ unsigned km_hash(unsigned seed, unsigned j) { return km_mix(km_mix(seed ^ 0x6B6D2B2BU) ^ j); }

struct KmAssignArgs {
    const float* x;
    const float* cent;
    const float* bias;
    int32_t* assign;      // fit mode: read (the previous assignment) before it is written
    float* dist;
    int64_t* classes;     // null or [rows]
    float* slab;          // null: assign only
    long rows, plane, tiles_per_wg;
    int k, metric;
};

template <int NCT, int LAYOUT>
__global__ __launch_bounds__(256, NCT <= 2 ? 3 : NCT == 4 ? 2 : 1) void kmeans_assign_kernel(KmAssignArgs a) {
    constexpr int KP = 16 * NCT, PPW = feat_pairs_per_wave(NCT);
    using L = KmAssignLds<NCT>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float* smem = reinterpret_cast<float*>(smem_raw);
    float *sc = smem + L::cent, *xs = smem + L::x, *sbias = smem + L::bias, *sx2 = smem + L::x2, *sred = smem + L::red;
    int* sasg = reinterpret_cast<int*>(smem + L::asg);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cg = lane >> 4, cc = lane & 15;
    const int k = a.k;
    const bool fit = a.slab != nullptr;
    const bool cosine = a.metric == MSST_KMEANS_COSINE;

    for (int e = tid; e < KP * FEAT_D; e += 256) {
        const int j = e / FEAT_D, d = e - j * FEAT_D;
        sc[j * KM_P + d] = j < k ? a.cent[e] : 0.f;
    }
    for (int j = tid; j < KP; j += 256) sbias[j] = j < k ? a.bias[j] : 0.f;

    const long rbeg = (long)blockIdx.x * a.tiles_per_wg * 64;
    const long rend = min(a.rows, rbeg + a.tiles_per_wg * 64);
    const long ntiles = rend > rbeg ? (rend - rbeg + 63) / 64 : 0;

    f32x4 pre[6];
    auto load_tile = [&](long r0) {
        if (LAYOUT == 0) feat_rows_prefetch(pre, a.x, r0, rend, tid);
        else feat_map_prefetch(pre, a.x, a.plane, r0, rend, tid);
    };
    if (ntiles > 0) load_tile(rbeg);

    f32x4 acc[PPW];
#pragma unroll
    for (int i = 0; i < PPW; ++i) acc[i] = zero4();
    int cnt = 0;
    float dist_acc = 0.f, moved_acc = 0.f;

    for (long t = 0; t < ntiles; ++t) {
        const long r0 = rbeg + t * 64;
        __syncthreads();   // the previous tile's operand reads (and, first, the centroids) are done
        if (LAYOUT == 0) feat_rows_store<KM_P>(xs, pre, tid);
        else feat_map_store<KM_P>(xs, pre, tid);
        __syncthreads();
        if (t + 1 < ntiles) load_tile(r0 + 64);
        {   // ---- |x|^2, four threads per row
            float* xr = xs + (tid >> 2) * KM_P + (tid & 3);
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < 24; ++i) s = fmaf(xr[4 * i], xr[4 * i], s);
            s += __shfl_xor(s, 1);
            s += __shfl_xor(s, 2);
            const bool bad = !(fabsf(s) <= 3.0e38f);
            if (bad) {
#pragma unroll
                for (int i = 0; i < 24; ++i) xr[4 * i] = 0.f;
            }
            if ((tid & 3) == 0) sx2[tid >> 2] = bad ? __builtin_nanf("") : s;
        }
        __syncthreads();
        // ---- scores of 16 rows x KP clusters
        f32x4 c[NCT];
#pragma unroll
        for (int jt = 0; jt < NCT; ++jt) c[jt] = zero4();
        feat_scores<NCT, KM_P, KM_P>(xs, sc, wave, cc, cg, c);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int rl = 16 * wave + 4 * cg + r;
            const long row = r0 + rl;
            const bool valid = row < rend;
            float bv = -INFINITY;
            int bi = 0x7fffffff;
#pragma unroll
            for (int jt = 0; jt < NCT; ++jt) {
                const int cls = 16 * jt + cc;
                const float s = c[jt][r] + sbias[cls];
                if (cls < k && s > bv) { bv = s; bi = cls; }
            }
            feat_group_argmax(bv, bi);
            const float x2 = sx2[rl];
            const int asg = (x2 != x2 || bi == 0x7fffffff) ? -1 : bi;
            const float draw = cosine ? 2.0f * (1.0f - bv) : x2 - 2.0f * bv;
            const float d = asg < 0 ? __builtin_nanf("") : fmaxf(draw, 0.f);
            if (cc == 0) {
                if (valid) {
                    if (fit) {
                        moved_acc += a.assign[row] != asg ? 1.0f : 0.f;
                        if (asg >= 0) dist_acc += d;
                    }
                    a.assign[row] = asg;
                    a.dist[row] = d;
                    if (a.classes) a.classes[row] = asg;
                }
                sasg[rl] = valid ? asg : -1;
            }
        }
        if (!fit) continue;   // uniform
        __syncthreads();
        // ---- sums += onehot^T x over the tile's 64 rows; counts
#pragma unroll 2
        for (int ks = 0; ks < 16; ++ks) {   // the pairs inside: a wave's accumulators are independent, one assignment read serves all
            const int sa = sasg[4 * ks + cg];
            const float* xrow = xs + (4 * ks + cg) * KM_P + cc;
#pragma unroll
            for (int i = 0; i < PPW; ++i) {
                int it, jt;
                if (feat_wave_pair<NCT>(wave, i, it, jt) && 16 * it < k) acc[i] = PF32::mma(sa == 16 * it + cc ? 1.0f : 0.f, xrow[16 * jt], acc[i]);
            }
        }
        if (tid < k) {
            const int4* s4 = reinterpret_cast<const int4*>(sasg);
#pragma unroll 2
            for (int r = 0; r < 16; ++r) {
                const int4 v = s4[r];
                cnt += (v.x == tid ? 1 : 0) + (v.y == tid ? 1 : 0) + (v.z == tid ? 1 : 0) + (v.w == tid ? 1 : 0);
            }
        }
    }
    if (!fit) return;

    // ---- the workgroup's partial sums
    if (cc == 0) {
        sred[(4 * wave + cg) * 2] = dist_acc;
        sred[(4 * wave + cg) * 2 + 1] = moved_acc;
    }
    float* out = a.slab + (long)blockIdx.x * (97 * k + 2);
    feat_store_pairs<NCT, FEAT_D>(out, acc, k, wave, cc, cg);
    if (tid < k) out[k * FEAT_D + tid] = (float)cnt;
    __syncthreads();
    if (tid == 0) {
        float ds = 0.f, mv = 0.f;
        for (int i = 0; i < 16; ++i) { ds += sred[2 * i]; mv += sred[2 * i + 1]; }
        out[97 * k] = ds;
        out[97 * k + 1] = mv;
    }
}

struct KmUpdateArgs {
    const float* __restrict__ slab;
    float* cent;
    float* bias;
    int32_t* counts;
    float* shift;
    float* hist;    // [2]: inertia, moved
    int k, nwg, metric;
};

__global__ __launch_bounds__(384) void kmeans_update_kernel(KmUpdateArgs a) {
    __shared__ float spart[4][FEAT_D];
    __shared__ float snew[FEAT_D];
    __shared__ float sold[FEAT_D];
    __shared__ float swg[2][FEAT_MAX_WGS];
    __shared__ long long scnt;
    const int tid = threadIdx.x;
    const int c = blockIdx.x, k = a.k;
    const int P = 97 * k + 2;
    const int d = tid % FEAT_D, slice = tid / FEAT_D;
    float part = 0.f;
#pragma unroll 8
    for (int g = slice; g < a.nwg; g += 4) part += a.slab[(long)g * P + c * FEAT_D + d];   // the loads of eight rows in flight, the additions in order
    spart[slice][d] = part;
    for (int g = tid; g < a.nwg; g += 384) {
        swg[0][g] = a.slab[(long)g * P + k * FEAT_D + c];
        if (c == 0) swg[1][g] = a.slab[(long)g * P + 97 * k];
    }
    if (tid < FEAT_D) sold[tid] = a.cent[c * FEAT_D + tid];
    __syncthreads();
    if (tid == 0) {
        long long n = 0;
        for (int g = 0; g < a.nwg; ++g) n += (long long)swg[0][g];   // whole numbers below 2^24 each: exact
        scnt = n;
        if (c == 0) {
            float inertia = 0.f;
            for (int g = 0; g < a.nwg; ++g) inertia += swg[1][g];
            a.hist[0] = inertia;
        }
    }
    if (tid < FEAT_D) snew[tid] = (spart[0][tid] + spart[1][tid]) + (spart[2][tid] + spart[3][tid]);
    __syncthreads();
    if (c == 0) {   // moved: the second pass over the table's second row
        for (int g = tid; g < a.nwg; g += 384) swg[1][g] = a.slab[(long)g * P + 97 * k + 1];
    }
    const long long n = scnt;
    float norm2 = 0.f;
    if (a.metric == MSST_KMEANS_COSINE) {
        for (int i = 0; i < FEAT_D; ++i) norm2 = fmaf(snew[i], snew[i], norm2);   // every thread the same chain
    }
    const bool keep = n == 0 || (a.metric == MSST_KMEANS_COSINE && !(norm2 > 0.f));
    __syncthreads();
    if (tid < FEAT_D) {
        float v = sold[tid];
        if (!keep) v = a.metric == MSST_KMEANS_COSINE ? snew[tid] / sqrtf(norm2) : snew[tid] / (float)n;
        snew[tid] = v;
        a.cent[c * FEAT_D + tid] = v;
    }
    __syncthreads();
    if (tid == 0) {
        float c2 = 0.f, s2 = 0.f;
        for (int i = 0; i < FEAT_D; ++i) {
            c2 = fmaf(snew[i], snew[i], c2);
            const float df = snew[i] - sold[i];
            s2 = fmaf(df, df, s2);
        }
        a.bias[c] = a.metric == MSST_KMEANS_COSINE ? 0.f : -0.5f * c2;
        a.counts[c] = (int32_t)n;
        a.shift[c] = sqrtf(s2);
        if (c == 0) {
            double mv = 0.0;
            for (int g = 0; g < a.nwg; ++g) mv += (double)swg[1][g];   // whole numbers: exact
            a.hist[1] = (float)mv;
        }
    }
}

struct KmPickArgs {
    const float* x;
    const float* dist;
    const float* slab;
    float* cent;
    float* bias;
    int32_t* seed_rows;
    long rows, tiles_per_wg;
    unsigned seed;
    int j, nwg, metric;
};

__global__ __launch_bounds__(256) void kmeans_pick_kernel(KmPickArgs a) {
    __shared__ float sd[256];
    __shared__ float sx[FEAT_D];
    __shared__ int stab[128];
    __shared__ double st;          // t = u total, exact in double (24 x 24 bits)
    __shared__ float sbefore;      // the prefix of the blocks before
    __shared__ long long sl[3];    // the block, the chosen row (-1: none yet), the last row of positive distance
    const int tid = threadIdx.x;
    const int j = a.j;
    const unsigned h = km_hash(a.seed, (unsigned)j);
    for (int i = tid; i < j; i += 256) stab[i] = a.seed_rows[i];
    __syncthreads();
    auto chosen = [&](long r) {
        for (int i = 0; i < j; ++i)
            if (stab[i] == r) return true;
        return false;
    };
    if (j == 0) {
        if (tid == 0) sl[1] = (long long)(((unsigned long long)(h >> 8) * (unsigned long long)a.rows) >> 24);
    } else {
        const int P = 97 * j + 2;
        if (tid == 0) {
            float total = 0.f;
            for (int g = 0; g < a.nwg; ++g) total += a.slab[(long)g * P + 97 * j];
            sl[0] = -1; sl[1] = -1; sl[2] = -1;
            if (total > 0.f) {
                const double t = (double)(h >> 8) * 5.9604644775390625e-8 * (double)total;
                float p = 0.f;
                int blk = -1, lastpos = -1;
                float before = 0.f, lastbefore = 0.f;
                for (int g = 0; g < a.nwg; ++g) {
                    const float s = a.slab[(long)g * P + 97 * j];
                    if (s > 0.f) { lastpos = g; lastbefore = p; }
                    const float q = p + s;
                    if ((double)q > t) { blk = g; before = p; break; }
                    p = q;
                }
                if (blk < 0) { blk = lastpos; before = lastbefore; }   // t rounded up to the total
                sl[0] = blk;
                st = t;
                sbefore = before;
            } else {
                long r = 0;
                while (chosen(r)) ++r;   // at most j rows are taken
                sl[1] = r;
            }
        }
        __syncthreads();
        if (sl[0] >= 0) {
            const long rbeg = (long)sl[0] * a.tiles_per_wg * 64;
            const long rend = min(a.rows, rbeg + a.tiles_per_wg * 64);
            const double t = st;
            float p = sbefore;   // thread 0's running prefix
            for (long r0 = rbeg; r0 < rend; r0 += 256) {
                const long r = r0 + tid;
                float dv = r < rend ? a.dist[r] : 0.f;
                if (!(dv > 0.f) || chosen(r)) dv = 0.f;
                sd[tid] = dv;
                __syncthreads();
                if (tid == 0) {
                    for (int i = 0; i < 256; ++i) {
                        const float dvi = sd[i];
                        if (dvi > 0.f) {
                            sl[2] = r0 + i;
                            p += dvi;
                            if ((double)p > t) { sl[1] = r0 + i; break; }
                        }
                    }
                }
                __syncthreads();
                if (sl[1] >= 0) break;   // uniform
            }
            if (tid == 0 && sl[1] < 0) {
                long r = sl[2];
                if (r < 0) { r = 0; while (chosen(r)) ++r; }   // (a block sum above 0 without a countable row: cannot happen)
                sl[1] = r;
            }
        }
    }
    __syncthreads();
    const long row = (long)sl[1];
    if (tid < FEAT_D) sx[tid] = a.x[row * FEAT_D + tid];
    __syncthreads();
    float n2 = 0.f;
    for (int i = 0; i < FEAT_D; ++i) n2 = fmaf(sx[i], sx[i], n2);   // every thread the same chain
    const bool cosine = a.metric == MSST_KMEANS_COSINE;
    if (tid < FEAT_D) a.cent[j * FEAT_D + tid] = (cosine && n2 > 0.f) ? sx[tid] / sqrtf(n2) : sx[tid];
    if (tid == 0) {
        a.bias[j] = cosine ? 0.f : -0.5f * n2;
        a.seed_rows[j] = (int32_t)row;
    }
}

template <int NCT, int LAYOUT>
int km_assign_launch(const KmAssignArgs& a, int nwg, hipStream_t st) {
    constexpr size_t lds = KmAssignLds<NCT>::bytes;
    if (int e = feat_allow_lds<&kmeans_assign_kernel<NCT, LAYOUT>>(lds)) return e;
    hipLaunchKernelGGL((kmeans_assign_kernel<NCT, LAYOUT>), dim3((unsigned)nwg), dim3(256), lds, st, a);
    return (int)hipGetLastError();
}

}  // namespace

long kmeans_scratch_floats(long rows, int k) {
    long per;
    int nwg;
    feat_partition(rows, &per, &nwg);
    return (long)nwg * (97 * k + 2);
}

int launch_kmeans_assign(const float* x, int x_layout, long rows, long plane, const float* centroids, const float* bias, int k, int metric,
                         int32_t* assign, float* dist, int64_t* classes, float* slab, hipStream_t st) {
    KmAssignArgs a;
    int nwg;
    feat_partition(rows, &a.tiles_per_wg, &nwg);
    a.x = x; a.cent = centroids; a.bias = bias; a.assign = assign; a.dist = dist; a.classes = classes; a.slab = slab;
    a.rows = rows; a.plane = plane; a.k = k; a.metric = metric;
    const bool rows_layout = x_layout == 0;
    return feat_dispatch_nct(k, [&](auto n) {
        constexpr int NCT = decltype(n)::value;
        return rows_layout ? km_assign_launch<NCT, 0>(a, nwg, st) : km_assign_launch<NCT, 1>(a, nwg, st);
    });
}

int launch_kmeans_update(const float* slab, long rows, int k, int metric, float* centroids, float* bias, int32_t* counts, float* shift,
                         float* history_row, hipStream_t st) {
    KmUpdateArgs a;
    long per;
    feat_partition(rows, &per, &a.nwg);
    a.slab = slab; a.cent = centroids; a.bias = bias; a.counts = counts; a.shift = shift; a.hist = history_row; a.k = k; a.metric = metric;
    hipLaunchKernelGGL(kmeans_update_kernel, dim3((unsigned)k), dim3(384), 0, st, a);
    return (int)hipGetLastError();
}

int launch_kmeans_pick(const float* x, long rows, const float* dist, const float* slab, int j, int metric, unsigned seed, float* centroids,
                       float* bias, int32_t* seed_rows, hipStream_t st) {
    KmPickArgs a;
    feat_partition(rows, &a.tiles_per_wg, &a.nwg);
    a.x = x; a.dist = dist; a.slab = slab; a.cent = centroids; a.bias = bias; a.seed_rows = seed_rows; a.rows = rows; a.seed = seed;
    a.j = j; a.metric = metric;
    hipLaunchKernelGGL(kmeans_pick_kernel, dim3(1), dim3(256), 0, st, a);
    return (int)hipGetLastError();
}

}  // namespace msst
