// Second-order statistics of frozen per-pixel features (msst_feat_moments, msst_feat_moments_finish, msst_feat_project;
// maskedsst_amd/pca.py): the mean and covariance of rows x [M][96] or of an encode_scene map [Bs][96][plane] read in place, and the
// projection of rows or a map onto 1 <= r <= 96 given directions (PCA scores, whitened scores, the squared Mahalanobis distance of the
// RX detector).  fp32, no atomics; every output has the same bits in every call.
//
// The tile loaders of both layouts, the centring and the row flags, the scores loop, the table store and the partition are msst_feat.h's.
// feat_moments  grid = workgroups of whole 64-row tiles (feat_partition), 256 threads = 4 waves, LDS: x tile [64][98] | centre [96] |
//             row flags [64]: 25 KB, two workgroups per CU.
//   tile      one tile ahead in registers; c = x - centre (null centre: zeros) is formed in fp32 in the registers on the way to LDS.
//   flags     four threads per row: a row with a channel that is not finite, and a row past the end, is zeroed in LDS (0 x NaN would
//             poison the sums) and not counted.
//   s2        sum c c^T as the product tile^T tile on v_mfma_f32_16x16x4_f32 with the ROW as the k index: A = c[row 4 ks + (l >> 4)]
//             [16 it + (l & 15)], B = c[row 4 ks + (l >> 4)][16 jt + (l & 15)], so an entry is the fmaf chain of its rows in row order
//             over all tiles of the workgroup.  s2 is symmetric and a c_i c_j product commutes, so only the 21 (it <= jt) of the 36
//             (channel tile, channel tile) pairs are computed, dealt round-robin to the 4 waves (pair p = wave + 4 i in the order (0,0)
//             .. (0,5), (1,1) .. (5,5): 6, 5, 5, 5 accumulators); an off-diagonal pair is stored twice, [i][j] and [j][i], from one
//             register, and inside a diagonal pair both chains multiply the same two numbers in the same order: s2 is symmetric bit
//             for bit.
//   s1, n     thread d < 96 sums column d of the tile in row order; wave 3 counts the unflagged rows (ballot), in integers.
//   partials  the workgroup writes [n (int32 bits) | s1 96 | s2 96 x 96] to its slab row: 9313 floats.
// feat_moments_finish  72 workgroups x 256 threads: threads 0 .. 127 one s2 entry each, 128 .. 223 one s1 channel each, 224 the count,
//             side by side: the slab rows summed in workgroup order in double (every workgroup sums n and s1 for itself, the same
//             chains), then count, mean = centre + s1 / n, cov = (s2 - s1 s1^T / n) / (n - ddof) evaluated in double and rounded once,
//             and the raw sums [s1 | s2] rounded to fp32.
// feat_project  LDS (rp = r rounded up to 16, 32, 64 or 96): components [rp][98] (rows from r on zero) | x tile [64][98] | out [64][rp + 1]
//             | mean [96] | flags [64]: 88 KB at rp = 96.  Up to 32 directions: one 64-row tile per workgroup (the table is small, the
//             whole device streams); more: the whole tiles of feat_partition, the table loaded once, one tile ahead in registers.
//             out[q][j] = the fmaf chain over d = 0 .. 95 of (x[q][d] - mean[d]) components[j][d] from zero (feat_scores); sumsq[q] =
//             over the lane's own j ascending by fmaf, then over the 16 lanes of the group (feat_group_sum): an order that depends on
//             r alone.  A flagged row gets NaN everywhere.
// No inline assembly.
#include "../../include/msst.h"
#include "msst_feat.h"
#include "msst_kernels.h"

namespace msst {

namespace {

constexpr int PCA_P = 98;                                    // LDS pitch of a feature row and of a component row
constexpr int PCA_PAIRS = 21;                                // channel tile pairs it <= jt
constexpr int PCA_PPW = (PCA_PAIRS + 3) / 4;                 // 6: wave 0 has six, the others five
constexpr int PCA_SLAB = 1 + FEAT_D + FEAT_D * FEAT_D;       // floats of a workgroup's slab row

// ---- pair p = wave + 4 i of the 21 (it <= jt), rows of the upper triangle in order; false: the wave has no i-th pair
__device__ __forceinline__ bool pca_wave_pair(int wave, int i, int& it, int& jt) {
    int p = wave + 4 * i;
    const bool has = p < PCA_PAIRS;
    it = 0;
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        if (it == t && p >= 6 - t) { p -= 6 - t; ++it; }
    }
    jt = it + p;
    return has;
}

struct PcaMomArgs {
    const float* x;
    const float* centre;   // null: zeros
    float* slab;
    long rows, plane, tiles_per_wg;
};

template <int LAYOUT>
__global__ __launch_bounds__(256, 2) void feat_moments_kernel(PcaMomArgs a) {
    __shared__ __attribute__((aligned(16))) float xs[64 * PCA_P];
    __shared__ __attribute__((aligned(16))) float scen[FEAT_D];
    __shared__ int sflag[64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cg = lane >> 4, cc = lane & 15;

    if (tid < FEAT_D) scen[tid] = a.centre ? a.centre[tid] : 0.f;
    int ao[PCA_PPW], bo[PCA_PPW];
#pragma unroll
    for (int i = 0; i < PCA_PPW; ++i) {
        int it, jt;
        pca_wave_pair(wave, i, it, jt);
        ao[i] = 16 * it;
        bo[i] = 16 * jt;
    }
    const bool six = wave == 0;   // pairs 20 .. 23: only wave 0 has a sixth

    const long rbeg = (long)blockIdx.x * a.tiles_per_wg * 64;
    const long rend = min(a.rows, rbeg + a.tiles_per_wg * 64);
    const long ntiles = rend > rbeg ? (rend - rbeg + 63) / 64 : 0;

    f32x4 pre[6];
    auto load_tile = [&](long r0) {
        if (LAYOUT == 0) feat_rows_prefetch(pre, a.x, r0, rend, tid);
        else feat_map_prefetch(pre, a.x, a.plane, r0, rend, tid);
    };
    if (ntiles > 0) load_tile(rbeg);

    f32x4 acc[PCA_PPW];
#pragma unroll
    for (int i = 0; i < PCA_PPW; ++i) acc[i] = zero4();
    float s1 = 0.f;
    int cnt = 0;

    for (long t = 0; t < ntiles; ++t) {
        const long r0 = rbeg + t * 64;
        __syncthreads();   // the previous tile's reads (and, first, the centre) are done
        if (LAYOUT == 0) {
            feat_centre_rows(pre, scen, tid);
            feat_rows_store<PCA_P>(xs, pre, tid);
        } else {
            feat_centre_map(pre, scen, tid);
            feat_map_store<PCA_P>(xs, pre, tid);
        }
        __syncthreads();
        if (t + 1 < ntiles) load_tile(r0 + 64);
        feat_flag_rows<PCA_P>(xs, sflag, r0, rend, tid);
        __syncthreads();
        // ---- s2 += tile^T tile over the 64 rows; the pairs inside, so that a wave's accumulators are independent
#pragma unroll 2
        for (int ks = 0; ks < 16; ++ks) {
            const float* xr = xs + (4 * ks + cg) * PCA_P + cc;
#pragma unroll
            for (int i = 0; i < PCA_PPW; ++i) {
                if (i + 1 < PCA_PPW || six) acc[i] = PF32::mma(xr[ao[i]], xr[bo[i]], acc[i]);
            }
        }
        if (tid < FEAT_D) {
#pragma unroll 8
            for (int r = 0; r < 64; ++r) s1 += xs[r * PCA_P + tid];
        }
        if (wave == 3) cnt += __popcll(__ballot(sflag[lane] == 0));
    }

    // ---- the workgroup's partial sums
    float* out = a.slab + (long)blockIdx.x * PCA_SLAB;
    if (tid == 192) reinterpret_cast<int*>(out)[0] = cnt;
    if (tid < FEAT_D) out[1 + tid] = s1;
    float* o2 = out + 1 + FEAT_D;
#pragma unroll
    for (int i = 0; i < PCA_PPW; ++i) {
        if (i + 1 < PCA_PPW || six) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = ao[i] + 4 * cg + r, col = bo[i] + cc;
                o2[row * FEAT_D + col] = acc[i][r];
                if (ao[i] != bo[i]) o2[col * FEAT_D + row] = acc[i][r];
            }
        }
    }
}

struct PcaFinArgs {
    const float* __restrict__ slab;
    const float* centre;   // null: zeros
    long long* count;
    float* mean;
    float* cov;            // null: not wanted
    float* raw;            // null: not wanted
    int nwg, ddof;
};

constexpr int PCA_FIN_ENTRIES = 128;    // s2 entries per workgroup of feat_moments_finish_kernel: threads 0 .. 127; 128 .. 223 sum s1, 224 sums n

__global__ __launch_bounds__(256) void feat_moments_finish_kernel(PcaFinArgs a) {
    __shared__ double sd1[FEAT_D];
    __shared__ long long sn;
    const int tid = threadIdx.x;
    const int e = blockIdx.x * PCA_FIN_ENTRIES + tid;
    double s = 0.0;
    if (tid < PCA_FIN_ENTRIES) {
        if (a.cov || a.raw) {
#pragma unroll 16
            for (int g = 0; g < a.nwg; ++g) s += (double)a.slab[(long)g * PCA_SLAB + 1 + FEAT_D + e];   // the loads in flight, the additions in order
        }
    } else if (tid < PCA_FIN_ENTRIES + FEAT_D) {
        const int d = tid - PCA_FIN_ENTRIES;
        double s1 = 0.0;
#pragma unroll 16
        for (int g = 0; g < a.nwg; ++g) s1 += (double)a.slab[(long)g * PCA_SLAB + 1 + d];
        sd1[d] = s1;
    } else if (tid == PCA_FIN_ENTRIES + FEAT_D) {
        long long n = 0;
        for (int g = 0; g < a.nwg; ++g) n += reinterpret_cast<const int*>(a.slab)[(long)g * PCA_SLAB];
        sn = n;
    }
    __syncthreads();
    const long long n = sn;
    if (blockIdx.x == 0) {
        if (tid == 0) a.count[0] = n;
        if (tid >= PCA_FIN_ENTRIES && tid < PCA_FIN_ENTRIES + FEAT_D) {
            const int d = tid - PCA_FIN_ENTRIES;
            a.mean[d] = (float)((a.centre ? (double)a.centre[d] : 0.0) + sd1[d] / (double)n);   // n == 0: NaN
            if (a.raw) a.raw[d] = (float)sd1[d];
        }
    }
    if (tid < PCA_FIN_ENTRIES) {
        const int i = e / FEAT_D, j = e - i * FEAT_D;
        if (a.raw) a.raw[FEAT_D + e] = (float)s;
        if (a.cov) {
            const long long dof = n - a.ddof;
            a.cov[e] = dof > 0 ? (float)((s - sd1[i] * sd1[j] / (double)n) / (double)dof) : __builtin_nanf("");
        }
    }
}

// the LDS of feat_project_kernel<NCT>, offsets in floats
template <int NCT>
struct PcaProjLds {
    static constexpr int LP = 16 * NCT + 1;                  // pitch of an out row
    static constexpr int comp = 0;                           // [16 NCT][PCA_P]
    static constexpr int x = comp + 16 * NCT * PCA_P;        // [64][PCA_P]
    static constexpr int out = x + 64 * PCA_P;               // [64][LP]
    static constexpr int mean = out + 64 * LP;               // [96]
    static constexpr int flag = mean + FEAT_D;               // [64] int
    static constexpr size_t bytes = (size_t)4 * (flag + 64);
    static_assert(mean % 4 == 0, "the mean is read 16 bytes at a time");
};

struct PcaProjArgs {
    const float* x;
    const float* mean;
    const float* comp;
    float* out;      // null: sumsq only
    float* sumsq;    // null: out only
    long rows, plane, tiles_per_wg;
    int r, x_layout, out_layout;
};

template <int NCT>
__global__ __launch_bounds__(256, NCT <= 2 ? 4 : NCT == 4 ? 2 : 1) void feat_project_kernel(PcaProjArgs a) {   // what the LDS allows
    using L = PcaProjLds<NCT>;
    constexpr int RP = 16 * NCT, LP = L::LP;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float* smem = reinterpret_cast<float*>(smem_raw);
    float *sc = smem + L::comp, *xs = smem + L::x, *sl = smem + L::out, *smean = smem + L::mean;
    int* sflag = reinterpret_cast<int*>(smem + L::flag);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cg = lane >> 4, cc = lane & 15;
    const int nr = a.r;
    const long rbeg = (long)blockIdx.x * a.tiles_per_wg * 64;
    const long rend = min(a.rows, rbeg + a.tiles_per_wg * 64);
    constexpr bool WALK = NCT > 2;   // the launcher gives the small tables one tile per workgroup: no loop to carry registers round
    const long ntiles = !WALK ? 1 : rend > rbeg ? (rend - rbeg + 63) / 64 : 0;

    for (int e = tid; e < RP * FEAT_D; e += 256) {
        const int j = e / FEAT_D, d = e - j * FEAT_D;
        sc[j * PCA_P + d] = j < nr ? a.comp[e] : 0.f;
    }
    if (tid < FEAT_D) smean[tid] = a.mean[tid];
    f32x4 pre[6];
    auto load_tile = [&](long r0) {
        if (a.x_layout == 0) feat_rows_prefetch(pre, a.x, r0, rend, tid);
        else feat_map_prefetch(pre, a.x, a.plane, r0, rend, tid);
    };
    if (ntiles > 0) load_tile(rbeg);

    for (long t = 0; t < ntiles; ++t) {
        const long r0 = rbeg + t * 64;
        const long nq = min((long)64, rend - r0);
        __syncthreads();   // the previous tile's reads (and, first, the components and the mean) are done
        if (a.x_layout == 0) {
            feat_centre_rows(pre, smean, tid);
            feat_rows_store<PCA_P>(xs, pre, tid);
        } else {
            feat_centre_map(pre, smean, tid);
            feat_map_store<PCA_P>(xs, pre, tid);
        }
        __syncthreads();
        if (WALK && t + 1 < ntiles) load_tile(r0 + 64);
        feat_flag_rows<PCA_P>(xs, sflag, r0, rend, tid);
        __syncthreads();
        f32x4 c[NCT];
#pragma unroll
        for (int jt = 0; jt < NCT; ++jt) c[jt] = zero4();
        feat_scores<NCT, PCA_P, PCA_P>(xs, sc, wave, cc, cg, c);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int rl = 16 * wave + 4 * cg + r;
            const bool bad = sflag[rl] == 1;
            float ss = 0.f;
#pragma unroll
            for (int jt = 0; jt < NCT; ++jt) {
                const int cls = 16 * jt + cc;
                const float v = bad ? __builtin_nanf("") : c[jt][r];
                sl[rl * LP + cls] = v;
                if (cls < nr) ss = fmaf(v, v, ss);
            }
            ss = feat_group_sum(ss);
            if (a.sumsq && cc == 0 && rl < nq) a.sumsq[r0 + rl] = ss;
        }
        if (a.out) {   // uniform
            __syncthreads();
            feat_store_table<256>(sl, LP, a.out, a.out_layout, r0, nq, nr, a.plane, tid);
        }
    }
}

template <int NCT>
int pca_project_launch(PcaProjArgs a, hipStream_t st) {
    constexpr size_t lds = PcaProjLds<NCT>::bytes;
    if (int e = feat_allow_lds<&feat_project_kernel<NCT>>(lds)) return e;
    // a small table is cheap to reload: one tile per workgroup keeps the whole device streaming; a large one is loaded once per
    // workgroup of feat_partition's whole tiles
    int nwg;
    if (NCT <= 2) {
        a.tiles_per_wg = 1;
        nwg = (int)((a.rows + 63) / 64);
    } else {
        feat_partition(a.rows, &a.tiles_per_wg, &nwg);
    }
    hipLaunchKernelGGL(feat_project_kernel<NCT>, dim3((unsigned)nwg), dim3(256), lds, st, a);
    return (int)hipGetLastError();
}

}  // namespace

long feat_moments_scratch_floats(long rows) {
    long per;
    int nwg;
    feat_partition(rows, &per, &nwg);
    return (long)nwg * PCA_SLAB;
}

int launch_feat_moments(const float* x, int x_layout, long rows, long plane, const float* centre, float* slab, hipStream_t st) {
    PcaMomArgs a;
    int nwg;
    feat_partition(rows, &a.tiles_per_wg, &nwg);
    a.x = x; a.centre = centre; a.slab = slab; a.rows = rows; a.plane = plane;
    if (x_layout == 0) hipLaunchKernelGGL(feat_moments_kernel<0>, dim3((unsigned)nwg), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(feat_moments_kernel<1>, dim3((unsigned)nwg), dim3(256), 0, st, a);
    return (int)hipGetLastError();
}

int launch_feat_moments_finish(const float* slab, long rows, const float* centre, int ddof, int64_t* count, float* mean, float* cov,
                               float* raw, hipStream_t st) {
    PcaFinArgs a;
    long per;
    feat_partition(rows, &per, &a.nwg);
    a.slab = slab; a.centre = centre; a.count = reinterpret_cast<long long*>(count); a.mean = mean; a.cov = cov; a.raw = raw; a.ddof = ddof;
    static_assert(FEAT_D * FEAT_D % PCA_FIN_ENTRIES == 0, "every workgroup has whole entries");
    hipLaunchKernelGGL(feat_moments_finish_kernel, dim3(FEAT_D * FEAT_D / PCA_FIN_ENTRIES), dim3(256), 0, st, a);
    return (int)hipGetLastError();
}

int launch_feat_project(const float* x, int x_layout, long rows, long plane, const float* mean, const float* components, int r, float* out,
                        int out_layout, float* sumsq, hipStream_t st) {
    PcaProjArgs a;
    a.x = x; a.mean = mean; a.comp = components; a.out = out; a.sumsq = sumsq; a.rows = rows; a.plane = plane; a.r = r;
    a.x_layout = x_layout; a.out_layout = out_layout;
    if (r > 64) return pca_project_launch<6>(a, st);   // 65 .. 96 directions: six tiles, not feat_nct's eight
    return feat_dispatch_nct(r, [&](auto n) { return pca_project_launch<decltype(n)::value>(a, st); });
}

}  // namespace msst
