// Gaussian mixtures of frozen per-pixel features by EM (msst_gmm_posterior, msst_gmm_moments, msst_gmm_update;
// maskedsst_amd/mixture.py).  The E-step's expensive part is msst_gauss_score (msst_gauss.hip), unchanged: it writes score_c(x) for
// every row and component.  This file adds what turns scores into a posterior, the responsibility-weighted second moments and the
// device-side factorisation, so that a whole fit queues launches and synchronises once.  fp32 in, double where sums meet; no float
// atomics; every sum in an order that depends on (rows, K) alone, the row partition on rows alone (feat_partition).
//
// The posterior of a row, one function for both kernels (gmm_row_lse): m = max_c s_c; lse = m + logf(sum_c expf(s_c - m)), c ascending
// in fp32; r_c = expf(s_c - lse).  expf(-inf) is exactly 0.  A NaN score: lse NaN.  Every score -inf: lse = -inf, r = 0.
//
// gmm_posterior  one thread per row, scores and probs as rows [rows][k] or as a map [rows / plane][k][plane].
// gmm_moments  grid = (workgroups of whole 64-row tiles (feat_partition), k): COMPONENTS ACROSS blockIdx.y.  A component's s2 is 21
//             (channel tile, channel tile) accumulators dealt to 4 waves, 6 f32x4 a lane; k of them do not fit a wave's registers and a
//             tile held in LDS across components would have to spill them per tile.  So a workgroup owns one component for its whole
//             walk (the accumulators never leave the registers) and the x tile is read again per component -- out of L2 for all but
//             the first.  256 threads = 4 waves, LDS: c tile [64][98] | scores tile [64][33] | centre [96] | r, sqrt r, lse, flags,
//             counted [64] each: 35 KB, two workgroups per CU.
//   tile      one tile ahead in registers; c = x - centre_c in fp32 on the way to LDS; row flags (feat_flag_rows): a row with a channel
//             that is not finite, and a row past the end, is zeroed and not counted.
//   rows      thread < 64 owns a row: lse and r_c from the scores tile.  Counted: flag 0 and lse finite.  Everything else gets r = 0
//             BY SELECTION.
//   s2        every row of the tile is multiplied by sqrt(r) (one rounding per entry), then tile^T tile on v_mfma_f32_16x16x4_f32 with
//             the row as the k index, the 21 pairs of msst_pca.hip: (sqrt(r) c_i)(sqrt(r) c_j) commutes, so s2 is symmetric bit for
//             bit, and for r in {0, 1} it is exact.
//   s1, n     thread d < 96: s1 = fmaf(sqrt(r), sqrt(r) c_d, s1) in row order; one thread sums r, one the counted rows' lse, wave 3
//             counts (ballot).
//   partials  slab row (workgroup g, component c) at (g k + c) 9313: [n | s1 96 | s2 96 x 96]; after all of them per workgroup
//             [counted (int32 bits) | sum lse], written by the workgroups of component 0.
// gmm_update  grid = k workgroups x 256 threads, LDS: S [96][97] double (the pitch keeps a column off one bank) | Sigma as fp32 [96][96]
//             | s1, row scratch [96] double | N [32] double: 113 KB.  The workgroup sums its component's slab rows in workgroup order
//             in double (s2: the lower triangle only; the upper is its mirror), sums all k counts for itself, forms mean and Sigma in
//             double, factorises and inverts in LDS (msst_gmm_core.h) and rounds once.  A starved component (N < min_count) and a
//             failed factorisation keep centre, table, covariance and logdet; weight and constant are always written.
// No inline assembly.
#include "../../include/msst.h"
#include "msst_feat.h"
#include "msst_gmm_core.h"
#include "msst_kernels.h"

namespace msst {

namespace {

constexpr int GMM_P = 98;                                    // LDS pitch of a feature row
constexpr int GMM_SP = 33;                                   // LDS pitch of a scores row (k <= 32)
constexpr int GMM_PAIRS = 21;                                // channel tile pairs it <= jt
constexpr int GMM_PPW = (GMM_PAIRS + 3) / 4;                 // 6: wave 0 has six, the others five
constexpr int GMM_SLAB = 1 + FEAT_D + FEAT_D * FEAT_D;       // floats of a (workgroup, component) slab row
constexpr int GMM_TRI = FEAT_D * (FEAT_D + 1) / 2;           // entries of a lower triangle
constexpr int GMM_EPT = (GMM_TRI + 255) / 256;               // 19: entries of the triangle a thread of gmm_update sums
constexpr int GMM_DP = FEAT_D + 1;                          // LDS pitch of a row of doubles

// ---- the posterior of one row: s[c * stride], c = 0 .. k - 1
__device__ __forceinline__ float gmm_row_lse(const float* s, long stride, int k) {
    float m = -__builtin_inff();
    bool bad = false;
    for (int c = 0; c < k; ++c) {
        const float v = s[c * stride];
        bad |= v != v;
        m = fmaxf(m, v);
    }
    if (bad) return __builtin_nanf("");
    if (!(fabsf(m) <= 3.4028234e38f)) return m;              // every score -inf: -inf (a score of +inf: +inf)
    float sum = 0.f;
    for (int c = 0; c < k; ++c) sum += expf(s[c * stride] - m);
    return m + logf(sum);
}

__device__ __forceinline__ float gmm_resp(float s, float lse) {
    return lse == -__builtin_inff() ? 0.f : expf(s - lse);   // NaN lse: NaN
}

struct GmmPostArgs {
    const float* scores;
    float* lse;
    float* probs;       // null: not wanted
    long rows, plane;
    int k, in_layout, out_layout;
};

__global__ __launch_bounds__(256) void gmm_posterior_kernel(GmmPostArgs a) {
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= a.rows) return;
    const long b = q / a.plane, p = q - b * a.plane;        // plane is 1 in the rows layout on both sides
    const float* s = a.in_layout == 0 ? a.scores + q * a.k : a.scores + b * a.k * a.plane + p;
    const long ss = a.in_layout == 0 ? 1 : a.plane;
    const float lse = gmm_row_lse(s, ss, a.k);
    a.lse[q] = lse;
    if (a.probs) {
        float* o = a.out_layout == 0 ? a.probs + q * a.k : a.probs + b * a.k * a.plane + p;
        const long os = a.out_layout == 0 ? 1 : a.plane;
        for (int c = 0; c < a.k; ++c) o[c * os] = gmm_resp(s[c * ss], lse);
    }
}

// ---- pair p = wave + 4 i of the 21 (it <= jt), rows of the upper triangle in order, as msst_pca.hip deals them
__device__ __forceinline__ bool gmm_wave_pair(int wave, int i, int& it, int& jt) {
    int p = wave + 4 * i;
    const bool has = p < GMM_PAIRS;
    it = 0;
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        if (it == t && p >= 6 - t) { p -= 6 - t; ++it; }
    }
    jt = it + p;
    return has;
}

struct GmmMomArgs {
    const float* x;
    const float* scores;    // [rows][k]
    const float* centres;   // [k][96]
    float* slab;
    long rows, plane, tiles_per_wg;
    int k;
};

template <int LAYOUT>
__global__ __launch_bounds__(256, 2) void gmm_moments_kernel(GmmMomArgs a) {
    __shared__ __attribute__((aligned(16))) float xs[64 * GMM_P];
    __shared__ __attribute__((aligned(16))) float scen[FEAT_D];
    __shared__ float ssc[64 * GMM_SP];
    __shared__ float sr[64], sq[64], sl[64];
    __shared__ int sflag[64], scnt[64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cg = lane >> 4, cc = lane & 15;
    const int k = a.k, comp = blockIdx.y;

    if (tid < FEAT_D) scen[tid] = a.centres[comp * FEAT_D + tid];
    int ao[GMM_PPW], bo[GMM_PPW];
#pragma unroll
    for (int i = 0; i < GMM_PPW; ++i) {
        int it, jt;
        gmm_wave_pair(wave, i, it, jt);
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

    f32x4 acc[GMM_PPW];
#pragma unroll
    for (int i = 0; i < GMM_PPW; ++i) acc[i] = zero4();
    float s1 = 0.f, nsum = 0.f, lsum = 0.f;
    int cnt = 0;

    for (long t = 0; t < ntiles; ++t) {
        const long r0 = rbeg + t * 64;
        const int nq = (int)min((long)64, rend - r0);
        __syncthreads();   // the previous tile's reads (and, first, the centre) are done
        if (LAYOUT == 0) {
            feat_centre_rows(pre, scen, tid);
            feat_rows_store<GMM_P>(xs, pre, tid);
        } else {
            feat_centre_map(pre, scen, tid);
            feat_map_store<GMM_P>(xs, pre, tid);
        }
        for (int e = tid; e < nq * k; e += 256) {   // the tile's scores: nq k consecutive floats
            const int row = e / k, c = e - row * k;
            ssc[row * GMM_SP + c] = a.scores[r0 * k + e];
        }
        __syncthreads();
        if (t + 1 < ntiles) load_tile(r0 + 64);
        feat_flag_rows<GMM_P>(xs, sflag, r0, rend, tid);
        __syncthreads();
        if (tid < 64) {
            float r = 0.f, l = 0.f;
            int counted = 0;
            if (sflag[tid] == 0) {
                const float lse = gmm_row_lse(ssc + tid * GMM_SP, 1, k);
                if (fabsf(lse) <= 3.4028234e38f) {   // finite: the row counts
                    counted = 1;
                    l = lse;
                    r = expf(ssc[tid * GMM_SP + comp] - lse);
                }
            }
            sr[tid] = r;
            sq[tid] = sqrtf(r);
            sl[tid] = l;
            scnt[tid] = counted;
        }
        __syncthreads();
        {   // c <- sqrt(r) c, four threads per row; a row that does not count is zeroed by selection
            float* xr = xs + (tid >> 2) * GMM_P + (tid & 3);
            const float w = sq[tid >> 2];
            const bool on = scnt[tid >> 2] != 0;
#pragma unroll
            for (int i = 0; i < 24; ++i) xr[4 * i] = on ? w * xr[4 * i] : 0.f;
        }
        __syncthreads();
        // ---- s2 += tile^T tile over the 64 rows; the pairs inside, so that a wave's accumulators are independent
#pragma unroll 2
        for (int ks = 0; ks < 16; ++ks) {
            const float* xr = xs + (4 * ks + cg) * GMM_P + cc;
#pragma unroll
            for (int i = 0; i < GMM_PPW; ++i) {
                if (i + 1 < GMM_PPW || six) acc[i] = PF32::mma(xr[ao[i]], xr[bo[i]], acc[i]);
            }
        }
        if (tid < FEAT_D) {
#pragma unroll 8
            for (int r = 0; r < 64; ++r) s1 = fmaf(sq[r], xs[r * GMM_P + tid], s1);
        }
        if (wave == 3) {
            cnt += __popcll(__ballot(scnt[lane] != 0));
            if (lane == 0) {
#pragma unroll 8
                for (int r = 0; r < 64; ++r) nsum += sr[r];
            }
            if (lane == 1) {
#pragma unroll 8
                for (int r = 0; r < 64; ++r) lsum += sl[r];
            }
        }
    }

    // ---- the workgroup's partial sums
    float* out = a.slab + ((long)blockIdx.x * k + comp) * GMM_SLAB;
    if (tid == 192) out[0] = nsum;
    if (tid < FEAT_D) out[1 + tid] = s1;
    float* o2 = out + 1 + FEAT_D;
#pragma unroll
    for (int i = 0; i < GMM_PPW; ++i) {
        if (i + 1 < GMM_PPW || six) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = ao[i] + 4 * cg + r, col = bo[i] + cc;
                o2[row * FEAT_D + col] = acc[i][r];
                if (ao[i] != bo[i]) o2[col * FEAT_D + row] = acc[i][r];
            }
        }
    }
    if (comp == 0) {
        float* tail = a.slab + (long)gridDim.x * k * GMM_SLAB + 2 * (long)blockIdx.x;
        if (tid == 192) reinterpret_cast<int*>(tail)[0] = cnt;
        if (tid == 193) tail[1] = lsum;
    }
}

// the LDS of gmm_update_kernel, offsets in bytes
struct GmmUpdLds {
    static constexpr size_t S = 0;                                        // [96][97] double
    static constexpr size_t s1 = S + sizeof(double) * FEAT_D * GMM_DP;    // [96] double
    static constexpr size_t row = s1 + sizeof(double) * FEAT_D;           // [96] double
    static constexpr size_t N = row + sizeof(double) * FEAT_D;            // [32] double
    static constexpr size_t misc = N + sizeof(double) * 32;               // [2] double: sum lse, counted
    static constexpr size_t cov = misc + sizeof(double) * 2;              // [96][96] float
    static constexpr size_t bytes = cov + sizeof(float) * FEAT_D * FEAT_D;
    static_assert(bytes <= 160 * 1024, "the LDS of a CU");
};

struct GmmUpdArgs {
    const float* __restrict__ slab;
    float* centres;
    float* tables;
    float* covs;
    float* logdet;
    float* consts;
    float* weights;
    float* raw;        // null: not wanted
    float* record;
    double reg_covar, min_count;
    int nwg, k, diag;
};

__global__ __launch_bounds__(256) void gmm_update_kernel(GmmUpdArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    double* S = reinterpret_cast<double*>(smem_raw + GmmUpdLds::S);
    double* sd1 = reinterpret_cast<double*>(smem_raw + GmmUpdLds::s1);
    double* srow = reinterpret_cast<double*>(smem_raw + GmmUpdLds::row);
    double* sN = reinterpret_cast<double*>(smem_raw + GmmUpdLds::N);
    double* smisc = reinterpret_cast<double*>(smem_raw + GmmUpdLds::misc);
    float* scov = reinterpret_cast<float*>(smem_raw + GmmUpdLds::cov);
    const int tid = threadIdx.x, c = blockIdx.x, k = a.k, nwg = a.nwg;
    const long wstride = (long)k * GMM_SLAB;
    const float* mine = a.slab + (long)c * GMM_SLAB;
    float* raw = a.raw ? a.raw + (long)c * GMM_SLAB : nullptr;

    // ---- the slab rows in workgroup order, in double: s2 (lower triangle), s1, every component's n, the counted rows, sum lse
    // A thread owns GMM_EPT entries of the lower triangle and walks the slab rows once: per slab row its loads are independent (they
    // stay in flight together), per entry the additions run in workgroup order.
    {
        double acc[GMM_EPT];
        int off[GMM_EPT];
#pragma unroll
        for (int q = 0; q < GMM_EPT; ++q) {
            const int e = tid + 256 * q;
            int i = (int)((sqrtf(8.f * (float)e + 1.f) - 1.f) * 0.5f);
            if (i * (i + 1) / 2 > e) --i;
            if ((i + 1) * (i + 2) / 2 <= e) ++i;
            off[q] = e < GMM_TRI ? i * FEAT_D + (e - i * (i + 1) / 2) : 0;   // past the triangle: entry 0 again, summed and dropped
            acc[q] = 0.0;
        }
        const float* src = mine + 1 + FEAT_D;
#pragma unroll 2
        for (int g = 0; g < nwg; ++g) {   // no branch inside: the GMM_EPT loads of a slab row are issued together
            const float* row = src + g * wstride;
            float v[GMM_EPT];
#pragma unroll
            for (int q = 0; q < GMM_EPT; ++q) v[q] = row[off[q]];
#pragma unroll
            for (int q = 0; q < GMM_EPT; ++q) acc[q] += (double)v[q];
        }
#pragma unroll
        for (int q = 0; q < GMM_EPT; ++q) {
            if (tid + 256 * q < GMM_TRI) {
                const int i = off[q] / FEAT_D, j = off[q] - i * FEAT_D;
                S[i * GMM_DP + j] = acc[q];
                if (raw) {
                    raw[1 + FEAT_D + i * FEAT_D + j] = (float)acc[q];
                    raw[1 + FEAT_D + j * FEAT_D + i] = (float)acc[q];
                }
            }
        }
    }
    if (tid < FEAT_D) {
        double s = 0.0;
#pragma unroll 16
        for (int g = 0; g < nwg; ++g) s += (double)mine[g * wstride + 1 + tid];
        sd1[tid] = s;
        if (raw) raw[1 + tid] = (float)s;
    } else if (tid < FEAT_D + 32) {
        const int t = tid - FEAT_D;
        double s = 0.0;
        if (t < k) {
#pragma unroll 16
            for (int g = 0; g < nwg; ++g) s += (double)a.slab[g * wstride + (long)t * GMM_SLAB];
        }
        sN[t] = s;
    } else if (tid == FEAT_D + 32) {
        const float* tail = a.slab + (long)nwg * wstride;
        double s = 0.0;
#pragma unroll 16
        for (int g = 0; g < nwg; ++g) s += (double)tail[2 * g + 1];
        smisc[0] = s;
    } else if (tid == FEAT_D + 33) {
        const int* tail = reinterpret_cast<const int*>(a.slab + (long)nwg * wstride);
        long long n = 0;
#pragma unroll 16
        for (int g = 0; g < nwg; ++g) n += tail[2 * g];
        smisc[1] = (double)n;
    }
    __syncthreads();

    const double N = sN[c];
    double total = 0.0;
    int nstarved = 0;
    for (int t = 0; t < k; ++t) {
        total += sN[t];
        nstarved += !(sN[t] >= a.min_count) ? 1 : 0;
    }
    const double w = total > 0.0 ? N / total : 0.0;
    const bool starved = !(N >= a.min_count);
    if (raw && tid == 0) raw[0] = (float)N;
    if (c == 0 && tid == 0) {
        const double counted = smisc[1];
        a.record[0] = counted > 0.0 ? (float)(smisc[0] / counted) : __builtin_nanf("");
        reinterpret_cast<int*>(a.record)[1] = (int)counted;
        reinterpret_cast<int*>(a.record)[2] = nstarved;
    }

    bool ok = false;
    double ld = 0.0;
    if (!starved) {   // uniform
        // ---- Sigma = s2 / N - delta delta^T + reg I about the current centre, in double; its fp32 rounding kept for the output
        for (int e = tid; e < FEAT_D * FEAT_D; e += 256) {
            const int i = e / FEAT_D, j = e - i * FEAT_D;
            if (j <= i) {
                double v = S[i * GMM_DP + j] / N - (sd1[i] / N) * (sd1[j] / N);
                if (i == j) v += a.reg_covar;
                else if (a.diag) v = 0.0;
                scov[i * FEAT_D + j] = (float)v;
                scov[j * FEAT_D + i] = (float)v;
                S[i * GMM_DP + j] = v;
            }
        }
        auto sync = [] { __syncthreads(); };
        ok = gmm_cholesky(S, FEAT_D, GMM_DP, tid, 256, sync, &ld);
        if (ok) {   // uniform: every thread read the same pivots
            gmm_tri_inverse(S, FEAT_D, GMM_DP, srow, tid, 256, sync);
            for (int e = tid; e < FEAT_D * FEAT_D; e += 256) {
                const int i = e / FEAT_D, j = e - i * FEAT_D;
                a.tables[(long)c * FEAT_D * FEAT_D + e] = j <= i ? (float)S[i * GMM_DP + j] : 0.f;
                a.covs[(long)c * FEAT_D * FEAT_D + e] = scov[e];
            }
            if (tid < FEAT_D) a.centres[c * FEAT_D + tid] = (float)((double)a.centres[c * FEAT_D + tid] + sd1[tid] / N);
            if (tid == 0) a.logdet[c] = (float)ld;
        } else if (tid == 0) {
            atomicAdd(reinterpret_cast<int*>(a.record) + 3, 1);   // an integer count: the order of the additions does not show
        }
    }
    if (tid == 0) {
        const double l = ok ? ld : (double)a.logdet[c];
        a.weights[c] = (float)w;
        a.consts[c] = (float)(log(w) - 0.5 * l - 0.5 * FEAT_D * 1.8378770664093454835606594728112);   // log(2 pi)
    }
}

}  // namespace

long gmm_scratch_floats(long rows, int k) {
    long per;
    int nwg;
    feat_partition(rows, &per, &nwg);
    return (long)nwg * ((long)k * GMM_SLAB + 2);
}

int launch_gmm_posterior(const float* scores, int in_layout, long rows, long plane, int k, float* lse, float* probs, int out_layout,
                         hipStream_t st) {
    GmmPostArgs a;
    a.scores = scores; a.lse = lse; a.probs = probs; a.rows = rows; a.k = k; a.in_layout = in_layout; a.out_layout = out_layout;
    a.plane = (in_layout == 1 || out_layout == 1) ? plane : 1;
    hipLaunchKernelGGL(gmm_posterior_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, a);
    return (int)hipGetLastError();
}

int launch_gmm_moments(const float* x, int x_layout, long rows, long plane, const float* scores, int k, const float* centres, float* slab,
                       hipStream_t st) {
    GmmMomArgs a;
    int nwg;
    feat_partition(rows, &a.tiles_per_wg, &nwg);
    a.x = x; a.scores = scores; a.centres = centres; a.slab = slab; a.rows = rows; a.plane = plane; a.k = k;
    if (x_layout == 0) hipLaunchKernelGGL(gmm_moments_kernel<0>, dim3((unsigned)nwg, (unsigned)k), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(gmm_moments_kernel<1>, dim3((unsigned)nwg, (unsigned)k), dim3(256), 0, st, a);
    return (int)hipGetLastError();
}

int launch_gmm_update(const float* slab, long rows, int k, int cov_kind, double reg_covar, double min_count, float* centres, float* tables,
                      float* covs, float* logdet, float* consts, float* weights, float* raw, float* record, hipStream_t st) {
    GmmUpdArgs a;
    long per;
    feat_partition(rows, &per, &a.nwg);
    a.slab = slab; a.centres = centres; a.tables = tables; a.covs = covs; a.logdet = logdet; a.consts = consts; a.weights = weights;
    a.raw = raw; a.record = record; a.reg_covar = reg_covar; a.min_count = min_count; a.k = k; a.diag = cov_kind == MSST_GMM_DIAG;
    if (int e = feat_allow_lds<&gmm_update_kernel>(GmmUpdLds::bytes)) return e;
    hipLaunchKernelGGL(gmm_update_kernel, dim3((unsigned)k), dim3(256), GmmUpdLds::bytes, st, a);
    return (int)hipGetLastError();
}

}  // namespace msst
