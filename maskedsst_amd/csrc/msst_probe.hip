// The linear probe on cached features (msst_probe_grad, msst_probe_update, msst_probe_fwd; maskedsst_amd/probe.py): multinomial
// logistic regression through a trainable LayerNorm(96) with Adam on a bank x [M][96].  theta = [gamma 96 | beta 96 | W nc x 96 | b nc],
// the layout of the flat buffer's mlp_head segment.  No atomics, no host synchronisation; every output has the same bits in every call.
//
// One algebraic step keeps the kernels small.  With xhat the normalised row (two-pass fp32 statistics, eps 1e-5) and xn = xhat g + beta,
//   logits  = xn W^T + b            = xhat (W o g)^T + (b + W beta)        (W o g: column k of W times gamma[k], folded once per workgroup)
//   dW      = dl^T xn               = (dl^T xhat) o g + db (x) beta        db = sum over rows of dl
//   dgamma  = sum_rows (dl W) xhat  = sum_j W[j][.] (dl^T xhat)[j][.]
//   dbeta   = sum_rows dl W         = sum_j db[j] W[j][.]
// so ONE matrix product behind the softmax, G1 = dl^T xhat [nc][96], gives all four gradients; dxn = dl W is never formed.
//
// The tile loaders of both layouts, the scores loop, the order, the pairs, the table store and the partition are msst_feat.h's.
// probe_grad  grid = workgroups of whole 64-row tiles (feat_partition), 256 threads = 4 waves, LDS (ncp = nc rounded up to 16, 32, 64 or
//             128, ProbeGradLds): W o g [ncp][98] | x tile [64][100] | dl [64][DP] | small vectors.
//   tile      one tile ahead in registers; rows past the slice are zero rows with dl = 0.
//   LN        four threads per row, channels 4 i + q: the 8 rows x 4 channels of a 32-lane group on 32 banks at pitch 100 (the
//             LayerNorm is three of the tile's four passes over LDS; the A-operand read of the logits pays a 2-way conflict
//             for it); xhat replaces x in LDS.
//   logits    the scores of xhat against W o g, from the folded bias.
//   softmax   per row over the 16 lanes of a class group: argmax with ties to the lowest class, exp, sum; dl = w_y (p - onehot)
//             goes to LDS; nll, w_y and the hit count stay on the lanes l & 15 == 0.
//   G1        each wave accumulates its (class tile, channel tile) pairs over ALL tiles of the workgroup in registers: A = dl[row 4 ks + (l >> 4)][class], B = xhat[row 4 ks + (l >> 4)][channel], 16 k-steps per tile.
//   partials  the workgroup writes [dgamma 96 | dbeta 96 | dW nc x 96 | db nc | nll sum, weight sum, hits, 0] to its slab row.
// probe_update  32 elements x 8 slab slices per workgroup: slices summed in a fixed order, divided by the weight sum (summed by a
//             fixed tree in double), torch.optim.Adam; every workgroup keeps its own copy of the step counter (step[blockIdx.x]) so
//             that none reads what another writes.
// probe_fwd   the same LN + logits on 64 rows per workgroup, rows [Q][96] or the map [Bs][96][plane] read in place; logits staged in LDS
//             (ProbeFwdLds) and stored by all threads as rows or as a map.
// No inline assembly.
#include "../../include/msst.h"
#include "msst_feat.h"
#include "msst_kernels.h"

namespace msst {

namespace {

constexpr int PB_XP = 100;             // LDS pitch of a feature row: 16-byte rows; (4 row + q) mod 32 distinct for the 8 rows x 4 q of a 32-lane group
constexpr int PB_WP = 98;              // LDS pitch of a weight row
constexpr float PB_LN_EPS = 1e-5f;

__host__ __device__ constexpr int pb_dp(int nct) { return nct == 1 ? 16 : 16 * nct + 16; }   // = 16 mod 32: the two row groups of a 32-lane half on 32 banks

// the LDS of probe_grad_kernel<NCT> and of probe_fwd_kernel<NCT>, offsets in floats
template <int NCT>
struct ProbeGradLds {
    static constexpr int wg = 0;                            // [16 NCT][PB_WP] W o g; at the end G1
    static constexpr int x = wg + 16 * NCT * PB_WP;         // [64][PB_XP] (a multiple of 4 floats: 16-byte rows)
    static constexpr int dl = x + 64 * PB_XP;               // [64][pb_dp(NCT)]
    static constexpr int bias = dl + 64 * pb_dp(NCT);       // [16 NCT]
    static constexpr int cw = bias + 16 * NCT;              // [16 NCT]
    static constexpr int red = cw + 16 * NCT;               // [4][16 NCT] db of the waves | [16 NCT] db | [16][3] row sums
    static constexpr size_t bytes = (size_t)4 * (red + 5 * 16 * NCT + 48);
    static_assert(x % 4 == 0, "the x tile takes 16-byte stores");
};

template <int NCT>
struct ProbeFwdLds {
    static constexpr int LP = 16 * NCT + 1;                 // pitch of a logits row
    static constexpr int wg = 0;                            // [16 NCT][PB_WP]
    static constexpr int x = wg + 16 * NCT * PB_WP;         // [64][PB_XP]
    static constexpr int logits = x + 64 * PB_XP;           // [64][LP]
    static constexpr int bias = logits + 64 * LP;           // [16 NCT]
    static constexpr int bad = bias + 16 * NCT;             // [64] int
    static constexpr size_t bytes = (size_t)4 * (bad + 64);
    static_assert(x % 4 == 0, "the x tile takes 16-byte stores");
};

struct ProbeGradArgs {
    const float* x;
    const int32_t* labels;
    const float* class_w;   // null: every class weighs 1
    const float* theta;
    float* slab;
    long row0, rows, tiles_per_wg;
    int nc;
};

// W o g into LDS [ncp][PB_WP] (rows past nc zero), the folded bias b + W beta and (cw != null) the class weights
__device__ __forceinline__ void pb_fold_weights(const float* theta, const float* class_w, int nc, int ncp, float* swg, float* sbias,
                                                float* scw, int tid) {
    const float* gamma = theta;
    const float* beta = theta + FEAT_D;
    const float* W = theta + 2 * FEAT_D;
    const float* b = W + (long)nc * FEAT_D;
    for (int e = tid; e < ncp * FEAT_D; e += 256) {
        const int j = e / FEAT_D, k = e - j * FEAT_D;
        swg[j * PB_WP + k] = j < nc ? W[e] * gamma[k] : 0.f;
    }
    for (int j = tid; j < ncp; j += 256) {
        float s = 0.f;
        if (j < nc) {
            s = b[j];
            for (int k = 0; k < FEAT_D; ++k) s = fmaf(W[j * FEAT_D + k], beta[k], s);
        }
        sbias[j] = s;
        if (scw) scw[j] = j < nc ? (class_w ? class_w[j] : 1.0f) : 0.f;
    }
}

// LayerNorm statistics of the 64 rows of an LDS tile, four threads per row; xhat replaces x.  Returns whether the thread's row is
// not finite (a NaN or infinite channel).
__device__ __forceinline__ bool pb_normalise(float* xs, int tid) {
    float* xr = xs + (tid >> 2) * PB_XP + (tid & 3);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 24; ++i) s += xr[4 * i];
    s += __shfl_xor(s, 1);
    s += __shfl_xor(s, 2);
    const float mean = s / FEAT_D;   // a division: the mean of a constant row is that constant whenever its sum is exact
    float d2 = 0.f;
#pragma unroll
    for (int i = 0; i < 24; ++i) {
        const float d = xr[4 * i] - mean;
        d2 = fmaf(d, d, d2);
    }
    d2 += __shfl_xor(d2, 1);
    d2 += __shfl_xor(d2, 2);
    const float rstd = 1.0f / sqrtf(d2 / FEAT_D + PB_LN_EPS);
#pragma unroll
    for (int i = 0; i < 24; ++i) xr[4 * i] = (xr[4 * i] - mean) * rstd;
    return !(d2 == d2) || !(fabsf(d2) <= 3.0e38f);
}

// the accumulators of the logits at their start value, the folded bias
template <int NCT>
__device__ __forceinline__ void pb_bias_init(const float* sbias, int cc, f32x4 (&c)[NCT]) {
#pragma unroll
    for (int jt = 0; jt < NCT; ++jt) {
        const float bv = sbias[16 * jt + cc];
        c[jt][0] = bv; c[jt][1] = bv; c[jt][2] = bv; c[jt][3] = bv;
    }
}

template <int NCT>
__global__ __launch_bounds__(256) void probe_grad_kernel(ProbeGradArgs a) {
    constexpr int NCP = 16 * NCT, DP = pb_dp(NCT), PPW = feat_pairs_per_wave(NCT);
    using L = ProbeGradLds<NCT>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float* smem = reinterpret_cast<float*>(smem_raw);
    float *swg = smem + L::wg, *xs = smem + L::x, *sdl = smem + L::dl, *sbias = smem + L::bias, *scw = smem + L::cw, *sred = smem + L::red;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cg = lane >> 4, cc = lane & 15;
    const int nc = a.nc;
    const int n = 2 * FEAT_D + (FEAT_D + 1) * nc;

    pb_fold_weights(a.theta, a.class_w, nc, NCP, swg, sbias, scw, tid);

    const long t0 = (long)blockIdx.x * a.tiles_per_wg;
    const long rbeg = t0 * 64;
    const long rend = min(a.rows, rbeg + a.tiles_per_wg * 64);
    const long ntiles = rend > rbeg ? (rend - rbeg + 63) / 64 : 0;
    const float* xbase = a.x + a.row0 * FEAT_D;
    const int32_t* lbase = a.labels + a.row0;

    f32x4 pre[6];
    if (ntiles > 0) feat_rows_prefetch(pre, xbase, rbeg, rend, tid);

    f32x4 acc[PPW];
#pragma unroll
    for (int i = 0; i < PPW; ++i) acc[i] = zero4();
    float dbacc[NCT];
#pragma unroll
    for (int jt = 0; jt < NCT; ++jt) dbacc[jt] = 0.f;
    float loss_acc = 0.f, w_acc = 0.f, hit_acc = 0.f;

    for (long t = 0; t < ntiles; ++t) {
        const long r0 = rbeg + t * 64;
        __syncthreads();   // the previous tile's operand reads (and, first, the folded weights) are done
        feat_rows_store<PB_XP>(xs, pre, tid);
        __syncthreads();
        if (t + 1 < ntiles) feat_rows_prefetch(pre, xbase, r0 + 64, rend, tid);
        pb_normalise(xs, tid);
        __syncthreads();
        f32x4 c[NCT];
        pb_bias_init<NCT>(sbias, cc, c);
        feat_scores<NCT, PB_XP, PB_WP>(xs, swg, wave, cc, cg, c);
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
                if (cls < nc && c[jt][r] > bv) { bv = c[jt][r]; bi = cls; }
            }
            feat_group_argmax(bv, bi);
            const int y = valid ? lbase[row] : -1;
            const bool labelled = (unsigned)y < (unsigned)nc;   // a label outside [0, nc) weighs nothing
            const float wy = labelled ? scw[y] : 0.f;
            float ly = 0.f, se = 0.f;
#pragma unroll
            for (int jt = 0; jt < NCT; ++jt) {
                const int cls = 16 * jt + cc;
                const float l = c[jt][r];
                ly += cls == y ? l : 0.f;
                const float e = cls < nc ? expf(l - bv) : 0.f;
                c[jt][r] = e;
                se += e;
            }
            ly = feat_group_sum(ly);
            se = feat_group_sum(se);
            const float inv = 1.0f / se;
#pragma unroll
            for (int jt = 0; jt < NCT; ++jt) {
                const int cls = 16 * jt + cc;
                const float d = wy * (c[jt][r] * inv - (cls == y ? 1.0f : 0.f));
                sdl[rl * DP + cls] = d;
                dbacc[jt] += d;
            }
            if (cc == 0 && valid) {
                if (labelled) {
                    loss_acc += wy * (bv + logf(se) - ly);
                    w_acc += wy;
                }
                hit_acc += bi == y ? 1.0f : 0.f;
            }
        }
        __syncthreads();
        // ---- G1 += dl^T xhat over the tile's 64 rows
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            int it, jt;
            if (feat_wave_pair<NCT>(wave, i, it, jt) && 16 * it < nc) {
                const float* da = sdl + cg * DP + 16 * it + cc;
                const float* xb = xs + cg * PB_XP + 16 * jt + cc;
#pragma unroll
                for (int ks = 0; ks < 16; ++ks) acc[i] = PF32::mma(da[4 * ks * DP], xb[4 * ks * PB_XP], acc[i]);
            }
        }
    }
    __syncthreads();   // the folded weights are no longer read: their LDS takes G1

    // ---- the workgroup's partial sums
#pragma unroll
    for (int jt = 0; jt < NCT; ++jt) {
        float d = dbacc[jt];
        d += __shfl_xor(d, 16);
        d += __shfl_xor(d, 32);
        if (cg == 0) sred[wave * NCP + 16 * jt + cc] = d;
    }
    if (cc == 0) {
        float* s = sred + 5 * NCP + (4 * wave + cg) * 3;
        s[0] = loss_acc; s[1] = w_acc; s[2] = hit_acc;
    }
    feat_store_pairs<NCT, PB_WP>(swg, acc, NCP, wave, cc, cg);
    __syncthreads();
    float* sdb = sred + 4 * NCP;
    for (int j = tid; j < NCP; j += 256) sdb[j] = ((sred[j] + sred[NCP + j]) + sred[2 * NCP + j]) + sred[3 * NCP + j];
    __syncthreads();
    const float* gamma = a.theta;
    const float* beta = a.theta + FEAT_D;
    const float* W = a.theta + 2 * FEAT_D;
    float* out = a.slab + (long)blockIdx.x * (n + 4);
    for (int e = tid; e < nc * FEAT_D; e += 256) {
        const int j = e / FEAT_D, k = e - j * FEAT_D;
        out[2 * FEAT_D + e] = fmaf(swg[j * PB_WP + k], gamma[k], sdb[j] * beta[k]);
    }
    if (tid < FEAT_D) {
        float dg = 0.f, dbt = 0.f;
        for (int j = 0; j < nc; ++j) {
            const float w = W[j * FEAT_D + tid];
            dg = fmaf(w, swg[j * PB_WP + tid], dg);
            dbt = fmaf(w, sdb[j], dbt);
        }
        out[tid] = dg;
        out[FEAT_D + tid] = dbt;
    }
    for (int j = tid; j < nc; j += 256) out[2 * FEAT_D + nc * FEAT_D + j] = sdb[j];
    if (tid == 0) {
        float l = 0.f, w = 0.f, h = 0.f;
        for (int i = 0; i < 16; ++i) {
            const float* s = sred + 5 * NCP + i * 3;
            l += s[0]; w += s[1]; h += s[2];
        }
        out[n] = l; out[n + 1] = w; out[n + 2] = h; out[n + 3] = 0.f;
    }
}

struct ProbeUpdateArgs {
    const float* slab;
    float* theta;
    float* m;
    float* v;
    int32_t* step;
    float* hist;       // [4]: loss, weight sum, hits, rows
    float* grad_out;   // null or [n]
    double lr, beta1, beta2, eps, wd;
    long rows;
    int nc, nwg, apply;
};

__global__ __launch_bounds__(256) void probe_update_kernel(ProbeUpdateArgs a) {
    __shared__ double ssum[3][FEAT_MAX_WGS];
    __shared__ float spart[8][32];
    __shared__ float sbc[2];
    const int tid = threadIdx.x;
    const int n = 2 * FEAT_D + (FEAT_D + 1) * a.nc, P = n + 4;
    // ---- loss, weight sum and hits of the launch: a fixed tree over the workgroups' partials, in double
    for (int g = tid; g < FEAT_MAX_WGS; g += 256) {
        const bool in = g < a.nwg;
#pragma unroll
        for (int q = 0; q < 3; ++q) ssum[q][g] = in ? (double)a.slab[(long)g * P + n + q] : 0.0;
    }
    __syncthreads();
    for (int s = FEAT_MAX_WGS / 2; s > 0; s >>= 1) {
        for (int g = tid; g < s; g += 256) {
#pragma unroll
            for (int q = 0; q < 3; ++q) ssum[q][g] += ssum[q][g + s];
        }
        __syncthreads();
    }
    const double wsum = ssum[1][0];
    const bool go = wsum > 0.0;
    const int t = a.apply ? a.step[blockIdx.x] + 1 : 1;   // apply = 0 only reduces: step may be null
    if (tid == 0) {
        sbc[0] = (float)(1.0 - pow(a.beta1, (double)t));
        sbc[1] = (float)sqrt(1.0 - pow(a.beta2, (double)t));
    }
    // ---- the gradient's elements: 8 slices of the slab per element, combined in a fixed order
    const int el = tid & 31, slice = tid >> 5;
    const int e = blockIdx.x * 32 + el;
    float part = 0.f;
    if (e < n)
        for (int g = slice; g < a.nwg; g += 8) part += a.slab[(long)g * P + e];
    spart[slice][el] = part;
    __syncthreads();
    if (slice == 0 && e < n) {
        const float sum = ((spart[0][el] + spart[1][el]) + (spart[2][el] + spart[3][el])) +
                          ((spart[4][el] + spart[5][el]) + (spart[6][el] + spart[7][el]));
        float g = sum / (float)wsum;   // a launch without weight: NaN
        if (a.grad_out) a.grad_out[e] = g;
        if (go && a.apply) {
            const float b1 = (float)a.beta1, b2 = (float)a.beta2, ob1 = (float)(1.0 - a.beta1), ob2 = (float)(1.0 - a.beta2);
            const float th = a.theta[e];
            g = fmaf((float)a.wd, th, g);
            const float mm = fmaf(b1, a.m[e], ob1 * g);
            const float vv = fmaf(b2, a.v[e], ob2 * g * g);
            a.m[e] = mm;
            a.v[e] = vv;
            const float denom = sqrtf(vv) / sbc[1] + (float)a.eps;
            a.theta[e] = th - ((float)a.lr / sbc[0]) * (mm / denom);
        }
    }
    if (tid == 0) {
        if (go && a.apply) a.step[blockIdx.x] = t;
        if (blockIdx.x == 0) {
            a.hist[0] = go ? (float)(ssum[0][0] / wsum) : __builtin_nanf("");
            a.hist[1] = (float)wsum;
            a.hist[2] = (float)ssum[2][0];
            a.hist[3] = (float)a.rows;
        }
    }
}

struct ProbeFwdArgs {
    const float* x;
    const float* theta;
    float* logits;
    int64_t* classes;
    long Q, plane;
    int nc, x_layout, out_layout;
};

template <int NCT>
__global__ __launch_bounds__(256) void probe_fwd_kernel(ProbeFwdArgs a) {
    using L = ProbeFwdLds<NCT>;
    constexpr int NCP = 16 * NCT, LP = L::LP;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float* smem = reinterpret_cast<float*>(smem_raw);
    float *swg = smem + L::wg, *xs = smem + L::x, *sl = smem + L::logits, *sbias = smem + L::bias;
    int* sbad = reinterpret_cast<int*>(smem + L::bad);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cg = lane >> 4, cc = lane & 15;
    const int nc = a.nc;
    const long q0 = (long)blockIdx.x * 64;
    const long nq = min((long)64, a.Q - q0);

    pb_fold_weights(a.theta, nullptr, nc, NCP, swg, sbias, nullptr, tid);
    f32x4 pre[6];
    if (a.x_layout == 0) {
        feat_rows_prefetch(pre, a.x, q0, q0 + nq, tid);
        feat_rows_store<PB_XP>(xs, pre, tid);
    } else {
        feat_map_prefetch(pre, a.x, a.plane, q0, q0 + nq, tid);
        feat_map_store<PB_XP>(xs, pre, tid);
    }
    __syncthreads();
    const bool bad = pb_normalise(xs, tid);
    if ((tid & 3) == 0) sbad[tid >> 2] = bad ? 1 : 0;
    __syncthreads();
    f32x4 c[NCT];
    pb_bias_init<NCT>(sbias, cc, c);
    feat_scores<NCT, PB_XP, PB_WP>(xs, swg, wave, cc, cg, c);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int rl = 16 * wave + 4 * cg + r;
        const bool rbad = sbad[rl] != 0;
        float bv = -INFINITY;
        int bi = 0x7fffffff;
#pragma unroll
        for (int jt = 0; jt < NCT; ++jt) {
            const int cls = 16 * jt + cc;
            const float l = rbad ? __builtin_nanf("") : c[jt][r];
            sl[rl * LP + cls] = l;
            if (cls < nc && l > bv) { bv = l; bi = cls; }
        }
        feat_group_argmax(bv, bi);
        if (cc == 0 && rl < nq) a.classes[q0 + rl] = (rbad || bi == 0x7fffffff) ? -1 : bi;
    }
    __syncthreads();
    feat_store_table<256>(sl, LP, a.logits, a.out_layout, q0, nq, nc, a.plane, tid);
}

template <int NCT>
int probe_grad_launch(const ProbeGradArgs& a, int nwg, hipStream_t st) {
    constexpr size_t lds = ProbeGradLds<NCT>::bytes;
    if (int e = feat_allow_lds<&probe_grad_kernel<NCT>>(lds)) return e;
    hipLaunchKernelGGL(probe_grad_kernel<NCT>, dim3((unsigned)nwg), dim3(256), lds, st, a);
    return (int)hipGetLastError();
}

template <int NCT>
int probe_fwd_launch(const ProbeFwdArgs& a, hipStream_t st) {
    constexpr size_t lds = ProbeFwdLds<NCT>::bytes;
    if (int e = feat_allow_lds<&probe_fwd_kernel<NCT>>(lds)) return e;
    hipLaunchKernelGGL(probe_fwd_kernel<NCT>, dim3((unsigned)((a.Q + 63) / 64)), dim3(256), lds, st, a);
    return (int)hipGetLastError();
}

}  // namespace

long probe_scratch_floats(long rows, int nc) {
    long per;
    int nwg;
    feat_partition(rows, &per, &nwg);
    return (long)nwg * (2 * FEAT_D + (FEAT_D + 1) * nc + 4);
}

int launch_probe_grad(const float* x, const int32_t* labels, const float* class_w, const float* theta, long row0, long rows, int nc,
                      float* slab, hipStream_t st) {
    ProbeGradArgs a;
    int nwg;
    feat_partition(rows, &a.tiles_per_wg, &nwg);
    a.x = x; a.labels = labels; a.class_w = class_w; a.theta = theta; a.slab = slab; a.row0 = row0; a.rows = rows; a.nc = nc;
    return feat_dispatch_nct(nc, [&](auto n) { return probe_grad_launch<decltype(n)::value>(a, nwg, st); });
}

int launch_probe_update(const float* slab, long rows, int nc, float* theta, float* m, float* v, int32_t* step, double lr, double beta1,
                        double beta2, double eps, double weight_decay, float* history_row, float* grad_out, int apply, hipStream_t st) {
    ProbeUpdateArgs a;
    long per;
    feat_partition(rows, &per, &a.nwg);
    a.slab = slab; a.theta = theta; a.m = m; a.v = v; a.step = step; a.hist = history_row; a.grad_out = grad_out;
    a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.wd = weight_decay; a.rows = rows; a.nc = nc; a.apply = apply;
    const int n = 2 * FEAT_D + (FEAT_D + 1) * nc;
    hipLaunchKernelGGL(probe_update_kernel, dim3((unsigned)((n + 31) / 32)), dim3(256), 0, st, a);
    return (int)hipGetLastError();
}

int launch_probe_fwd(const float* x, int x_layout, long Q, long plane, const float* theta, int nc, float* logits, int out_layout,
                     int64_t* classes, hipStream_t st) {
    ProbeFwdArgs a;
    a.x = x; a.theta = theta; a.logits = logits; a.classes = classes; a.Q = Q; a.plane = plane; a.nc = nc; a.x_layout = x_layout;
    a.out_layout = out_layout;
    return feat_dispatch_nct(nc, [&](auto n) { return probe_fwd_launch<decltype(n)::value>(a, st); });
}

}  // namespace msst
