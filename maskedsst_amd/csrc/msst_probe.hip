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
// probe_grad  grid = workgroups of whole 64-row tiles (the partition depends on (rows, nc) only: probe_partition), 256 threads = 4 waves,
//             LDS (ncp = nc rounded up to 16, 32, 64 or 128): W o g [ncp][98] | x tile [64][100] | dl [64][DP] | small vectors.
//   tile      16-byte global loads one tile ahead in registers (as msst_knn.hip); rows past the slice are zero rows with dl = 0.
//   LN        four threads per row, channels 4 i + q: the 8 rows x 4 channels of a 32-lane group on 32 banks at pitch 100 (the
//             LayerNorm is three of the tile's four passes over LDS; the A-operand read of the logits pays a 2-way conflict
//             for it); xhat replaces x in LDS.
//   logits    wave w owns rows 16 w .. 16 w + 15: v_mfma_f32_16x16x4_f32, A = xhat[row l & 15][4 ks + (l >> 4)], B = (W o g)[class][k],
//             24 k-steps from the folded bias; lane l then holds rows 4 (l >> 4) + r, classes 16 jt + (l & 15).
//   softmax   per row over the 16 lanes of a class group (xor 1, 2, 4, 8): argmax with ties to the lowest class, exp, sum; dl = w_y (p - onehot)
//             goes to LDS; nll, w_y and the hit count stay on the lanes l & 15 == 0.
//   G1        the (class tile, channel tile) pairs are dealt round-robin to the 4 waves; each accumulates its pairs over ALL tiles of the
//             workgroup in registers: A = dl[row 4 ks + (l >> 4)][class], B = xhat[row 4 ks + (l >> 4)][channel], 16 k-steps per tile.
//   partials  the workgroup writes [dgamma 96 | dbeta 96 | dW nc x 96 | db nc | nll sum, weight sum, hits, 0] to its slab row.
// probe_update  32 elements x 8 slab slices per workgroup: slices summed in a fixed order, divided by the weight sum (summed by a
//             fixed tree in double), torch.optim.Adam; every workgroup keeps its own copy of the step counter (step[blockIdx.x]) so
//             that none reads what another writes.
// probe_fwd   the same LN + logits on 64 rows per workgroup, rows [Q][96] or the map [Bs][96][plane] read in place; logits staged in LDS
//             and stored by all threads as in knn_vote_kernel.
// No inline assembly.
#include "../../include/msst.h"
#include "msst_dev.h"
#include "msst_kernels.h"

#include <atomic>

namespace msst {

namespace {

constexpr int PB_D = 96;
constexpr int PB_XP = 100;             // LDS pitch of a feature row: 16-byte rows; (4 row + q) mod 32 distinct for the 8 rows x 4 q of a 32-lane group
constexpr int PB_WP = 98;              // LDS pitch of a weight row (msst_knn.hip)
constexpr int PB_MAX_WGS = 512;        // 256 CUs x 2
constexpr float PB_LN_EPS = 1e-5f;

__host__ __device__ constexpr int pb_dp(int nct) { return nct == 1 ? 16 : 16 * nct + 16; }   // = 16 mod 32: the two row groups of a 32-lane half on 32 banks
__host__ __device__ constexpr int pb_pairs_per_wave(int nct) { return (nct * 6 + 3) / 4; }

int pb_nct(int nc) { return nc <= 16 ? 1 : nc <= 32 ? 2 : nc <= 64 ? 4 : 8; }

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
    const float* beta = theta + PB_D;
    const float* W = theta + 2 * PB_D;
    const float* b = W + (long)nc * PB_D;
    for (int e = tid; e < ncp * PB_D; e += 256) {
        const int j = e / PB_D, k = e - j * PB_D;
        swg[j * PB_WP + k] = j < nc ? W[e] * gamma[k] : 0.f;
    }
    for (int j = tid; j < ncp; j += 256) {
        float s = 0.f;
        if (j < nc) {
            s = b[j];
            for (int k = 0; k < PB_D; ++k) s = fmaf(W[j * PB_D + k], beta[k], s);
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
    const float mean = s / PB_D;   // a division: the mean of a constant row is that constant whenever its sum is exact
    float d2 = 0.f;
#pragma unroll
    for (int i = 0; i < 24; ++i) {
        const float d = xr[4 * i] - mean;
        d2 = fmaf(d, d, d2);
    }
    d2 += __shfl_xor(d2, 1);
    d2 += __shfl_xor(d2, 2);
    const float rstd = 1.0f / sqrtf(d2 / PB_D + PB_LN_EPS);
#pragma unroll
    for (int i = 0; i < 24; ++i) xr[4 * i] = (xr[4 * i] - mean) * rstd;
    return !(d2 == d2) || !(fabsf(d2) <= 3.0e38f);
}

template <int NCT>
__device__ __forceinline__ void pb_logits(const float* xs, const float* swg, const float* sbias, int wave, int cc, int cg, f32x4* c) {
#pragma unroll
    for (int jt = 0; jt < NCT; ++jt) {
        const float bv = sbias[16 * jt + cc];
        c[jt][0] = bv; c[jt][1] = bv; c[jt][2] = bv; c[jt][3] = bv;
    }
    const float* xa = xs + (16 * wave + cc) * PB_XP + cg;
    const float* wb = swg + cc * PB_WP + cg;
#pragma unroll
    for (int ks = 0; ks < 24; ++ks) {
        const float a = xa[4 * ks];
#pragma unroll
        for (int jt = 0; jt < NCT; ++jt) c[jt] = PF32::mma(a, wb[16 * jt * PB_WP + 4 * ks], c[jt]);
    }
}

// the best (value, class) of a row over the 16 lanes of its class group; ties to the lowest class
__device__ __forceinline__ void pb_row_argmax(float& bv, int& bi) {
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) {
        const float ov = __shfl_xor(bv, m);
        const int oi = __shfl_xor(bi, m);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
}

__device__ __forceinline__ float pb_row_sum(float v) {
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 8);
    return v;
}

template <int NCT>
__global__ __launch_bounds__(256) void probe_grad_kernel(ProbeGradArgs a) {
    constexpr int NCP = 16 * NCT, DP = pb_dp(NCT), NPAIR = NCT * 6, PPW = pb_pairs_per_wave(NCT);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float* swg = reinterpret_cast<float*>(smem_raw);   // [NCP][PB_WP]; at the end G1 [NCP][PB_WP]
    float* xs = swg + NCP * PB_WP;                     // [64][PB_XP] (NCP PB_WP is a multiple of 4 floats: 16-byte rows)
    float* sdl = xs + 64 * PB_XP;                      // [64][DP]
    float* sbias = sdl + 64 * DP;                      // [NCP]
    float* scw = sbias + NCP;                          // [NCP]
    float* sred = scw + NCP;                           // [4][NCP] db of the waves | [NCP] db | [16][3] row sums
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cg = lane >> 4, cc = lane & 15;
    const int nc = a.nc;
    const int n = 2 * PB_D + (PB_D + 1) * nc;

    pb_fold_weights(a.theta, a.class_w, nc, NCP, swg, sbias, scw, tid);

    const long t0 = (long)blockIdx.x * a.tiles_per_wg;
    const long rbeg = t0 * 64;
    const long rend = min(a.rows, rbeg + a.tiles_per_wg * 64);
    const long ntiles = rend > rbeg ? (rend - rbeg + 63) / 64 : 0;
    const float* xbase = a.x + a.row0 * PB_D;
    const int32_t* lbase = a.labels + a.row0;

    f32x4 pre[6];
    auto load_tile = [&](long r0) {
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const int e = tid + 256 * i;
            const int row = e / 24, c4 = e - row * 24;
            const long r = r0 + row;
            pre[i] = r < rend ? *reinterpret_cast<const f32x4*>(xbase + r * PB_D + 4 * c4) : zero4();
        }
    };
    if (ntiles > 0) load_tile(rbeg);

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
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const int e = tid + 256 * i;
            const int row = e / 24, c4 = e - row * 24;
            *reinterpret_cast<f32x4*>(xs + row * PB_XP + 4 * c4) = pre[i];
        }
        __syncthreads();
        if (t + 1 < ntiles) load_tile(r0 + 64);
        pb_normalise(xs, tid);
        __syncthreads();
        f32x4 c[NCT];
        pb_logits<NCT>(xs, swg, sbias, wave, cc, cg, c);
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
            pb_row_argmax(bv, bi);
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
            ly = pb_row_sum(ly);
            se = pb_row_sum(se);
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
            const int p = wave + 4 * i;
            const int it = p / 6, jt = p - it * 6;
            if (p < NPAIR && 16 * it < nc) {
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
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
        const int p = wave + 4 * i;
        const int it = p / 6, jt = p - it * 6;
        if (p < NPAIR) {
#pragma unroll
            for (int r = 0; r < 4; ++r) swg[(16 * it + 4 * cg + r) * PB_WP + 16 * jt + cc] = acc[i][r];
        }
    }
    __syncthreads();
    float* sdb = sred + 4 * NCP;
    for (int j = tid; j < NCP; j += 256) sdb[j] = ((sred[j] + sred[NCP + j]) + sred[2 * NCP + j]) + sred[3 * NCP + j];
    __syncthreads();
    const float* gamma = a.theta;
    const float* beta = a.theta + PB_D;
    const float* W = a.theta + 2 * PB_D;
    float* out = a.slab + (long)blockIdx.x * (n + 4);
    for (int e = tid; e < nc * PB_D; e += 256) {
        const int j = e / PB_D, k = e - j * PB_D;
        out[2 * PB_D + e] = fmaf(swg[j * PB_WP + k], gamma[k], sdb[j] * beta[k]);
    }
    if (tid < PB_D) {
        float dg = 0.f, dbt = 0.f;
        for (int j = 0; j < nc; ++j) {
            const float w = W[j * PB_D + tid];
            dg = fmaf(w, swg[j * PB_WP + tid], dg);
            dbt = fmaf(w, sdb[j], dbt);
        }
        out[tid] = dg;
        out[PB_D + tid] = dbt;
    }
    for (int j = tid; j < nc; j += 256) out[2 * PB_D + nc * PB_D + j] = sdb[j];
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
    __shared__ double ssum[3][PB_MAX_WGS];
    __shared__ float spart[8][32];
    __shared__ float sbc[2];
    const int tid = threadIdx.x;
    const int n = 2 * PB_D + (PB_D + 1) * a.nc, P = n + 4;
    // ---- loss, weight sum and hits of the launch: a fixed tree over the workgroups' partials, in double
    for (int g = tid; g < PB_MAX_WGS; g += 256) {
        const bool in = g < a.nwg;
#pragma unroll
        for (int q = 0; q < 3; ++q) ssum[q][g] = in ? (double)a.slab[(long)g * P + n + q] : 0.0;
    }
    __syncthreads();
    for (int s = PB_MAX_WGS / 2; s > 0; s >>= 1) {
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
    constexpr int NCP = 16 * NCT, LP = NCP + 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float* swg = reinterpret_cast<float*>(smem_raw);   // [NCP][PB_WP]
    float* xs = swg + NCP * PB_WP;                     // [64][PB_XP]
    float* sl = xs + 64 * PB_XP;                       // [64][LP] logits
    float* sbias = sl + 64 * LP;                       // [NCP]
    int* sbad = reinterpret_cast<int*>(sbias + NCP);   // [64]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cg = lane >> 4, cc = lane & 15;
    const int nc = a.nc;
    const long q0 = (long)blockIdx.x * 64;
    const long nq = min((long)64, a.Q - q0);

    pb_fold_weights(a.theta, nullptr, nc, NCP, swg, sbias, nullptr, tid);
    if (a.x_layout == 0) {
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const int e = tid + 256 * i;
            const int row = e / 24, c4 = e - row * 24;
            *reinterpret_cast<f32x4*>(xs + row * PB_XP + 4 * c4) =
                row < nq ? *reinterpret_cast<const f32x4*>(a.x + (q0 + row) * PB_D + 4 * c4) : zero4();
        }
    } else {
        const int row = tid & 63;
        const long q = q0 + row;
        const bool in = row < nq;
        const long b = in ? q / a.plane : 0, p = in ? q - b * a.plane : 0;
        const float* src = a.x + b * PB_D * a.plane + p;
#pragma unroll
        for (int i = 0; i < 24; ++i) {
            const int d = 4 * i + (tid >> 6);
            xs[row * PB_XP + d] = in ? src[d * a.plane] : 0.f;
        }
    }
    __syncthreads();
    const bool bad = pb_normalise(xs, tid);
    if ((tid & 3) == 0) sbad[tid >> 2] = bad ? 1 : 0;
    __syncthreads();
    f32x4 c[NCT];
    pb_logits<NCT>(xs, swg, sbias, wave, cc, cg, c);
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
        pb_row_argmax(bv, bi);
        if (cc == 0 && rl < nq) a.classes[q0 + rl] = (rbad || bi == 0x7fffffff) ? -1 : bi;
    }
    __syncthreads();
    if (a.out_layout == 0) {
        for (long e = tid; e < nq * nc; e += 256) {
            const int ql = (int)(e / nc), cl = (int)(e - (long)ql * nc);
            a.logits[q0 * nc + e] = sl[ql * LP + cl];
        }
    } else {
        const int row = tid & 63;
        if (row < nq) {
            const long q = q0 + row;
            const long b = q / a.plane, p = q - b * a.plane;
            for (int cl = tid >> 6; cl < nc; cl += 4) a.logits[(b * nc + cl) * a.plane + p] = sl[row * LP + cl];
        }
    }
}

void probe_partition(long rows, long* tiles_per_wg, int* nwg) {
    const long tiles = (rows + 63) / 64;
    const long per = (tiles + PB_MAX_WGS - 1) / PB_MAX_WGS;
    *tiles_per_wg = per;
    *nwg = (int)((tiles + per - 1) / per);
}

size_t probe_grad_lds(int nct) { return (size_t)4 * (16 * nct * PB_WP + 64 * PB_XP + 64 * pb_dp(nct) + 2 * 16 * nct + 5 * 16 * nct + 48); }
size_t probe_fwd_lds(int nct) { return (size_t)4 * (16 * nct * PB_WP + 64 * PB_XP + 64 * (16 * nct + 1) + 16 * nct + 64); }

template <typename K>
int probe_set_lds(K kernel, size_t lds, std::atomic<bool>& done) {
    if (!done) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
        done = true;
    }
    return 0;
}

template <int NCT>
int probe_grad_launch(const ProbeGradArgs& a, int nwg, hipStream_t st) {
    static std::atomic<bool> done{false};
    const size_t lds = probe_grad_lds(NCT);
    if (int e = probe_set_lds(&probe_grad_kernel<NCT>, lds, done)) return e;
    hipLaunchKernelGGL(probe_grad_kernel<NCT>, dim3((unsigned)nwg), dim3(256), lds, st, a);
    return (int)hipGetLastError();
}

template <int NCT>
int probe_fwd_launch(const ProbeFwdArgs& a, hipStream_t st) {
    static std::atomic<bool> done{false};
    const size_t lds = probe_fwd_lds(NCT);
    if (int e = probe_set_lds(&probe_fwd_kernel<NCT>, lds, done)) return e;
    hipLaunchKernelGGL(probe_fwd_kernel<NCT>, dim3((unsigned)((a.Q + 63) / 64)), dim3(256), lds, st, a);
    return (int)hipGetLastError();
}

}  // namespace

long probe_scratch_floats(long rows, int nc) {
    long per;
    int nwg;
    probe_partition(rows, &per, &nwg);
    return (long)nwg * (2 * PB_D + (PB_D + 1) * nc + 4);
}

int launch_probe_grad(const float* x, const int32_t* labels, const float* class_w, const float* theta, long row0, long rows, int nc,
                      float* slab, hipStream_t st) {
    ProbeGradArgs a;
    int nwg;
    probe_partition(rows, &a.tiles_per_wg, &nwg);
    a.x = x; a.labels = labels; a.class_w = class_w; a.theta = theta; a.slab = slab; a.row0 = row0; a.rows = rows; a.nc = nc;
    switch (pb_nct(nc)) {
        case 1: return probe_grad_launch<1>(a, nwg, st);
        case 2: return probe_grad_launch<2>(a, nwg, st);
        case 4: return probe_grad_launch<4>(a, nwg, st);
        default: return probe_grad_launch<8>(a, nwg, st);
    }
}

int launch_probe_update(const float* slab, long rows, int nc, float* theta, float* m, float* v, int32_t* step, double lr, double beta1,
                        double beta2, double eps, double weight_decay, float* history_row, float* grad_out, int apply, hipStream_t st) {
    ProbeUpdateArgs a;
    long per;
    probe_partition(rows, &per, &a.nwg);
    a.slab = slab; a.theta = theta; a.m = m; a.v = v; a.step = step; a.hist = history_row; a.grad_out = grad_out;
    a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.wd = weight_decay; a.rows = rows; a.nc = nc; a.apply = apply;
    const int n = 2 * PB_D + (PB_D + 1) * nc;
    hipLaunchKernelGGL(probe_update_kernel, dim3((unsigned)((n + 31) / 32)), dim3(256), 0, st, a);
    return (int)hipGetLastError();
}

int launch_probe_fwd(const float* x, int x_layout, long Q, long plane, const float* theta, int nc, float* logits, int out_layout,
                     int64_t* classes, hipStream_t st) {
    ProbeFwdArgs a;
    a.x = x; a.theta = theta; a.logits = logits; a.classes = classes; a.Q = Q; a.plane = plane; a.nc = nc; a.x_layout = x_layout;
    a.out_layout = out_layout;
    switch (pb_nct(nc)) {
        case 1: return probe_fwd_launch<1>(a, st);
        case 2: return probe_fwd_launch<2>(a, st);
        case 4: return probe_fwd_launch<4>(a, st);
        default: return probe_fwd_launch<8>(a, st);
    }
}

}  // namespace msst
