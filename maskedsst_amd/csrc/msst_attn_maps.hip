// Attention maps (msst_attn_maps; ViTSpatialSpectral.attention_maps): the probabilities P = softmax(q k^T dim_head^-0.5) of one
// block, q = LN1(x) Wq^T, k = LN1(x) Wk^T, from the block's INPUT x -- the reference's `attn` (vit_spatial_spectral.py:67-74) before
// dropout.  The block kernels keep P in registers; this kernel recomputes it in exact fp32 whatever the model's precision.
//
// attn_maps   one workgroup per (sample, head), 256 threads = 4 waves, 125,696 bytes of LDS (one workgroup per CU).
//   prologue  Wq_h and Wk_h (64 x 96 each) from the fp32 master to_qkv.weight into LDS; Wq_h is multiplied by dim_head^-0.5 = 1/8
//             on the way (a power of two: exact), so the score GEMM needs no scale.
//   per 64-row tile of the sample (TS = 64 / L whole sequences, TileMap's packing restricted to one sample):
//     1. rows -> LN1 -> xn [64][96]: four lanes per row, 16-byte loads, two-pass mean / variance (DPP quad sums), eps 1e-5.
//        Padding rows (slot >= TS, or a sequence past the sample's G) are not read: their xn is zero.
//     2. q, k = xn Wq^T, xn Wk^T on v_mfma_f32_16x16x4_f32: wave w owns rows 16 w .. 16 w + 15 and all 2 x 4 feature tiles; the
//        weights are the A operand and the rows the B operand (one B fragment per k-step shared by the eight MFMAs), so a lane
//        holds four consecutive features of one row and the C tiles go to LDS row-major [row][dh] as 8-byte stores.
//     3. s = q k^T (16 k-steps), wave w again the 16 query rows x 64 keys.  A key of another sequence is masked (-inf); row maximum
//        and row sum over the 4 column tiles of a lane and then the 16 lanes of a lane group (the C layout: row = 4 (lane >> 4) + r,
//        column = lane & 15); p = exp(s - max) * (1 / sum) -> LDS [64][64].
//     4. MSST_ATTN_PER_SEQ: the diagonal L x L blocks are stored, consecutive threads on consecutive floats of a map.
//        MSST_ATTN_MEAN_SEQ: thread t owns elements t, t + 256, ... of the L x L result (at most 16) in registers and adds the
//        tile's sequences in slot order; after the last tile it divides by (float)G and stores.
//   The sum over a sample's sequences therefore runs in one workgroup in the order g = 0 .. G - 1 from 0: no atomics, nothing to
//   zero, the same bits in every call and in every batch the sample sits in.
// LDS pitches: the k-contiguous fp32 operand load reads element (row = lane & 15, k = lane >> 4); a 32-lane half (the conflict
// group of a one-dword read, 32 banks) holds 16 rows x 2 k, bank (pitch row + k) % 32: pitch 98 / 66 (= 2 mod 32) makes the 32
// distinct, where the pitch 100 / 68 of the 16-byte-aligned rows elsewhere would put rows r and r + 8 on one bank.  The probability
// tile has pitch 65 so that the row-wise reads of step 4 walk the banks.
// No inline assembly.
#include "../../include/msst.h"
#include "msst_dev.h"
#include "msst_kernels.h"
#include <atomic>

namespace msst {

namespace {

constexpr int AM_XP = 98;    // pitch of xn, Wq, Wk rows (96 floats)
constexpr int AM_QP = 66;    // pitch of q, k rows (64 floats)
constexpr int AM_PP = 65;    // pitch of the probability tile
constexpr int AM_ACC = 16;   // 64 * 64 / 256 elements of the mean per thread

struct AttnMapsSmem {
    float wq[64 * AM_XP], wk[64 * AM_XP];
    float xn[64 * AM_XP];
    float q[64 * AM_QP], k[64 * AM_QP];
    float p[64 * AM_PP];
};

struct AttnMapsArgs {
    const float* x;
    const float* ln_g;
    const float* ln_b;
    const float* wqkv;
    float* maps;
    long sample_stride;
    int mode, S, N, heads, reduce;
};

__global__ __launch_bounds__(256) void attn_maps_kernel(AttnMapsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    AttnMapsSmem& sm = *reinterpret_cast<AttnMapsSmem*>(smem_raw);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long b = blockIdx.x;
    const int h = blockIdx.y;
    const int S = a.S, N = a.N;
    const int L = a.mode == 0 ? N : S, G = a.mode == 0 ? S : N;
    const int TS = 64 / L, LL = L * L;
    const int ntiles = (G + TS - 1) / TS;
    const long T = (long)S * N;
    const float* xb = a.x + b * T * 96;

    // ---- prologue: the head's Wq (scaled by dim_head^-0.5) and Wk
    {
        const float* wq = a.wqkv + (long)h * 64 * 96;
        const float* wk = a.wqkv + ((long)a.heads + h) * 64 * 96;
        for (int e = tid; e < 64 * 96; e += 256) {
            const int d = e / 96, c = e - d * 96;
            sm.wq[d * AM_XP + c] = wq[e] * 0.125f;
            sm.wk[d * AM_XP + c] = wk[e];
        }
    }

    // the mean's elements of this thread: e = tid + 256 m -> (i, j), offset into a sequence's diagonal block of the probability tile
    float acc[AM_ACC];
    int poff[AM_ACC];
#pragma unroll
    for (int m = 0; m < AM_ACC; ++m) {
        const int e = tid + 256 * m;
        const int i = e / L, j = e - i * L;
        acc[m] = 0.f;
        poff[m] = i * AM_PP + j;
    }

    // row of the LN phase: four lanes per row
    const int lrow = tid >> 2, lq = tid & 3;
    const int lslot = lrow / L, lpos = lrow - lslot * L;
    // rows of the softmax phase: C layout
    const int cg = lane >> 4, cc = lane & 15;

    for (int tile = 0; tile < ntiles; ++tile) {
        const int g0 = tile * TS;
        const int nvalid = min(TS, G - g0);   // sequences of this tile
        // ---- 1. LN1 of the tile's rows
        {
            const int g = g0 + lslot;
            const bool valid = lslot < nvalid;
            const long tok = a.mode == 0 ? (long)g * N + lpos : (long)lpos * N + g;
            f32x4 v[6];
            float s = 0.f;
#pragma unroll
            for (int m = 0; m < 6; ++m) {
                v[m] = valid ? *reinterpret_cast<const f32x4*>(xb + tok * 96 + 4 * (lq + 4 * m)) : zero4();
                s += (v[m][0] + v[m][1]) + (v[m][2] + v[m][3]);
            }
            const float mean = quad_sum(s) * (1.0f / 96.0f);
            float ss = 0.f;
#pragma unroll
            for (int m = 0; m < 6; ++m) {
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    v[m][t] -= mean;
                    ss += v[m][t] * v[m][t];
                }
            }
            const float rstd = 1.0f / sqrtf(quad_sum(ss) * (1.0f / 96.0f) + 1e-5f);
            float* dst = sm.xn + lrow * AM_XP;
#pragma unroll
            for (int m = 0; m < 6; ++m) {
                const int c0 = 4 * (lq + 4 * m);
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    dst[c0 + t] = valid ? v[m][t] * rstd * a.ln_g[c0 + t] + a.ln_b[c0 + t] : 0.f;
            }
        }
        __syncthreads();   // xn (and, first tile, the weights) written; the previous tile's readers of q, k, p are done (barrier below)
        // ---- 2. q, k of rows 16 wave .. + 15: weights are the A operand, rows the B operand, so a lane holds four consecutive
        //         features of one row (C[feature 4 (lane >> 4) + r][row lane & 15])
        {
            f32x4 cq[4], ck[4];
#pragma unroll
            for (int it = 0; it < 4; ++it) { cq[it] = zero4(); ck[it] = zero4(); }
            const float* brow = sm.xn + 16 * wave * AM_XP;
#pragma unroll 2
            for (int k0 = 0; k0 < 96; k0 += 4) {
                const float bf = PF32::ld_kc(brow + k0, AM_XP);
#pragma unroll
                for (int it = 0; it < 4; ++it) {
                    cq[it] = PF32::mma(PF32::ld_kc(sm.wq + 16 * it * AM_XP + k0, AM_XP), bf, cq[it]);
                    ck[it] = PF32::mma(PF32::ld_kc(sm.wk + 16 * it * AM_XP + k0, AM_XP), bf, ck[it]);
                }
            }
            // rows of pitch 66 floats start on 8 bytes: two 8-byte stores per C tile
            float* qd = sm.q + (16 * wave + cc) * AM_QP + 4 * cg;
            float* kd = sm.k + (16 * wave + cc) * AM_QP + 4 * cg;
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                *reinterpret_cast<float2*>(qd + 16 * it) = make_float2(cq[it][0], cq[it][1]);
                *reinterpret_cast<float2*>(qd + 16 * it + 2) = make_float2(cq[it][2], cq[it][3]);
                *reinterpret_cast<float2*>(kd + 16 * it) = make_float2(ck[it][0], ck[it][1]);
                *reinterpret_cast<float2*>(kd + 16 * it + 2) = make_float2(ck[it][2], ck[it][3]);
            }
        }
        __syncthreads();
        // ---- 3. scores and softmax of query rows 16 wave .. + 15
        {
            f32x4 cs[4];
#pragma unroll
            for (int jt = 0; jt < 4; ++jt) cs[jt] = zero4();
            const float* arow = sm.q + 16 * wave * AM_QP;
#pragma unroll 2
            for (int k0 = 0; k0 < 64; k0 += 4) {
                const float af = PF32::ld_kc(arow + k0, AM_QP);
#pragma unroll
                for (int jt = 0; jt < 4; ++jt)
                    cs[jt] = PF32::mma(af, PF32::ld_kc(sm.k + 16 * jt * AM_QP + k0, AM_QP), cs[jt]);
            }
            int kslot[4];
#pragma unroll
            for (int jt = 0; jt < 4; ++jt) kslot[jt] = (16 * jt + cc) / L;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * wave + 4 * cg + r;
                const int rslot = row / L;
                const bool rvalid = rslot < nvalid;
                float mx = -INFINITY;
#pragma unroll
                for (int jt = 0; jt < 4; ++jt) {
                    if (kslot[jt] != rslot) cs[jt][r] = -INFINITY;
                    mx = fmaxf(mx, cs[jt][r]);
                }
                mx = fmaxf(mx, __shfl_xor(mx, 1));
                mx = fmaxf(mx, __shfl_xor(mx, 2));
                mx = fmaxf(mx, __shfl_xor(mx, 4));
                mx = fmaxf(mx, __shfl_xor(mx, 8));
                if (!rvalid) mx = 0.f;   // a padding row (every key masked): keep the arithmetic finite, nothing of it is stored
                float e[4], sum = 0.f;
#pragma unroll
                for (int jt = 0; jt < 4; ++jt) {
                    e[jt] = expf(cs[jt][r] - mx);
                    sum += e[jt];
                }
                sum = rowgroup_sum(sum);
                const float inv = rvalid ? 1.0f / sum : 0.f;
#pragma unroll
                for (int jt = 0; jt < 4; ++jt) sm.p[row * AM_PP + 16 * jt + cc] = rvalid ? e[jt] * inv : 0.f;
            }
        }
        __syncthreads();
        // ---- 4. the diagonal blocks
        if (a.reduce == MSST_ATTN_PER_SEQ) {
            float* out = a.maps + b * a.sample_stride;
            for (int e = tid; e < nvalid * LL; e += 256) {
                const int s = e / LL, rem = e - s * LL;
                const int i = rem / L, j = rem - i * L;
                out[((long)(g0 + s) * a.heads + h) * LL + rem] = sm.p[(s * L + i) * AM_PP + s * L + j];
            }
        } else {
            for (int s = 0; s < nvalid; ++s) {
                const float* blk = sm.p + s * L * (AM_PP + 1);
#pragma unroll
                for (int m = 0; m < AM_ACC; ++m)
                    if (tid + 256 * m < LL) acc[m] += blk[poff[m]];
            }
        }
        // (the next tile's step 1 writes xn only, which steps 3 and 4 do not read; its first barrier orders q, k, p)
    }
    if (a.reduce == MSST_ATTN_MEAN_SEQ) {
        float* out = a.maps + b * a.sample_stride + (long)h * LL;
        const float fG = (float)G;
#pragma unroll
        for (int m = 0; m < AM_ACC; ++m)
            if (tid + 256 * m < LL) out[tid + 256 * m] = acc[m] / fG;
    }
}

}  // namespace

int launch_attn_maps(const float* x, const float* ln_g, const float* ln_b, const float* wqkv, float* maps, long sample_stride,
                     int mode, int B, int S, int N, int heads, int reduce, hipStream_t st) {
    if (N > 64 || S > 64 || heads > 16) return MSST_ERR_UNSUPPORTED;
    static std::atomic<bool> attr_set{false};
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_maps_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)sizeof(AttnMapsSmem));
        if (e != hipSuccess) return (int)e;
        attr_set = true;
    }
    AttnMapsArgs a;
    a.x = x; a.ln_g = ln_g; a.ln_b = ln_b; a.wqkv = wqkv; a.maps = maps; a.sample_stride = sample_stride;
    a.mode = mode; a.S = S; a.N = N; a.heads = heads; a.reduce = reduce;
    hipLaunchKernelGGL(attn_maps_kernel, dim3((unsigned)B, (unsigned)heads), dim3(256), sizeof(AttnMapsSmem), st, a);
    return (int)hipGetLastError();
}

}  // namespace msst
