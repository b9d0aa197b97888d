// Spectral MLP classification head (reference vit_spatial_spectral.py:440-453, :536-564 with spectral_mlp_head=True):
// 'b (c h w) d -> b h w (c d)' (NO mean over c: feature j = c * 96 + d), LayerNorm(96 S), Linear(96 S -> n_classes);
// logits [B][n_classes][N], the layout of cls_head_fwd_kernel.  fp32 throughout, VALU (no MFMA: see DESIGN.md 8).
//
// A row is one spatial position (b, n) of one sample: F = 96 S features gathered from the S tokens y[b, c N + n, :], each a
// contiguous 384-byte slice.  Row mapping of the two row kernels: one wave owns RPW rows at once; lane l holds the float4
// pieces q = l + 64 i (i < NQ) of every one of them (piece q = token q / 24, floats 4 (q % 24) .. + 3), so the row
// statistics and the per-class dot products are wave-shuffle reductions, and every W / gamma / beta float4 a lane loads
// serves its RPW rows.  W (n_classes x F, up to 786 KB) is streamed through the caches in those per-lane K slices, one
// class row at a time; it is never staged whole.
//
// Backward, three launches plus the shared fixed-order reduction:
//   spec_head_bwd_rows:  per row, dxn = W^T dl, LayerNorm backward dx = rstd (g - mean(g) - xhat mean(g xhat)), g = gamma dxn,
//                        scattered back to the S tokens (dy fully written, no 1/S factor); the row's (mean, rstd) are kept
//                        (store_row_stats: arithmetic pinned with explicit fmaf, the same bits from either variant).
//                        With a null dy (a frozen body: nobody consumes it) the variant compiled without all of that runs: it
//                        reads the rows and keeps their (mean, rstd), the only thing the weight-gradient pass takes from here, so
//                        the four head gradients are bit-identical.
//   spec_head_wgrad:     A[k][j] = sum_rows dl[k] xhat[j] and sum_rows dl[k], per (token c, row chunk g) workgroup into slab g.
//                        The row chunks are a static partition of the B N rows (spec_head_chunks: depends on B N only), so
//                        every partial sums the same rows in the same order on every device.
//   launch_reduce_segs:  the G slabs -> A, db (fixed slab order).
//   spec_head_wgrad_finish: dW = gamma A + beta db^T, dgamma = sum_k W A, dbeta = sum_k W db (xn = gamma xhat + beta, dxn = W^T dl).
// No float atomics anywhere: the results are bitwise reproducible run to run and independent of the CU count.
#include "msst_dev.h"
#include "msst_kernels.h"

namespace msst {

namespace {

__device__ __forceinline__ float wave_sum64(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;   // the butterfly leaves the same bits on every lane (each step adds the same two values on both partners)
}

__device__ __forceinline__ float dot4(f32x4 a, f32x4 b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3]; }
__device__ __forceinline__ float sum4(f32x4 a) { return (a[0] + a[1]) + (a[2] + a[3]); }

// float offset of piece q of row (b, n) relative to y + b T 96 + n 96
__device__ __forceinline__ long piece_off(int q, int N) {
    const int c = q / 24;
    return (long)c * N * 96 + (q - c * 24) * 4;
}

// loads the RPW rows of a wave into v, returns their (mean, rstd) (two-pass, biased variance, eps 1e-5 as nn.LayerNorm)
template <int NQ, int RPW>
__device__ __forceinline__ void load_rows(const SpecHeadArgs& a, int row0, int lane, f32x4 (&v)[RPW][NQ], float (&mean)[RPW],
                                          float (&rstd)[RPW]) {
    const int F4 = a.S * 24;
    const float invF = 1.f / (float)(a.S * 96);
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        const int row = row0 + r;
        const bool ok = row < a.R;
        const int b = ok ? row / a.N : 0, n = ok ? row - b * a.N : 0;
        const float* base = a.y + ((long)b * a.T + n) * 96;
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            const int q = lane + 64 * i;
            v[r][i] = (ok && q < F4) ? *reinterpret_cast<const f32x4*>(base + piece_off(q, a.N)) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NQ; ++i) s += sum4(v[r][i]);
        mean[r] = wave_sum64(s) * invF;
    }
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            if (lane + 64 * i < F4) {
                const f32x4 d = v[r][i] - mean[r];
                s += dot4(d, d);
            }
        }
        rstd[r] = rsqrtf(wave_sum64(s) * invF + 1e-5f);
    }
}

// (mean, rstd) of the RPW rows in v -> stats, as the weight-gradient pass reads them.  Written with explicit fmaf and nothing else
// that could contract: which products the compiler fuses otherwise depends on what else the calling kernel computes, and the
// with-dy and the no-dy variant of the row backward must leave the same bits here (their head gradients are compared bit for bit).
template <int NQ, int RPW>
__device__ __forceinline__ void store_row_stats(const SpecHeadArgs& a, int row0, int lane, const f32x4 (&v)[RPW][NQ]) {
    const int F4 = a.S * 24;
    const float invF = 1.f / (float)(a.S * 96);
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NQ; ++i) s += sum4(v[r][i]);
        const float ws = wave_sum64(s);
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            if (lane + 64 * i < F4) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float d = __builtin_fmaf(-ws, invF, v[r][i][e]);
                    q = __builtin_fmaf(d, d, q);
                }
            }
        }
        const float rstd = rsqrtf(__builtin_fmaf(wave_sum64(q), invF, 1e-5f));
        if (lane == 0 && row0 + r < a.R) { a.stats[2 * (row0 + r)] = ws * invF; a.stats[2 * (row0 + r) + 1] = rstd; }
    }
}

}  // namespace

// grid (ceil(R / (4 RPW))), 256 threads
template <int NQ, int RPW>
__global__ __launch_bounds__(256) void spec_head_fwd_kernel(SpecHeadArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row0 = (blockIdx.x * 4 + wave) * RPW;
    if (row0 >= a.R) return;   // (wave uniform)
    const int F4 = a.S * 24, F = a.S * 96;
    f32x4 v[RPW][NQ];
    float mean[RPW], rstd[RPW];
    load_rows<NQ, RPW>(a, row0, lane, v, mean, rstd);
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        const int q = lane + 64 * i;
        if (q < F4) {
            const f32x4 g4 = *reinterpret_cast<const f32x4*>(a.ln_g + 4 * q), b4 = *reinterpret_cast<const f32x4*>(a.ln_b + 4 * q);
#pragma unroll
            for (int r = 0; r < RPW; ++r) v[r][i] = (v[r][i] - mean[r]) * rstd[r] * g4 + b4;
        }
    }
    // four classes per pass: their W loads and wave reductions are independent, so their latencies overlap
    for (int k0 = 0; k0 < a.NC; k0 += 4) {
        float acc[4][RPW];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int r = 0; r < RPW; ++r) acc[u][r] = 0.f;
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            const int q = lane + 64 * i;
            if (q < F4) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (k0 + u < a.NC) {
                        const f32x4 w4 = *reinterpret_cast<const f32x4*>(a.w + (long)(k0 + u) * F + 4 * q);
#pragma unroll
                        for (int r = 0; r < RPW; ++r) acc[u][r] += dot4(w4, v[r][i]);
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int r = 0; r < RPW; ++r) {
                const float s = wave_sum64(acc[u][r]);
                const int row = row0 + r, k = k0 + u;
                if (lane == 0 && row < a.R && k < a.NC) {
                    const int b = row / a.N, n = row - b * a.N;
                    a.logits[((long)b * a.NC + k) * a.N + n] = s + a.b[k];
                }
            }
        }
    }
}

// grid (ceil(R / (4 RPW))), 256 threads
template <int NQ, int RPW, bool WANT_DY>
__global__ __launch_bounds__(256) void spec_head_bwd_rows_kernel(SpecHeadArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row0 = (blockIdx.x * 4 + wave) * RPW;
    if (row0 >= a.R) return;   // (wave uniform)
    const int F4 = a.S * 24, F = a.S * 96;
    const float invF = 1.f / (float)F;
    f32x4 v[RPW][NQ], d[RPW][NQ];
    float mean[RPW], rstd[RPW];
    load_rows<NQ, RPW>(a, row0, lane, v, mean, rstd);
    store_row_stats<NQ, RPW>(a, row0, lane, v);
    if constexpr (!WANT_DY) return;
    int bb[RPW], nn[RPW];
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        const int row = row0 + r < a.R ? row0 + r : 0;
        bb[r] = row / a.N;
        nn[r] = row - bb[r] * a.N;
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            v[r][i] = (v[r][i] - mean[r]) * rstd[r];   // xhat (pieces past F stay unused)
            d[r][i] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    // dxn = W^T dl
    // four classes per pass (independent loads in flight); each d element still accumulates the classes in order k = 0, 1, ...
    for (int k0 = 0; k0 < a.NC; k0 += 4) {
        float dl[4][RPW];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int r = 0; r < RPW; ++r)
                dl[u][r] = k0 + u < a.NC ? a.dlogits[((long)bb[r] * a.NC + k0 + u) * a.N + nn[r]] : 0.f;
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            const int q = lane + 64 * i;
            if (q < F4) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (k0 + u < a.NC) {
                        const f32x4 w4 = *reinterpret_cast<const f32x4*>(a.w + (long)(k0 + u) * F + 4 * q);
#pragma unroll
                        for (int r = 0; r < RPW; ++r) d[r][i] += dl[u][r] * w4;
                    }
                }
            }
        }
    }
    float g1[RPW], g2[RPW];
#pragma unroll
    for (int r = 0; r < RPW; ++r) { g1[r] = 0.f; g2[r] = 0.f; }
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        const int q = lane + 64 * i;
        if (q < F4) {
            const f32x4 g4 = *reinterpret_cast<const f32x4*>(a.ln_g + 4 * q);
#pragma unroll
            for (int r = 0; r < RPW; ++r) {
                d[r][i] *= g4;
                g1[r] += sum4(d[r][i]);
                g2[r] += dot4(d[r][i], v[r][i]);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        const int row = row0 + r;
        const float m1 = wave_sum64(g1[r]) * invF, m2 = wave_sum64(g2[r]) * invF;
        if (row >= a.R) continue;
        float* base = a.dy + ((long)bb[r] * a.T + nn[r]) * 96;
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            const int q = lane + 64 * i;
            if (q < F4) *reinterpret_cast<f32x4*>(base + piece_off(q, a.N)) = rstd[r] * (d[r][i] - m1 - v[r][i] * m2);
        }
    }
}

// grid (S, G), 192 threads = 8 row slots x 24 float4 lanes of one token's 96 features.  Slab g: [NC][F] A partials, then NC dl sums
// (written by the c == 0 workgroup of the chunk).  NCB: n_classes rounded up to the accumulator count.
template <int NCB>
__global__ __launch_bounds__(192) void spec_head_wgrad_kernel(SpecHeadArgs a) {
    __shared__ float dl_s[64][NCB + 1];
    __shared__ float st_s[64][2];
    __shared__ f32x4 red[4][24][NCB];
    const int c = blockIdx.x, g = blockIdx.y, t = threadIdx.x, slot = t / 24, f = t - slot * 24;
    const int F = a.S * 96, NC = a.NC;
    const int rbeg = g * a.RC, rend = min(a.R, rbeg + a.RC);
    f32x4 acc[NCB];
#pragma unroll
    for (int k = 0; k < NCB; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    float dbs = 0.f;   // thread t < NC of the c == 0 workgroup: sum of dl[k = t] over the chunk
    for (int r0 = rbeg; r0 < rend; r0 += 64) {
        const int nr = min(64, rend - r0);
        __syncthreads();
        for (int e = t; e < nr * NC; e += 192) {
            const int rr = e / NC, k = e - rr * NC, row = r0 + rr;
            const int b = row / a.N, n = row - b * a.N;
            dl_s[rr][k] = a.dlogits[((long)b * NC + k) * a.N + n];
        }
        for (int e = t; e < nr * 2; e += 192) st_s[e >> 1][e & 1] = a.stats[2L * r0 + e];
        __syncthreads();
        if (c == 0 && t < NC)
            for (int rr = 0; rr < nr; ++rr) dbs += dl_s[rr][t];
        for (int rr = slot; rr < nr; rr += 8) {
            const int row = r0 + rr, b = row / a.N, n = row - b * a.N;
            const f32x4 y4 = *reinterpret_cast<const f32x4*>(a.y + ((long)b * a.T + (long)c * a.N + n) * 96 + 4 * f);
            const f32x4 xh = (y4 - st_s[rr][0]) * st_s[rr][1];
#pragma unroll
            for (int k = 0; k < NCB; ++k)
                if (k < NC) acc[k] += dl_s[rr][k] * xh;
        }
    }
    // the 8 slots' partials in a fixed tree order: (s, s + 4), then (s, s + 2), then (0, 1)
#pragma unroll
    for (int half = 4; half >= 1; half >>= 1) {
        __syncthreads();
        if (slot >= half && slot < 2 * half)
#pragma unroll
            for (int k = 0; k < NCB; ++k) red[slot - half][f][k] = acc[k];
        __syncthreads();
        if (slot < half)
#pragma unroll
            for (int k = 0; k < NCB; ++k) acc[k] += red[slot][f][k];
    }
    float* slab = a.slab + (long)g * a.slab_stride;
    if (slot == 0)
#pragma unroll
        for (int k = 0; k < NCB; ++k)
            if (k < NC) *reinterpret_cast<f32x4*>(slab + (long)k * F + c * 96 + 4 * f) = acc[k];
    if (c == 0 && t < NC) slab[(long)NC * F + t] = dbs;
}

// grid (ceil(F / 256)), 256 threads: one feature j per thread
__global__ __launch_bounds__(256) void spec_head_wgrad_finish_kernel(SpecHeadArgs a, const float* A, const float* db, float* dw,
                                                                     float* dg, float* dbeta) {
    const int F = a.S * 96, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= F) return;
    const float gj = a.ln_g[j], bj = a.ln_b[j];
    float s1 = 0.f, s2 = 0.f;
    for (int k = 0; k < a.NC; ++k) {
        const float av = A[(long)k * F + j], dk = db[k], wk = a.w[(long)k * F + j];
        dw[(long)k * F + j] = gj * av + bj * dk;
        s1 += wk * av;
        s2 += wk * dk;
    }
    dg[j] = s1;
    dbeta[j] = s2;
}

// ------------------------------------------------------------------------------------------ host side
// static row partition of the weight-gradient pass: G chunks of RC consecutive rows (a function of R = B N only)
void spec_head_chunks(long R, int& G, int& RC) {
    G = (int)(R < 1 ? 1 : (R + 31) / 32 < 128 ? (R + 31) / 32 : 128);
    RC = (int)((R + G - 1) / G);
}

long spec_head_bwd_slab_floats(int B, int S, int N, int NC) {
    const long R = (long)B * N, F = 96L * S;
    int G, RC;
    spec_head_chunks(R, G, RC);
    const long stats = (2 * R + 3) / 4 * 4;
    const long stride = NC * F + 32;
    return stats + G * stride + NC * F;
}

static bool spec_head_shape_ok(const SpecHeadArgs& a) {
    return a.B >= 1 && a.S >= 1 && a.S <= 64 && a.N >= 1 && a.N <= 64 && a.NC >= 1 && a.NC <= 32;
}

// NQ = float4 pieces per lane (24 S / 64, rounded up to a bucket); each launcher picks its rows per wave RPW from it
template <template <int> class Launch>
static int dispatch_rows(const SpecHeadArgs& a, hipStream_t st) {
    if (a.S <= 5) return Launch<2>::go(a, st);
    if (a.S <= 10) return Launch<4>::go(a, st);
    if (a.S <= 21) return Launch<8>::go(a, st);
    if (a.S <= 42) return Launch<16>::go(a, st);
    return Launch<24>::go(a, st);
}

// registers per lane: RPW NQ 4 floats for the rows (forward), twice that (xhat and dxn) in the backward
template <int NQ>
struct FwdLaunch {
    static constexpr int RPW = NQ <= 8 ? 4 : NQ <= 16 ? 2 : 1;
    static int go(const SpecHeadArgs& a, hipStream_t st) {
        hipLaunchKernelGGL((spec_head_fwd_kernel<NQ, RPW>), dim3((a.R + 4 * RPW - 1) / (4 * RPW)), dim3(256), 0, st, a);
        return (int)hipGetLastError();
    }
};
template <int NQ>
struct BwdLaunch {
    static constexpr int RPW = NQ <= 4 ? 4 : NQ <= 8 ? 2 : 1;
    static int go(const SpecHeadArgs& a, hipStream_t st) {
        const dim3 grid((a.R + 4 * RPW - 1) / (4 * RPW));
        if (a.dy) hipLaunchKernelGGL((spec_head_bwd_rows_kernel<NQ, RPW, true>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((spec_head_bwd_rows_kernel<NQ, RPW, false>), grid, dim3(256), 0, st, a);
        return (int)hipGetLastError();
    }
};

int launch_spec_head_fwd(const SpecHeadArgs& a, hipStream_t st) {
    if (!spec_head_shape_ok(a)) return MSST_ERR_UNSUPPORTED;
    return dispatch_rows<FwdLaunch>(a, st);
}

int launch_spec_head_bwd_rows(const SpecHeadArgs& a, hipStream_t st) {
    if (!spec_head_shape_ok(a)) return MSST_ERR_UNSUPPORTED;
    return dispatch_rows<BwdLaunch>(a, st);
}

int launch_spec_head_wgrad(const SpecHeadArgs& a, hipStream_t st) {
    if (!spec_head_shape_ok(a)) return MSST_ERR_UNSUPPORTED;
    const dim3 grid(a.S, a.G);
    if (a.NC <= 8) hipLaunchKernelGGL(spec_head_wgrad_kernel<8>, grid, dim3(192), 0, st, a);
    else if (a.NC <= 16) hipLaunchKernelGGL(spec_head_wgrad_kernel<16>, grid, dim3(192), 0, st, a);
    else hipLaunchKernelGGL(spec_head_wgrad_kernel<32>, grid, dim3(192), 0, st, a);
    return (int)hipGetLastError();
}

int launch_spec_head_wgrad_finish(const SpecHeadArgs& a, const float* A, const float* db, float* dw, float* dg, float* dbeta,
                                  hipStream_t st) {
    hipLaunchKernelGGL(spec_head_wgrad_finish_kernel, dim3((a.S * 96 + 255) / 256), dim3(256), 0, st, a, A, db, dw, dg, dbeta);
    return (int)hipGetLastError();
}

}  // namespace msst
