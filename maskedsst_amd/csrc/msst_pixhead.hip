// Pixelwise centre-pixel classification head (reference vit_spatial_spectral.py:466-478 and :536-564 with pixelwise=True):
// 'b (c h w) d -> b c h w d', mean over c, LayerNorm(96) per position, Flatten (feature j = n 96 + d, n = h W + w),
// Linear(96 N -> n_classes) -> logits [B][n_classes] (one class vector per window, for its centre pixel).  fp32, VALU.
//
// Forward, two launches:
//   pix_head_norm:    rows (b, n): mean over the S tokens, two-pass LayerNorm statistics, eps 1e-5 -> xn [B][96 N] (workspace).
//                     This is the pass that reads y (B S N 384 bytes, the byte floor); xn is 1/S of that.
//   pix_head_logits:  logits = xn W^T + b, a [B, 96 N] x [96 N, nc] product.  A workgroup owns SPB = 128 / NCB samples and every
//                     class, so each W float4 it loads serves SPB samples: W is read B / SPB times in all (through L2), not B times.
//                     The K loop leaves 128 partial dot products per lane; they are summed by recursive halving across the wave and
//                     then over the four waves in a fixed order.
// Backward (given dl [B][nc]), one launch plus the shared fixed-order reduction:
//   pix_head_bwd:     workgroup (n, g) = position n of the 32 samples of group g (a static partition of B: G = ceil(B / 32)).
//                     It stages W[:, n 96 .. n 96 + 95] and dl of its samples in LDS, recomputes the row statistics, forms
//                     dxn = W^T dl for its slice, the LayerNorm backward, and writes dy[b, c, n, :] = dx / S for every c (fully
//                     written).  Then it writes the partials of its 32 samples: dW[:, n slice] and db (n == 0) into slab g,
//                     dgamma / dbeta into partial row (g, n).  With a null dy (a frozen body: nobody consumes it) the variant compiled
//                     without the LayerNorm backward and the dy stores runs; everything that feeds the four head gradients is
//                     the same arithmetic in the same order (bit-identical results).
//   launch_reduce_segs: the G slabs -> dW, db, and the G N partial rows -> dgamma, dbeta (fixed slab order).
// No float atomics: the gradients are bitwise reproducible run to run and independent of the CU count.
//
// Scene centre assembly (msst_scene_centre_assemble): window logits [nwin][nc] go to the centre pixel (y0 + w / 2, x0 + w / 2) of
// their window, with the argmax; each pixel is the centre of at most one window, so every write is owned by one thread.  The finish
// pass writes class -1 and logit 0 to the pixels that are no window's centre.
#include "msst_dev.h"
#include "msst_kernels.h"

namespace msst {

namespace {

constexpr int PIX_GROUP = 32;   // samples per workgroup of the row kernels (and the static partition of the backward)

__device__ __forceinline__ float sum8(float v) {
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    return v;   // the butterfly leaves the same bits on all 8 lanes of the row
}

// the four terms in one fixed order, as explicit fused multiply-adds.  Written as a0 b0 + a1 b1 + a2 b2 + a3 b3 the compiler packed
// the dot products of two neighbouring samples into one v_pk_fma_f32 chain and, to do so, commuted the first sum of the upper one
// (fma(a0, b0, a1 b1) beside fma(a1, b1, a0 b0)): the last bits of a sample's logits then depended on whether its index in the launch
// was even or odd.  This is the order one sample of every such pair always had.
__device__ __forceinline__ float dot4(f32x4 a, f32x4 b) { return fmaf(a[3], b[3], fmaf(a[2], b[2], fmaf(a[1], b[1], a[0] * b[0]))); }

// row (b, n): lane part (0..7) owns features 12 part .. 12 part + 11.  m <- the mean over the S tokens; (mean, rstd) of LayerNorm(96)
__device__ __forceinline__ void pix_row(const PixHeadArgs& a, int b, int n, int part, float (&m)[12], float& mean, float& rstd) {
#pragma unroll
    for (int i = 0; i < 12; ++i) m[i] = 0.f;
    const float* base = a.y + ((long)b * a.T + n) * 96 + part * 12;
    const long cstride = (long)a.N * 96;
#pragma unroll 4
    for (int c = 0; c < a.S; ++c) {
        const f32x4* src = reinterpret_cast<const f32x4*>(base + c * cstride);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const f32x4 t4 = src[i];
            m[4 * i] += t4[0]; m[4 * i + 1] += t4[1]; m[4 * i + 2] += t4[2]; m[4 * i + 3] += t4[3];
        }
    }
    const float invS = 1.f / a.S;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 12; ++i) { m[i] *= invS; s += m[i]; }
    mean = sum8(s) * (1.f / 96.f);
    float vs = 0.f;
#pragma unroll
    for (int i = 0; i < 12; ++i) { const float d = m[i] - mean; vs += d * d; }
    rstd = rsqrtf(sum8(vs) * (1.f / 96.f) + 1e-5f);
}

// one step of the recursive halving: lanes with bit m set keep the upper H values, the others the lower H, each adding its
// partner's copy of the half it keeps
template <int H>
__device__ __forceinline__ void halve(float (&v)[128], int lane, int m) {
    const bool up = (lane & m) != 0;
#pragma unroll
    for (int i = 0; i < H; ++i) {
        const float send = up ? v[i] : v[i + H];
        const float keep = up ? v[i + H] : v[i];
        v[i] = keep + __shfl_xor(send, m);
    }
}

}  // namespace

// grid (N, G), 256 threads = 32 rows (samples) x 8 lanes
__global__ __launch_bounds__(256) void pix_head_norm_kernel(PixHeadArgs a) {
    const int n = blockIdx.x, t = threadIdx.x, r = t >> 3, part = t & 7;
    const int b = blockIdx.y * PIX_GROUP + r;
    if (b >= a.B) return;   // (uniform over the 8 lanes of a row)
    float m[12], mean, rstd;
    pix_row(a, b, n, part, m, mean, rstd);
    f32x4* dst = reinterpret_cast<f32x4*>(a.xn + (long)b * a.N * 96 + n * 96 + part * 12);
    const f32x4* g4 = reinterpret_cast<const f32x4*>(a.ln_g + part * 12);
    const f32x4* b4 = reinterpret_cast<const f32x4*>(a.ln_b + part * 12);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const f32x4 x = f32x4{m[4 * i], m[4 * i + 1], m[4 * i + 2], m[4 * i + 3]};
        dst[i] = (x - mean) * rstd * g4[i] + b4[i];
    }
}

// grid (ceil(B / SPB)), 256 threads; SPB samples x NCB classes = 128 dot products per workgroup
template <int NCB>
__global__ __launch_bounds__(256) void pix_head_logits_kernel(PixHeadArgs a) {
    constexpr int SPB = 128 / NCB;
    __shared__ float red[4][128];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int b0 = blockIdx.x * SPB;
    const int K4 = a.N * 24;
    const long K = (long)a.N * 96;
    float acc[128];
#pragma unroll
    for (int i = 0; i < 128; ++i) acc[i] = 0.f;
    for (int q = t; q < K4; q += 256) {
        f32x4 x[SPB];
#pragma unroll
        for (int s = 0; s < SPB; ++s)
            x[s] = b0 + s < a.B ? *reinterpret_cast<const f32x4*>(a.xn + (long)(b0 + s) * K + 4 * q) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < NCB; ++k) {
            if (k < a.NC) {
                const f32x4 w4 = *reinterpret_cast<const f32x4*>(a.w + k * K + 4 * q);
#pragma unroll
                for (int s = 0; s < SPB; ++s) acc[s * NCB + k] += dot4(w4, x[s]);
            }
        }
    }
    halve<64>(acc, lane, 32);
    halve<32>(acc, lane, 16);
    halve<16>(acc, lane, 8);
    halve<8>(acc, lane, 4);
    halve<4>(acc, lane, 2);
    halve<2>(acc, lane, 1);
    // lane l now holds products 2 rev6(l) and 2 rev6(l) + 1 (rev6: the six lane bits reversed)
    const int off = ((lane >> 5) & 1) * 64 + ((lane >> 4) & 1) * 32 + ((lane >> 3) & 1) * 16 + ((lane >> 2) & 1) * 8 +
                    ((lane >> 1) & 1) * 4 + (lane & 1) * 2;
    red[wave][off] = acc[0];
    red[wave][off + 1] = acc[1];
    __syncthreads();
    if (t < 128) {
        const float v = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
        const int s = t / NCB, k = t - s * NCB, b = b0 + s;
        if (b < a.B && k < a.NC) a.logits[(long)b * a.NC + k] = v + a.b[k];
    }
}

// grid (N, G), 256 threads = 32 rows (samples) x 8 lanes.  Slab layout (floats): [G][NC][96 N] dW partials | [G][32] db partials |
// [G N][96] dgamma partials | [G N][96] dbeta partials
template <int NCB, bool WANT_DY>
__global__ __launch_bounds__(256) void pix_head_bwd_kernel(PixHeadArgs a) {
    __shared__ float w_s[NCB][96];
    __shared__ float dl_s[PIX_GROUP][NCB + 1];
    __shared__ float xn_s[PIX_GROUP][97];
    __shared__ float pg_s[PIX_GROUP][97];
    __shared__ float pb_s[PIX_GROUP][97];
    const int n = blockIdx.x, g = blockIdx.y, t = threadIdx.x, r = t >> 3, part = t & 7;
    const int NC = a.NC;
    const long K = (long)a.N * 96;
    for (int e = t; e < NCB * 96; e += 256) {
        const int k = e / 96, d = e - k * 96;
        w_s[k][d] = k < NC ? a.w[k * K + n * 96 + d] : 0.f;
    }
    for (int e = t; e < PIX_GROUP * NC; e += 256) {
        const int rr = e / NC, k = e - rr * NC, b = g * PIX_GROUP + rr;
        dl_s[rr][k] = b < a.B ? a.dlogits[(long)b * NC + k] : 0.f;
    }
    __syncthreads();
    const int b = g * PIX_GROUP + r;
    if (b < a.B) {   // (uniform over the 8 lanes of a row)
        float m[12], mean, rstd;
        pix_row(a, b, n, part, m, mean, rstd);
        float dxn[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) { m[i] = (m[i] - mean) * rstd; dxn[i] = 0.f; }   // m = xhat
        for (int k = 0; k < NC; ++k) {
            const float dl = dl_s[r][k];
#pragma unroll
            for (int i = 0; i < 12; ++i) dxn[i] += dl * w_s[k][part * 12 + i];
        }
        float g1 = 0.f, g2 = 0.f;
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            const int d = part * 12 + i;
            const float gam = a.ln_g[d];
            xn_s[r][d] = m[i] * gam + a.ln_b[d];
            pg_s[r][d] = dxn[i] * m[i];
            pb_s[r][d] = dxn[i];
            if constexpr (WANT_DY) {
                dxn[i] *= gam;
                g1 += dxn[i];
                g2 += dxn[i] * m[i];
            }
        }
        if constexpr (WANT_DY) {
            g1 = sum8(g1) * (1.f / 96.f);
            g2 = sum8(g2) * (1.f / 96.f);
            const float invS = 1.f / a.S;
            f32x4 o[3];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) o[i][e] = rstd * (dxn[4 * i + e] - g1 - m[4 * i + e] * g2) * invS;
            float* base = a.dy + ((long)b * a.T + n) * 96 + part * 12;
            const long cstride = (long)a.N * 96;
            for (int c = 0; c < a.S; ++c) {
                f32x4* dst = reinterpret_cast<f32x4*>(base + c * cstride);
#pragma unroll
                for (int i = 0; i < 3; ++i) dst[i] = o[i];
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            const int d = part * 12 + i;
            xn_s[r][d] = 0.f; pg_s[r][d] = 0.f; pb_s[r][d] = 0.f;
        }
    }
    __syncthreads();
    float* dw_p = a.slab + (long)g * NC * K;
    for (int e = t; e < NC * 96; e += 256) {
        const int k = e / 96, d = e - k * 96;
        float s = 0.f;
        for (int rr = 0; rr < PIX_GROUP; ++rr) s += dl_s[rr][k] * xn_s[rr][d];
        dw_p[k * K + n * 96 + d] = s;
    }
    float* db_p = a.slab + (long)a.G * NC * K;
    if (n == 0 && t < NC) {
        float s = 0.f;
        for (int rr = 0; rr < PIX_GROUP; ++rr) s += dl_s[rr][t];
        db_p[g * 32 + t] = s;
    }
    float* dg_p = db_p + (long)a.G * 32;
    float* dbeta_p = dg_p + (long)a.G * a.N * 96;
    if (t < 192) {
        const int d = t < 96 ? t : t - 96;
        float s = 0.f;
        if (t < 96)
            for (int rr = 0; rr < PIX_GROUP; ++rr) s += pg_s[rr][d];
        else
            for (int rr = 0; rr < PIX_GROUP; ++rr) s += pb_s[rr][d];
        (t < 96 ? dg_p : dbeta_p)[((long)g * a.N + n) * 96 + d] = s;
    }
}

// one thread per window of the call: its logits to the window's centre pixel, and their argmax (first maximum, NaN counts as the
// maximum: torch.argmax, as scene_finalize_kernel)
__global__ __launch_bounds__(256) void scene_centre_scatter_kernel(SceneArgs a) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.nwin) return;
    const long gw = a.win0 + i, wps = (long)a.nr * a.nq;
    const long s = gw / wps;
    const int rem = (int)(gw - s * wps), r = rem / a.nq, q = rem - r * a.nq;
    const int y = r * a.stride + a.win / 2, x = q * a.stride + a.win / 2;
    const long plane = (long)a.Hs * a.Ws, pix = (long)y * a.Ws + x;
    float* out = a.logits + s * a.NC * plane + pix;
    const float* src = a.win_logits + i * a.NC;
    float best = 0.f;
    int arg = 0;
    for (int k = 0; k < a.NC; ++k) {
        const float v = src[k];
        out[k * plane] = v;
        if (k == 0 || (best == best && (v > best || v != v))) { best = v; arg = k; }
    }
    a.classes[s * plane + pix] = arg;
}

// every pixel that is no window's centre: logits 0, class -1
__global__ __launch_bounds__(256) void scene_centre_fill_kernel(SceneArgs a) {
    const long plane = (long)a.Hs * a.Ws;
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= (long)a.Bs * plane) return;
    const long s = p / plane, pix = p - s * plane;
    const int y = (int)(pix / a.Ws) - a.win / 2, x = (int)(pix % a.Ws) - a.win / 2;
    const bool centre = y >= 0 && x >= 0 && y % a.stride == 0 && x % a.stride == 0 && y / a.stride < a.nr && x / a.stride < a.nq;
    if (centre) return;
    float* out = a.logits + s * a.NC * plane + pix;
    for (int k = 0; k < a.NC; ++k) out[k * plane] = 0.f;
    a.classes[p] = -1;
}

// ------------------------------------------------------------------------------------------ host side
int pix_head_groups(int B) { return (B + PIX_GROUP - 1) / PIX_GROUP; }

long pix_head_bwd_slab_floats(int B, int N, int NC) {
    const long G = pix_head_groups(B), K = 96L * N;
    return G * NC * K + G * 32 + 2 * G * N * 96;
}

int launch_pix_head_fwd(const PixHeadArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(pix_head_norm_kernel, dim3(a.N, a.G), dim3(256), 0, st, a);
    if (a.NC <= 8) hipLaunchKernelGGL(pix_head_logits_kernel<8>, dim3((a.B + 15) / 16), dim3(256), 0, st, a);
    else if (a.NC <= 16) hipLaunchKernelGGL(pix_head_logits_kernel<16>, dim3((a.B + 7) / 8), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(pix_head_logits_kernel<32>, dim3((a.B + 3) / 4), dim3(256), 0, st, a);
    return (int)hipGetLastError();
}

template <bool WANT_DY>
static void pix_head_bwd_go(const PixHeadArgs& a, hipStream_t st) {
    const dim3 grid(a.N, a.G);
    if (a.NC <= 8) hipLaunchKernelGGL((pix_head_bwd_kernel<8, WANT_DY>), grid, dim3(256), 0, st, a);
    else if (a.NC <= 16) hipLaunchKernelGGL((pix_head_bwd_kernel<16, WANT_DY>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((pix_head_bwd_kernel<32, WANT_DY>), grid, dim3(256), 0, st, a);
}

int launch_pix_head_bwd(const PixHeadArgs& a, hipStream_t st) {
    if (a.dy) pix_head_bwd_go<true>(a, st);
    else pix_head_bwd_go<false>(a, st);
    return (int)hipGetLastError();
}

int launch_scene_centre_scatter(const SceneArgs& a, hipStream_t st) {
    if (a.nwin < 1) return 0;
    hipLaunchKernelGGL(scene_centre_scatter_kernel, dim3((unsigned)((a.nwin + 255) / 256)), dim3(256), 0, st, a);
    return (int)hipGetLastError();
}

int launch_scene_centre_fill(const SceneArgs& a, hipStream_t st) {
    const long grid = ((long)a.Bs * a.Hs * a.Ws + 255) / 256;
    if (grid > 0x7fffffffL) return MSST_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(scene_centre_fill_kernel, dim3((unsigned)grid), dim3(256), 0, st, a);
    return (int)hipGetLastError();
}

}  // namespace msst
