// Input gradient of the MaskedSST tokenizer for gfx950: d(loss)/d(img) from dx0, the gradient at the tokenizer's output
// (what torch autograd hands the reference for free when img.requires_grad).
//
//   tokenize_bwd_input   recompute of tokenize_fwd (pre-norm LN over the P pixels, W_c xn + b_c, post-norm LN over 96), the
//                        embedding dropout undone on dx0, post-norm LN backward, dxn = W_c^T de, pre-norm LN backward, store
//   head_bwd_target      the SimMIM L1 loss's direct dependence on the input (its target is the raw pixels of the masked patches),
//                        gathered through the inverse CSR of head_bwd
//   scene_border_zero    the pixels of a tile batch that belong to no window
//   scene_fold_at        per-window input gradients of windows at listed origins, which overlap -> d(loss)/d(scene): every pixel sums
//                        the windows covering it in a fixed order, found through an inverse index over origin cells
//
// tokenize_bwd_kernel (msst_bwd.hip) computes the same dxn on its way to the pre-norm weight gradient, but it is organised for the
// cross-sample weight reductions: grid (S, nchunk), serial over its samples, at the 256-register limit.  Nothing is reduced over
// samples here, so this kernel is one workgroup per (sample, spectral block), launched only when somebody asks for img.grad.
// fp32 throughout, no atomics: equal inputs give equal bits.
#include "msst_dev.h"
#include "msst_kernels.h"

namespace msst {

// KC: ceil(P / 4), the 16-byte pieces of a weight row.  The [96][P] weight lies in LDS with rows of 20 floats, zero beyond P: a
// thread reads a row as KC ds_read_b128 (tokenize_bwd_kernel: P ds_read_b32 per row and use, which is what bound it), the four
// threads of a token read rows 4 apart = 80 floats = banks 16 apart, the 16 tokens of a wave the same addresses (broadcast).
// thread <-> (token n = tid / 4, features 16 (i / 4) + 4 part + i % 4, i < 24): the mapping of tokenize_fwd_kernel / tokenize_bwd_kernel,
// so a dropout group (four consecutive features) is one thread's f32x4 and has their element address.
// KIND: where sample b's pixels lie (WinRef, msst_kernels.h) and so the place of its gradient.  WIN_BATCH: dimg of the batch's shape.
// WIN_GRID: stored in place, to the window's pixels of dscene (stride == window: every pixel in at most one window, plain stores), no
// mask, no dtarget.  WIN_LISTED: stored stacked as for a batch -- dwin [B][S*P][N], plain stores; listed windows overlap,
// scene_fold_at_kernel below sums them; no mask, no dtarget.
template <int KC, int KIND>
__global__ __launch_bounds__(256) void tokenize_bwd_input_kernel(TokInArgs a) {
    constexpr int KP = 4 * KC;
    __shared__ float patch[16][64];
    __shared__ float outp[16][64];
    __shared__ __attribute__((aligned(16))) float W[96][20];
    __shared__ float bias[96], postg[96], preg[16], preb[16];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / a.S, c = blockIdx.x - b * a.S;
    const int P = a.P, N = a.N, T = a.T;
    for (int i = tid; i < 96 * 20; i += 256) {
        const int d = i / 20, k = i - d * 20;
        W[d][k] = k < P ? a.w_emb[((long)c * 96 + d) * P + k] : 0.f;
    }
    if (tid < 96) { bias[tid] = a.b_emb[c * 96 + tid]; postg[tid] = a.post_g[tid]; }
    if (tid < 16) { preg[tid] = tid < P ? a.pre_g[tid] : 0.f; preb[tid] = tid < P ? a.pre_b[tid] : 0.f; }
    const auto plane = win_plane<KIND>(a.src, N);
    const float* src = win_origin<KIND>(a.src.base, a.src, b, c, a.S, P, N);
    if constexpr (KIND == WIN_BATCH) {   // a cube's tile is P * N contiguous floats
        for (int i = tid; i < P * N; i += 256) patch[i / N][i % N] = src[i];
    } else {
        for (int i = tid; i < P * N; i += 256) {
            const int k = i / N, nn = i - k * N;
            patch[k][nn] = src[k * plane + win_pixel<KIND>(a.src, b, nn)];
        }
    }
    __syncthreads();
    const int n = tid >> 2, part = tid & 3;
    if (n < N) {
        const int t = c * N + n;
        const bool masked = a.mask ? a.mask[(long)b * T + t] != 0 : false;
        if (masked) {
            // a masked token's output is the mask token: it does not depend on its pixels
#pragma unroll
            for (int k = 0; k < KP; ++k) if ((k & 3) == part) outp[k][n] = 0.f;
        } else {
            f32x4 drow[6];
            const float* dsrc = a.dx0 + ((long)b * T + t) * 96 + part * 4;
#pragma unroll
            for (int i = 0; i < 6; ++i) drow[i] = *reinterpret_cast<const f32x4*>(dsrc + 16 * i);
            // ---- recompute of the forward
            float xh[KP], xn[KP];
            float mean = 0.f;
#pragma unroll
            for (int k = 0; k < KP; ++k) { xh[k] = k < P ? patch[k][n] : 0.f; mean += xh[k]; }
            mean /= P;
            float var = 0.f;
#pragma unroll
            for (int k = 0; k < KP; ++k) { const float d = k < P ? xh[k] - mean : 0.f; xh[k] = d; var += d * d; }
            const float rstd = rsqrtf(var / P + 1e-5f);
#pragma unroll
            for (int k = 0; k < KP; ++k) { xh[k] *= rstd; xn[k] = xh[k] * preg[k] + preb[k]; }   // k >= P: preg = preb = 0
            float e[24];
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < 24; ++i) {
                const int d = 16 * (i >> 2) + 4 * part + (i & 3);
                float acc = bias[d];
#pragma unroll
                for (int q = 0; q < KC; ++q) {
                    const f32x4 w4 = *reinterpret_cast<const f32x4*>(&W[d][4 * q]);
                    acc += w4[0] * xn[4 * q] + w4[1] * xn[4 * q + 1] + w4[2] * xn[4 * q + 2] + w4[3] * xn[4 * q + 3];
                }
                e[i] = acc;
                s += acc;
            }
            s += __shfl_xor(s, 1); s += __shfl_xor(s, 2);
            const float m2 = s * (1.f / 96.f);
            float v2 = 0.f;
#pragma unroll
            for (int i = 0; i < 24; ++i) { const float d = e[i] - m2; v2 += d * d; }
            v2 += __shfl_xor(v2, 1); v2 += __shfl_xor(v2, 2);
            const float rstd2 = rsqrtf(v2 * (1.f / 96.f) + 1e-5f);
            // ---- dx0 with the embedding dropout undone (element addressing of tokenize_bwd_kernel), post-norm LN backward
            float dt[24];
            float g1 = 0.f, g2 = 0.f;
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                f32x4 t4 = drow[i];
                if (a.drop.thr) t4 = drop4(a.drop, 0, (unsigned)(((long)b * T + t) * 24 + 4 * i + part), t4);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int ii = 4 * i + j;
                    const float eh = (e[ii] - m2) * rstd2;
                    e[ii] = eh;
                    dt[ii] = t4[j] * postg[16 * i + 4 * part + j];
                    g1 += dt[ii];
                    g2 += dt[ii] * eh;
                }
            }
            g1 += __shfl_xor(g1, 1); g1 += __shfl_xor(g1, 2);
            g2 += __shfl_xor(g2, 1); g2 += __shfl_xor(g2, 2);
            g1 *= (1.f / 96.f); g2 *= (1.f / 96.f);
            // ---- dxn = W_c^T de
            float dxn[KP];
#pragma unroll
            for (int k = 0; k < KP; ++k) dxn[k] = 0.f;
#pragma unroll
            for (int i = 0; i < 24; ++i) {
                const int d = 16 * (i >> 2) + 4 * part + (i & 3);
                const float de = rstd2 * (dt[i] - g1 - e[i] * g2);
#pragma unroll
                for (int q = 0; q < KC; ++q) {
                    const f32x4 w4 = *reinterpret_cast<const f32x4*>(&W[d][4 * q]);
                    dxn[4 * q] += w4[0] * de; dxn[4 * q + 1] += w4[1] * de; dxn[4 * q + 2] += w4[2] * de; dxn[4 * q + 3] += w4[3] * de;
                }
            }
            // ---- pre-norm LN backward; every thread of the token holds the sums, thread `part` stores pixels k = part mod 4
            float h1 = 0.f, h2 = 0.f;
#pragma unroll
            for (int k = 0; k < KP; ++k) {
                float v = dxn[k];
                v += __shfl_xor(v, 1); v += __shfl_xor(v, 2);
                v *= preg[k];
                dxn[k] = v;
                h1 += v;
                h2 += v * xh[k];
            }
            h1 /= P; h2 /= P;
#pragma unroll
            for (int k = 0; k < KP; ++k) if ((k & 3) == part) outp[k][n] = rstd * (dxn[k] - h1 - xh[k] * h2);
        }
    }
    __syncthreads();
    if constexpr (KIND == WIN_GRID) {   // in place
        float* dst = win_origin<KIND>(a.dimg, a.src, b, c, a.S, P, N);
        for (int i = tid; i < P * N; i += 256) {
            const int k = i / N, nn = i - k * N;
            dst[k * plane + win_pixel<KIND>(a.src, b, nn)] = outp[k][nn];
        }
    } else {   // stacked
        float* dst = win_origin<WIN_BATCH>(a.dimg, a.src, b, c, a.S, P, N);
        const long org = dst - a.dimg;
        for (int i = tid; i < P * N; i += 256) {
            float v = outp[i / N][i % N];
            if (a.dtarget) v += a.dtarget[org + i];
            dst[i] = v;
        }
    }
}

// dtarget[b][c P + p][n] = -gs sum_{e in CSR list of token (c, n) of row b} dpred[b][csr_pos[e]][p]: a gather with a sum in CSR
// order (head_bwd_kernel's gsh, negated: the target enters the loss as pred - target).  A row's index list may name a token more
// than once; tokens no index names get 0.  One workgroup per (sample, spectral block).
__global__ __launch_bounds__(256) void head_bwd_target_kernel(const float* dpred, const int* csr_ptr, const int* csr_pos, const float* gout,
                                                              float gscale, float* dtarget, int S, int N, int P, int K) {
    const int b = blockIdx.x / S, c = blockIdx.x - b * S;
    const int T = S * N;
    const float gs = gout ? gscale * gout[0] : gscale;
    float* dst = dtarget + ((long)b * S + c) * P * N;
    for (int i = threadIdx.x; i < P * N; i += 256) {
        const int p = i / N, n = i - p * N;
        const int t = c * N + n;
        const int e0 = csr_ptr[(long)b * (T + 1) + t], e1 = csr_ptr[(long)b * (T + 1) + t + 1];
        float s = 0.f;
        for (int e = e0; e < e1; ++e) s += dpred[((long)b * K + csr_pos[(long)b * K + e]) * P + p];
        dst[i] = -(s * gs);
    }
}

// zero for the pixels of dscene [Bs][C][Hs][Ws] beyond the window grid: rows >= rows_in or columns >= cols_in.  One thread per
// (plane row, column); the pixels inside the grid are not touched (the windows' workgroups store them).
__global__ __launch_bounds__(256) void scene_border_zero_kernel(float* dscene, long rows, int Hs, int Ws, int rows_in, int cols_in) {
    const long total = rows * Ws;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long row = i / Ws;
        const int x = (int)(i - row * Ws), y = (int)(row % Hs);
        if (y >= rows_in || x >= cols_in) dscene[i] = 0.f;
    }
}

// dscene [Bs][C][Hs][Ws] (+)= the per-window planes dwin [nwin][C][win * win] of windows at listed origins, summed per pixel over the
// windows covering it.  The windows are found through an inverse index over origin cells (maskedsst_amd.scene.origins_csr): the cell of a
// window is (scene * Hs + y0) * Ws + x0, cell_ptr [Bs Hs Ws + 1] the CSR row pointers, cell_win [nwin] the window numbers sorted by
// cell, ascending within a cell.  Pixel (s, y, x) is covered by the windows whose origin lies in the rectangle y0 in [max(0, y - win + 1),
// min(y, Hs - win)] x x0 likewise: it walks the rows y0 ascending, in a row the cells x0 ascending (consecutive cells: one more pointer
// read per cell), in a cell its list in order -- ascending (y0, x0, window number), a fixed order without atomics, so equal inputs give
// equal bits and a table that lists a regular grid in grid order may be split into consecutive calls (accumulate).
// The shape of scene_fold_kernel (msst_fwd.hip): grid (256-pixel pieces of the flattened scenes, channel group), one thread per (pixel,
// group), lanes along x -- the lanes of a wave that sit in the same window read consecutive floats of one of its rows and all lanes
// read / write consecutive floats of dscene; the group's channels are independent sums in 16 registers; no LDS.
// accumulate == 0: the sum starts from 0 and every pixel is written (0 where no window covers it).  Otherwise it starts from the value
// in dscene, and a pixel no window of this call covers is not touched.  An entry outside [0, nwin) is skipped.
__global__ __launch_bounds__(256) void scene_fold_at_kernel(SceneFoldAtArgs a) {
    const long plane = (long)a.Hs * a.Ws;
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= (long)a.Bs * plane) return;
    const int c0 = blockIdx.y * a.group, cn = min(a.group, a.C - c0);
    const long s = p / plane;
    const int pix = (int)(p - s * plane);
    const int y = pix / a.Ws, x = pix - y * a.Ws;
    const int ylo = max(0, y - a.win + 1), yhi = min(y, a.Hs - a.win);
    const int xlo = max(0, x - a.win + 1), xhi = min(x, a.Ws - a.win);
    const int N = a.win * a.win;
    float* out = a.dscene + (s * a.C + c0) * plane + pix;
    float acc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] = (k < cn && a.accumulate) ? out[k * plane] : 0.f;
    bool any = false;
    for (int y0 = ylo; y0 <= yhi; ++y0) {
        const int32_t* row = a.cell_ptr + (s * a.Hs + y0) * a.Ws;
        int e0 = xlo <= xhi ? max(row[xlo], 0) : 0;
        for (int x0 = xlo; x0 <= xhi; ++x0) {
            const int e1 = min(row[x0 + 1], a.nwin);
            const int off = (y - y0) * a.win + (x - x0);
            for (int e = e0; e < e1; ++e) {
                const int i = a.cell_win[e];
                if ((unsigned)i >= (unsigned)a.nwin) continue;
                const float* w = a.dwin + ((long)i * a.C + c0) * N + off;
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    if (k < cn) acc[k] += w[k * N];
                any = true;
            }
            e0 = max(e1, e0);
        }
    }
    if (!any && a.accumulate) return;
#pragma unroll
    for (int k = 0; k < 16; ++k)
        if (k < cn) out[k * plane] = acc[k];
}

// one launcher for the three sources (windows of a scene, numbered or listed: an empty call is no launch); KC = ceil(P / 4)
template <int KIND>
static int launch_tokenize_bwd_input_src(const TokInArgs& a, hipStream_t st) {
    if (a.P > 16 || a.N > 64 || (long)a.B * a.S > 0x7fffffffL) return MSST_ERR_UNSUPPORTED;
    if (KIND != WIN_BATCH && a.B < 1) return 0;
    ProfScope ps(K_TOK_BWD_INPUT, st);
    const dim3 grid((unsigned)((long)a.B * a.S));
    switch ((a.P + 3) / 4) {
    case 1: hipLaunchKernelGGL((tokenize_bwd_input_kernel<1, KIND>), grid, dim3(256), 0, st, a); break;
    case 2: hipLaunchKernelGGL((tokenize_bwd_input_kernel<2, KIND>), grid, dim3(256), 0, st, a); break;
    case 3: hipLaunchKernelGGL((tokenize_bwd_input_kernel<3, KIND>), grid, dim3(256), 0, st, a); break;
    default: hipLaunchKernelGGL((tokenize_bwd_input_kernel<4, KIND>), grid, dim3(256), 0, st, a); break;
    }
    return (int)hipGetLastError();
}
int launch_tokenize_bwd_input(const TokInArgs& a, int kind, hipStream_t st) {
    switch (kind) {
    case WIN_BATCH: return launch_tokenize_bwd_input_src<WIN_BATCH>(a, st);
    case WIN_GRID: return launch_tokenize_bwd_input_src<WIN_GRID>(a, st);
    case WIN_LISTED: return launch_tokenize_bwd_input_src<WIN_LISTED>(a, st);
    }
    return MSST_ERR_UNSUPPORTED;   // oriented input gradients: no instance
}

int launch_scene_fold_at(const SceneFoldAtArgs& a, hipStream_t st) {
    const long pixels = (long)a.Bs * a.Hs * a.Ws;
    const long grid = (pixels + 255) / 256, ny = ((long)a.C + a.group - 1) / a.group;
    if (a.group > 16 || a.win * a.win > 64 || grid > 0x7fffffffL || ny > 65535) return MSST_ERR_UNSUPPORTED;
    ProfScope ps(K_TOK_BWD_INPUT, st);
    hipLaunchKernelGGL(scene_fold_at_kernel, dim3((unsigned)grid, (unsigned)ny), dim3(256), 0, st, a);
    return (int)hipGetLastError();
}

int launch_scene_border_zero(float* dscene, long rows, int Hs, int Ws, int rows_in, int cols_in, hipStream_t st) {
    if (rows_in >= Hs && cols_in >= Ws) return 0;
    const long total = rows * Ws;
    long grid = (total + 255) / 256;
    if (grid > 4096) grid = 4096;
    ProfScope ps(K_TOK_BWD_INPUT, st);
    hipLaunchKernelGGL(scene_border_zero_kernel, dim3((unsigned)grid), dim3(256), 0, st, dscene, rows, Hs, Ws, rows_in, cols_in);
    return (int)hipGetLastError();
}

int launch_head_bwd_target(const float* dpred, const int* csr_ptr, const int* csr_pos, const float* gout, float gscale, float* dtarget,
                           int B, int S, int N, int P, int K, hipStream_t st) {
    ProfScope ps(K_HEAD_BWD_TARGET, st);
    hipLaunchKernelGGL(head_bwd_target_kernel, dim3((unsigned)((long)B * S)), dim3(256), 0, st, dpred, csr_ptr, csr_pos, gout, gscale,
                       dtarget, S, N, P, K);
    return (int)hipGetLastError();
}

}  // namespace msst
