// SimMIM reconstruction: to_pixels (reference vit_simmim_original.py:9-40, :328-332) over EVERY token of the encoder output, stored
// transposed into the cube layout, with the per-band absolute error over the masked pixels taken in the same pass.
//
//   y [B][T][96] (T = S N, token t = c N + n)  ->  recon [B][S P][N]:  recon[b][c P + k][n] = b_c[k] + sum_d W_c[k][d] y[b][c N + n][d]
//   blend: a token whose mask byte is 0 gets img's P values instead (the bits of img)
//   band_err [B][S P] (double) = sum over the MASKED n of |pred - img|,  band_cnt [B][S P] = how many n are masked (blend or not)
//
// recon_fwd   grid (S, chunks of samples), 256 threads = 4 waves.  A workgroup owns one spectral block c: W_c [P][96] and b_c are
//             staged in LDS once, then it walks its samples.  The N rows of a (sample, block) are one contiguous run of 96 N floats:
//             the workgroup reads it as 16-byte pieces (a wave instruction = 1 KiB of consecutive addresses) into registers -- the
//             NEXT sample's pieces are in flight while this one is computed -- and parks them in LDS, rows 100 floats apart (a
//             ds_read_b128 of lane n starts at bank 36 n mod 64: no two lanes of a 16-lane group on one bank).  Lane n of every wave
//             is position n; wave w computes bands k = w, w + 4, w + 8, w + 12 (< P): its W reads are one address per wave
//             (broadcast), its stores and its img reads are N consecutive floats of one band plane.  fp32, one fmaf chain per
//             output: bias, then d = 0 .. 95.
//             A band's N outputs sit in ONE wave, so its error sum is a butterfly over the wave's lanes (a fixed order) of doubles
//             -- |pred - img| is formed in double, exactly -- and its count a ballot.  No atomics, nothing to zero: every word of
//             recon, band_err and band_cnt is written, two calls give the same bits.
// The head is 96 P multiply-adds per token against the encoder's tens of thousands: VALU, no MFMA.
#include "msst_dev.h"
#include "msst_kernels.h"

namespace msst {

namespace {

constexpr int RECON_YS = 100;   // floats between the LDS rows of two positions (96 + one 16-byte slot)

__global__ __launch_bounds__(256) void recon_fwd_kernel(ReconArgs a) {
    __shared__ __attribute__((aligned(16))) float ys[64 * RECON_YS];
    __shared__ __attribute__((aligned(16))) float ws[16 * 96];
    __shared__ float bs[16];
    const int tid = threadIdx.x, w = tid >> 6, n = tid & 63;
    const int c = blockIdx.x, S = a.S, N = a.N, P = a.P;
    const int wc = a.per_block ? c : 0;
    for (int i = tid; i < P * 96; i += 256) ws[i] = a.w_pix[(long)wc * P * 96 + i];
    if (tid < P) bs[tid] = a.b_pix[wc * P + tid];
    const int npiece = N * 24;   // 16-byte pieces of the N rows of one (sample, block)
    f32x4 pre[6];
    auto fetch = [&](int b) {
        const f32x4* src = reinterpret_cast<const f32x4*>(a.y + ((long)b * S + c) * N * 96);
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const int i = tid + 256 * j;
            if (i < npiece) pre[j] = src[i];
        }
    };
    int b = blockIdx.y;
    if (b < a.B) fetch(b);
    for (; b < a.B; b += gridDim.y) {
        __syncthreads();   // the previous sample's rows have been read (first pass: nothing pending)
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const int i = tid + 256 * j;
            if (i < npiece) {
                const int r = i / 24, q = i - r * 24;
                *reinterpret_cast<f32x4*>(&ys[r * RECON_YS + 4 * q]) = pre[j];
            }
        }
        __syncthreads();   // rows (and, first pass, W_c and b_c) are in LDS
        if (b + (int)gridDim.y < a.B) fetch(b + gridDim.y);
        float acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = w + 4 * j < P ? bs[w + 4 * j] : 0.f;
        const f32x4* yr = reinterpret_cast<const f32x4*>(&ys[n * RECON_YS]);   // rows n >= N hold stale values: computed, never stored
#pragma unroll 4
        for (int d4 = 0; d4 < 24; ++d4) {
            const f32x4 yv = yr[d4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (w + 4 * j < P) {   // one answer per wave
                    const f32x4 wv = reinterpret_cast<const f32x4*>(&ws[(w + 4 * j) * 96])[d4];
                    acc[j] = fmaf(wv[0], yv[0], acc[j]);
                    acc[j] = fmaf(wv[1], yv[1], acc[j]);
                    acc[j] = fmaf(wv[2], yv[2], acc[j]);
                    acc[j] = fmaf(wv[3], yv[3], acc[j]);
                }
            }
        }
        const bool on = n < N;
        const bool masked = on && a.mask[((long)b * S + c) * N + n] != 0;
        const int cnt = __popcll(__ballot(masked));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = w + 4 * j;
            if (k >= P) continue;
            const long band = ((long)b * S + c) * P + k;
            double e = 0.0;
            if (on) {
                const float t = a.img[band * N + n];
                a.recon[band * N + n] = (a.blend && !masked) ? t : acc[j];
                if (masked) e = fabs((double)acc[j] - (double)t);
            }
            if (a.band_err) {
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o);
                if (n == 0) {
                    a.band_err[band] = e;
                    a.band_cnt[band] = cnt;
                }
            }
        }
    }
}

}  // namespace

int launch_recon_fwd(const ReconArgs& a, hipStream_t st) {
    if (a.N > 64 || a.P > 16) return MSST_ERR_UNSUPPORTED;
    // about four workgroups per CU in flight, each staging W_c once for its share of the samples
    int chunks = 1024 / a.S;
    if (chunks < 1) chunks = 1;
    if (chunks > a.B) chunks = a.B;
    ProfScope ps(K_RECON, st);
    hipLaunchKernelGGL(recon_fwd_kernel, dim3(a.S, chunks), dim3(256), 0, st, a);
    return (int)hipGetLastError();
}

}  // namespace msst
