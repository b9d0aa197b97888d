// Whole-scene embedding maps (ViTSpatialSpectral.encode_scene): the tail behind the encoder.  Encoder output of windows of a scene
// y [nwin][S N][96] -> per-window features [nwin][96][N] (msst_pool_spectral_fwd: mean over the S spectral tokens of a position, the
// quantity the default head normalises) -> scene maps feat [Bs][96][Hs][Ws] = mean over the windows covering a pixel, optionally
// divided by its L2 norm, NaN where no window covers the pixel, and the cover map (msst_scene_embed_assemble).
//
// pool_spectral   one workgroup per window, 256 threads.  A window's S slabs of N rows x 96 floats are read once as 16-byte pieces,
//             piece i = (row n = i / 24, floats 4 (i % 24) ..) <-> thread i % 256: a wave reads 1 KiB of consecutive bytes per
//             load.  Each thread adds the S pieces of its (n, d4) in the order c = 0 .. S - 1, divides by (float)S and puts the four
//             values into the LDS tile [n][d] (pitch 97 floats); after one barrier thread o % 256 reads (d = o / N, n = o % N) and
//             stores out[b][d][n]: the window's 96 N outputs are consecutive floats, so every wave stores 256 consecutive bytes.
//             LDS banks (32 banks of 4 bytes for one-dword reads and writes, conflicts per 32-lane half): the transposed read has
//             bank (97 n + d) % 32 = (n + d) % 32, all different over 32 consecutive n.  The write of component j of piece d4 has
//             bank (n + 4 d4 + j) % 32: 4 d4 % 32 takes 8 values over the 24 pieces of a row, three pieces per value, whatever the
//             pitch; so the lanes write component (j + d4 / 8) % 4 in step j, which gives the three pieces of a value three
//             different banks: no conflict inside a row, two lanes on a bank at most where a half-wave spans two rows.
// scene_embed_finalize   the running sums are the shared fold's (scene_fold_kernel, msst_fwd.hip; launch_scene_fold with C = D, 16
//             planes per grid row: any split into calls gives the same bits).  Finalize: one thread per pixel, lanes along x;
//             sum / k written back plane by plane while the squares are added in the order d = 0 .. D - 1, then (l2norm) a
//             second pass over the planes it has just written divides by max(sqrt(sum of squares), 1e-12) -- F.normalize.
// Memory-bound VALU work: no MFMA, no inline assembly.
#include "msst_dev.h"
#include "msst_kernels.h"

namespace msst {

namespace {

constexpr int POOL_PITCH = 97;   // floats per LDS row [n][0 .. 95]: odd, so that the transposed read walks the banks

__global__ __launch_bounds__(256) void pool_spectral_kernel(const float* __restrict__ y, float* __restrict__ out, int S, int N) {
    __shared__ float tile[64 * POOL_PITCH];
    const int tid = threadIdx.x;
    const long b = blockIdx.x;
    const int pieces = N * 24;                                  // 16-byte pieces of one spectral slab [N][96]
    const float4* src = reinterpret_cast<const float4*>(y) + b * S * pieces;
    const float fS = (float)S;
    for (int i = tid; i < pieces; i += 256) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int c = 0; c < S; ++c) {
            const float4 v = src[(long)c * pieces + i];
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
        acc.x /= fS; acc.y /= fS; acc.z /= fS; acc.w /= fS;
        const int n = i / 24, d4 = i - n * 24, rot = d4 >> 3;
        float* row = tile + n * POOL_PITCH + 4 * d4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int jj = (j + rot) & 3;
            row[jj] = jj == 0 ? acc.x : jj == 1 ? acc.y : jj == 2 ? acc.z : acc.w;
        }
    }
    __syncthreads();
    float* dst = out + b * 96 * N;
    for (int o = tid; o < 96 * N; o += 256) {
        const int d = o / N, n = o - d * N;
        dst[o] = tile[n * POOL_PITCH + d];
    }
}

__global__ __launch_bounds__(256) void scene_embed_finalize_kernel(SceneEmbedArgs a) {
    const long plane = (long)a.Hs * a.Ws;
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= (long)a.Bs * plane) return;
    const long s = p / plane, pix = p - s * plane;
    const int y = (int)(pix / a.Ws), x = (int)(pix - (long)y * a.Ws);
    float* out = a.feat + s * a.D * plane + pix;
    int rlo, rhi, qlo, qhi;
    const int k = scene_cover(a, y, x, rlo, rhi, qlo, qhi) ? (rhi - rlo + 1) * (qhi - qlo + 1) : 0;
    a.cover[p] = k;
    if (k == 0) {   // no window here: absent, not a made-up number
        const float nan = __builtin_nanf("");
        for (int d = 0; d < a.D; ++d) out[d * plane] = nan;
        return;
    }
    const float cnt = (float)k;
    float ss = 0.f;
    for (int d = 0; d < a.D; ++d) {
        const float v = out[d * plane] / cnt;
        out[d * plane] = v;
        ss += v * v;
    }
    if (!a.l2norm) return;
    const float nrm = fmaxf(sqrtf(ss), 1e-12f);
    for (int d = 0; d < a.D; ++d) out[d * plane] = out[d * plane] / nrm;   // the thread's own stores: visible to it in program order
}

}  // namespace

int launch_pool_spectral(const float* y, float* out, int B, int S, int N, hipStream_t st) {
    if (N > 64 || S > 64) return MSST_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(pool_spectral_kernel, dim3((unsigned)B), dim3(256), 0, st, y, out, S, N);
    return (int)hipGetLastError();
}

int launch_scene_embed_finalize(const SceneEmbedArgs& a, hipStream_t st) {
    const long grid = ((long)a.Bs * a.Hs * a.Ws + 255) / 256;
    if (grid > 0x7fffffffL) return MSST_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(scene_embed_finalize_kernel, dim3((unsigned)grid), dim3(256), 0, st, a);
    return (int)hipGetLastError();
}

}  // namespace msst
