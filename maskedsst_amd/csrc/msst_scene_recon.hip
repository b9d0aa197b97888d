// Whole-scene SimMIM reconstruction, the assembling end (msst_scene_recon_assemble): the counterpart of scene_accumulate / scene_finalize
// (msst_fwd.hip) for pixels.  Per-window predictions win_recon [nwin][S P][win * win] (msst_recon_fwd, blend = 0, of windows of a scene)
// -> the scene cube [Bs][S P][Hs][Ws] = mean of the predictions of every window covering a pixel, blended with the scene where the
// token is not masked, with the per-band |prediction - scene| sums over the masked covered pixels and the cover map.
//
// scene_recon_accumulate   grid (256-pixel pieces of the flattened (scene, pixel row) rows the call's windows reach, spectral block c),
//             one thread per (pixel, block): lanes run along x, so a wave reads runs of consecutive floats of a window row of
//             win_recon (one run per covering window column) and reads / writes consecutive floats of `cube`.  The P bands of the
//             block are P independent sums held in registers; each adds its windows in window order (row, then column): no atomics, a
//             fixed order, whatever the split into calls.  A pixel whose first covering window is in this call starts from 0 (nothing to
//             zero beforehand), one with no window in this call is not touched.
// scene_recon_finalize     one workgroup per (scene, band) plane, 256 threads, pixel i of the plane <-> thread i % 256 (lanes along x).
//             sum / k (k = windows covering the pixel), blend, NaN where nothing covers the pixel and nothing is blended.  The
//             plane's |prediction - scene| terms (formed in double: exact) are added in one fixed order: each thread its pixels
//             i = tid, tid + 256, ... in turn, a butterfly over the wave's lanes, the four waves in order 0 .. 3 by thread 0.  The
//             workgroups of band 0 also write the cover map.
// Memory-bound VALU work: no MFMA, no LDS beyond the four wave partials.
#include "msst_dev.h"
#include "msst_kernels.h"

namespace msst {

namespace {

__global__ __launch_bounds__(256) void scene_recon_accumulate_kernel(SceneReconArgs a, long pixels) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= pixels) return;
    const int c = blockIdx.y, P = a.P;
    const long R = a.row0 + p / a.Ws;
    const int x = (int)(p % a.Ws);
    const long s = R / a.Hs;
    const int y = (int)(R - s * a.Hs);
    int rlo, rhi, qlo, qhi;
    if (!scene_cover(a, y, x, rlo, rhi, qlo, qhi)) return;
    const long wps = (long)a.nr * a.nq, base = s * wps;
    const long first = base + (long)rlo * a.nq + qlo, last = base + (long)rhi * a.nq + qhi, end = a.win0 + a.nwin;
    if (last < a.win0 || first >= end) return;
    const int N = a.win * a.win;
    const long plane = (long)a.Hs * a.Ws;
    float* out = a.cube + ((s * a.S + c) * P) * plane + (long)y * a.Ws + x;
    float acc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] = (k < P && first < a.win0) ? out[k * plane] : 0.f;
    for (int r = rlo; r <= rhi; ++r) {
        const long g0 = base + (long)r * a.nq;
        for (int q = qlo; q <= qhi; ++q) {
            const long g = g0 + q;
            if (g < a.win0 || g >= end) continue;
            const float* src = a.win_recon + (((g - a.win0) * a.S + c) * P) * N + (y - r * a.stride) * a.win + (x - q * a.stride);
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (k < P) acc[k] += src[k * N];
        }
    }
#pragma unroll
    for (int k = 0; k < 16; ++k)
        if (k < P) out[k * plane] = acc[k];
}

__global__ __launch_bounds__(256) void scene_recon_finalize_kernel(SceneReconArgs a) {
    __shared__ double werr[4];
    __shared__ int wcnt[4];
    const int tid = threadIdx.x;
    const long pb = blockIdx.x;   // (scene, band)
    const int C = a.S * a.P;
    const long s = pb / C;
    const int band = (int)(pb - s * C), c = band / a.P;
    const long plane = (long)a.Hs * a.Ws;
    const float* src = a.scene + pb * plane;
    float* out = a.cube + pb * plane;
    const uint8_t* msk = a.scene_mask + (s * a.S + c) * plane;
    int32_t* cov = band == 0 ? a.cover + s * plane : nullptr;
    double e = 0.0;
    int n = 0;
    for (long i = tid; i < plane; i += 256) {
        const int y = (int)(i / a.Ws), x = (int)(i - (long)y * a.Ws);
        int rlo, rhi, qlo, qhi;
        const int k = scene_cover(a, y, x, rlo, rhi, qlo, qhi) ? (rhi - rlo + 1) * (qhi - qlo + 1) : 0;
        const bool masked = msk[i] != 0;
        const float t = src[i];
        float v;
        if (k == 0) {
            v = a.blend ? t : __builtin_nanf("");   // nothing predicted here: the input's bits, or absent
        } else {
            const float pred = out[i] / (float)k;
            v = (a.blend && !masked) ? t : pred;
            if (masked) { e += fabs((double)pred - (double)t); ++n; }
        }
        out[i] = v;
        if (cov) cov[i] = k;
    }
    if (a.band_err) {   // one answer per launch
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { e += __shfl_xor(e, o); n += __shfl_xor(n, o); }
        if ((tid & 63) == 0) { werr[tid >> 6] = e; wcnt[tid >> 6] = n; }
        __syncthreads();
        if (tid == 0) {
            a.band_err[pb] = ((werr[0] + werr[1]) + werr[2]) + werr[3];
            a.band_cnt[pb] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        }
    }
}

}  // namespace

int launch_scene_recon_accumulate(const SceneReconArgs& a, long pixels, hipStream_t st) {
    if (pixels < 1) return 0;
    if (a.P > 16 || a.S > 65535) return MSST_ERR_UNSUPPORTED;
    const long grid = (pixels + 255) / 256;
    if (grid > 0x7fffffffL) return MSST_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(scene_recon_accumulate_kernel, dim3((unsigned)grid, a.S), dim3(256), 0, st, a, pixels);
    return (int)hipGetLastError();
}

int launch_scene_recon_finalize(const SceneReconArgs& a, hipStream_t st) {
    const long grid = (long)a.Bs * a.S * a.P;
    if (grid > 0x7fffffffL) return MSST_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(scene_recon_finalize_kernel, dim3((unsigned)grid), dim3(256), 0, st, a);
    return (int)hipGetLastError();
}

}  // namespace msst
