// Whole-scene SimMIM reconstruction, the assembling end (msst_scene_recon_assemble).  Per-window predictions win_recon
// [nwin][S P][win * win] (msst_recon_fwd, blend = 0, of windows of a scene) -> the scene cube [Bs][S P][Hs][Ws] = mean of the
// predictions of every window covering a pixel, blended with the scene where the token is not masked, with the per-band
// |prediction - scene| sums over the masked covered pixels and the cover map.
//
// The running sums are the shared fold's (scene_fold_kernel, msst_fwd.hip; launch_scene_fold with C = S P and the P bands of a
// spectral block per grid row); this file holds what is particular to pixels:
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

int launch_scene_recon_finalize(const SceneReconArgs& a, hipStream_t st) {
    const long grid = (long)a.Bs * a.S * a.P;
    if (grid > 0x7fffffffL) return MSST_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(scene_recon_finalize_kernel, dim3((unsigned)grid), dim3(256), 0, st, a);
    return (int)hipGetLastError();
}

}  // namespace msst
