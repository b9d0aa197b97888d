// Gradient accumulation over micro-batches and the global-norm clip, as streaming passes over the flat gradient buffers
// (msst_grad_accumulate, msst_grad_finalize).  One launch each over a table of disjoint element ranges -- the trainable, unfrozen
// parts of the flat buffer -- instead of one small kernel per parameter tensor:
//   accumulate:  a = first ? g : acc + g;  acc = a;  [out = a * scale;]  [workgroup partial of sum a^2 (double) and of non-finite a]
//   finalize:    total = scale * sqrt(sum of the partials);  coef = min(1, max_norm / (total + 1e-6));  g = (acc * scale) * coef
// the operations of torch.nn.utils.clip_grad_norm_ on the mean gradient.  No atomics and nothing to zero beforehand: a workgroup
// owns its slot of the partials, sums in a fixed order, and every workgroup of the finalize launch re-reduces all slots in the same
// fixed order, so two calls on the same input give the same bits.  A range's 16-byte aligned interior moves as dwordx4, its ragged
// ends (at most 3 + 3 floats) as single floats through the range's first workgroup, as in adam_groups_kernel.
#include "msst_dev.h"
#include "msst_kernels.h"
#include <math.h>

namespace msst {

__device__ __forceinline__ unsigned grad_nonfinite(float a) { return (__float_as_uint(a) & 0x7f800000u) == 0x7f800000u ? 1u : 0u; }

__device__ __forceinline__ GradSeg grad_seg_of_block(const GradTable& t) {
    int si = 0;
    while (si + 1 < t.nseg && (int)blockIdx.x >= t.s[si + 1].blk0) ++si;   // (block uniform)
    return t.s[si];
}

// sum over the 256 threads in a fixed order (shuffle tree inside a wave, then the four waves in order); the result is thread 0's
__device__ __forceinline__ void grad_block_sum(double& sum, unsigned& bad, double* sh_sum, unsigned* sh_bad) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sum += __shfl_down(sum, o);
        bad += __shfl_down(bad, o);
    }
    if (lane_id() == 0) { sh_sum[threadIdx.x >> 6] = sum; sh_bad[threadIdx.x >> 6] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        sum = ((sh_sum[0] + sh_sum[1]) + sh_sum[2]) + sh_sum[3];
        bad = sh_bad[0] + sh_bad[1] + sh_bad[2] + sh_bad[3];
    }
}

// out may be g itself (a lane reads its elements before it writes them), so g and out are not __restrict__
template <bool NORM>
__global__ __launch_bounds__(256) void grad_accum_kernel(float* acc, const float* g, float* out, float scale, int first,
                                                         double* part_sum, unsigned* part_bad, GradTable t) {
    const GradSeg s = grad_seg_of_block(t);
    const int lb = (int)blockIdx.x - s.blk0;
    f32x4* acc4 = reinterpret_cast<f32x4*>(acc);
    const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
    f32x4* out4 = reinterpret_cast<f32x4*>(out);
    double sum = 0.0;
    unsigned bad = 0;
    constexpr int U = GRAD_U;
    const long qend = s.a1 >> 2;
    for (long q0 = (s.a0 >> 2) + (long)lb * (256 * U) + threadIdx.x; q0 < qend; q0 += (long)s.nblk * (256 * U)) {
        // every load of the trip before its first store: a lane only ever rewrites what it has read itself
        f32x4 a[U], b[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (q0 + u * 256 < qend) a[u] = g4[q0 + u * 256];
        if (!first) {
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (q0 + u * 256 < qend) b[u] = acc4[q0 + u * 256];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long q = q0 + u * 256;
            if (q < qend) {
                if (!first) a[u] = b[u] + a[u];
                acc4[q] = a[u];
                if (out) out4[q] = a[u] * scale;
                if (NORM) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) { sum += (double)a[u][e] * (double)a[u][e]; bad += grad_nonfinite(a[u][e]); }
                }
            }
        }
    }
    if (lb == 0) {
        // ragged ends: [start, a0) and [a1, end) -- or the whole range when the buffers themselves are not 16-byte aligned
        const long nhead = s.a0 - s.start, ntail = s.end - s.a1;
        for (long k = threadIdx.x; k < nhead + ntail; k += 256) {
            const long i = k < nhead ? s.start + k : s.a1 + (k - nhead);
            float a = g[i];
            if (!first) a = acc[i] + a;
            acc[i] = a;
            if (out) out[i] = a * scale;
            if (NORM) { sum += (double)a * (double)a; bad += grad_nonfinite(a); }
        }
    }
    if (NORM) {
        __shared__ double sh_sum[4];
        __shared__ unsigned sh_bad[4];
        grad_block_sum(sum, bad, sh_sum, sh_bad);
        if (threadIdx.x == 0) { part_sum[blockIdx.x] = sum; part_bad[blockIdx.x] = bad; }
    }
}

__global__ __launch_bounds__(256) void grad_finalize_kernel(const float* __restrict__ acc, float* __restrict__ g, float scale,
                                                            float max_norm, const double* __restrict__ part_sum,
                                                            const unsigned* __restrict__ part_bad, int nparts,
                                                            float* __restrict__ record, GradTable t) {
    __shared__ double sh_sum[4];
    __shared__ unsigned sh_bad[4];
    __shared__ float sh_coef;
    // every workgroup forms the same total from the same partials in the same order: thread i sums slots [i c, (i + 1) c) in index
    // order, then the fixed tree over the threads
    const int c = (nparts + 255) / 256;
    const int i0 = (int)threadIdx.x * c, i1 = min(nparts, i0 + c);
    double sum = 0.0;
    unsigned bad = 0;
    for (int i = i0; i < i1; ++i) { sum += part_sum[i]; bad += part_bad[i]; }
    grad_block_sum(sum, bad, sh_sum, sh_bad);
    if (threadIdx.x == 0) {
        const float total = (float)((double)scale * sqrt(sum));
        const float coef = max_norm > 0.f ? fminf(1.f, max_norm / (total + 1e-6f)) : 1.f;
        sh_coef = coef;
        if (blockIdx.x == 0) { record[0] = total; record[1] = coef; record[2] = (float)bad; record[3] = 0.f; }
    }
    __syncthreads();
    const float coef = sh_coef;

    const GradSeg s = grad_seg_of_block(t);
    const int lb = (int)blockIdx.x - s.blk0;
    const f32x4* acc4 = reinterpret_cast<const f32x4*>(acc);
    f32x4* g4 = reinterpret_cast<f32x4*>(g);
    constexpr int U = GRAD_U;
    const long qend = s.a1 >> 2;
    for (long q0 = (s.a0 >> 2) + (long)lb * (256 * U) + threadIdx.x; q0 < qend; q0 += (long)s.nblk * (256 * U)) {
        f32x4 a[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (q0 + u * 256 < qend) a[u] = acc4[q0 + u * 256];
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (q0 + u * 256 < qend) g4[q0 + u * 256] = (a[u] * scale) * coef;
    }
    if (lb == 0) {
        const long nhead = s.a0 - s.start, ntail = s.end - s.a1;
        for (long k = threadIdx.x; k < nhead + ntail; k += 256) {
            const long i = k < nhead ? s.start + k : s.a1 + (k - nhead);
            g[i] = (acc[i] * scale) * coef;
        }
    }
}

int launch_grad_accumulate(float* acc, const float* g, float* out, float scale, int first, double* part_sum, unsigned* part_bad,
                           const GradTable& t, hipStream_t st) {
    if (t.nseg < 1 || t.nblocks < 1) return 0;
    ProfScope ps(K_GRAD_ACCUM, st);
    if (part_sum)
        hipLaunchKernelGGL(grad_accum_kernel<true>, dim3((unsigned)t.nblocks), dim3(256), 0, st, acc, g, out, scale, first, part_sum, part_bad, t);
    else
        hipLaunchKernelGGL(grad_accum_kernel<false>, dim3((unsigned)t.nblocks), dim3(256), 0, st, acc, g, out, scale, first, part_sum, part_bad, t);
    return (int)hipGetLastError();
}

int launch_grad_finalize(const float* acc, float* g, float scale, float max_norm, const double* part_sum, const unsigned* part_bad,
                         int nparts, float* record, const GradTable& t, hipStream_t st) {
    if (t.nseg < 1 || t.nblocks < 1) return 0;
    ProfScope ps(K_GRAD_FINAL, st);
    hipLaunchKernelGGL(grad_finalize_kernel, dim3((unsigned)t.nblocks), dim3(256), 0, st, acc, g, scale, max_norm, part_sum, part_bad, nparts,
                       record, t);
    return (int)hipGetLastError();
}

}  // namespace msst
