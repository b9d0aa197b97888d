// Softmax cross entropy with ignore_index over class-major logits, with the gradient and every count the finetune training and
// validation loops need from one pass (reference src/utils.py:645-658: CrossEntropyLoss(ignore_index) forward and backward, the
// pixel accuracy on valid labels, the NaN check; finetune.py:144-146: macro accuracy; src/utils.py:531-541 in validation).
//
// Logits [R0][NC][M] fp32 ([B, nc, H, W]: R0 = B, M = H W; [B, nc]: M = 1), labels [R0][M] int64.  A row is one (sample, pixel).
//   ce_fwd      one lane per row; adjacent lanes take adjacent pixels, so each of the NC loads of a wave (stride M floats per
//               lane step c) is one coalesced segment when M > 1.  Row maximum and argmax (ties: lowest index; a NaN is the
//               maximum, as torch.argmax), sum of exp(x - max), loss = log sum + max - x[label], d = softmax - onehot written
//               in the logits' layout (zeros for rows that do not count).  NC <= 32: the row stays in registers (buckets 8 /
//               16 / 32); above: three passes over the row, the second and third out of L2.  A workgroup leaves ONE fp32 partial
//               of its rows' losses (wave shuffles, then the four waves in a fixed order) and one int32 slab row
//               [n_valid, n_correct, bad_labels, nonfinite, support[NC], correct[NC]] (LDS integer atomics, 1024 classes per
//               pass: any NC).  Nothing needs zeroing: every slab word is written.
//   ce_finish   workgroup 0: the partials in a fixed order (double, the pattern of loss_reduce) -> record slot 0 and the mean
//               loss (NaN over no rows); a wave per slab column -> the int64 slots of the record.
//   ce_bwd      dlogits = (d / n_valid) * gout, n_valid and gout read on the device.
// Integer sums are exact in any order, the float sum has one order: loss, record and gradient are bit-reproducible.
#include "msst_dev.h"
#include "msst_kernels.h"

namespace msst {

namespace {

constexpr int CE_CHUNK = 1024;   // classes per histogram pass (2 * CE_CHUNK ints of LDS)

// NR > 0: NC <= NR and the row lives in registers; NR == 0: any NC, the row is re-read.  WRITE: d is wanted
template <int NR, bool WRITE>
__global__ __launch_bounds__(256) void ce_fwd_kernel(CeArgs a) {
    __shared__ int hist[2 * CE_CHUNK];
    __shared__ int cnt[4];
    __shared__ float wsum[4];
    const int tid = threadIdx.x, NC = a.NC;
    const long r = (long)blockIdx.x * 256 + tid;
    const bool on = r < a.rows;
    if (tid < 4) cnt[tid] = 0;
    long label = a.ignore_index;
    bool skipped = false;
    long base = 0;
    if (on) {
        label = a.labels[r];
        skipped = a.skip && a.skip[r] < 0;
        const long r0 = r / a.M;
        base = r0 * NC * a.M + (r - r0 * a.M);
    }
    const bool cand = on && !skipped && label != a.ignore_index;   // would count, were its label a class
    const bool counts = cand && label >= 0 && label < NC;
    const bool bad = cand && !counts;
    const float* x = a.logits + base;
    float* d = WRITE ? a.d + base : nullptr;
    const long M = a.M;
    float loss = 0.f;
    bool hit = false, nonfin = false;
    if (on) {
        float mx = 0.f, sum = 0.f, xl = 0.f;
        int am = 0;
        if constexpr (NR > 0) {
            float v[NR];
#pragma unroll
            for (int c = 0; c < NR; ++c) v[c] = c < NC ? x[c * M] : 0.f;
            mx = v[0];
#pragma unroll
            for (int c = 1; c < NR; ++c)
                if (c < NC && (v[c] > mx || (v[c] != v[c] && mx == mx))) { mx = v[c]; am = c; }
#pragma unroll
            for (int c = 0; c < NR; ++c) {
                v[c] = c < NC ? expf(v[c] - mx) : 0.f;
                sum += v[c];
                if (c < NC && c == (int)label) xl = x[c * M];   // the logit again (one L1 hit): v holds the exponentials now
            }
            if (WRITE) {
                const float inv = 1.0f / sum;
#pragma unroll
                for (int c = 0; c < NR; ++c)
                    if (c < NC) d[c * M] = counts ? v[c] * inv - (c == (int)label ? 1.f : 0.f) : 0.f;
            }
        } else {
            mx = x[0];
            for (int c = 1; c < NC; ++c) {
                const float t = x[c * M];
                if (t > mx || (t != t && mx == mx)) { mx = t; am = c; }
            }
            for (int c = 0; c < NC; ++c) sum += expf(x[c * M] - mx);
            if (counts) xl = x[label * M];
            if (WRITE) {
                const float inv = 1.0f / sum;
                for (int c = 0; c < NC; ++c)
                    d[c * M] = counts ? expf(x[c * M] - mx) * inv - (c == (int)label ? 1.f : 0.f) : 0.f;
            }
        }
        if (counts) {
            loss = logf(sum) + mx - xl;
            hit = am == (int)label;
            nonfin = !(fabsf(loss) <= 3.402823466e38f);   // NaN or +-inf
        }
    }
    // the workgroup's loss partial: lanes of a wave by butterfly (every lane ends with the same sum), then the waves in order
    float ls = loss;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ls += __shfl_xor(ls, o);
    if ((tid & 63) == 0) wsum[tid >> 6] = ls;
    __syncthreads();   // cnt zeroed, wsum written
    const unsigned long long bv = __ballot(counts), bc = __ballot(hit), bb = __ballot(bad), bn = __ballot(nonfin);
    if ((tid & 63) == 0) {
        atomicAdd(&cnt[0], __popcll(bv));
        atomicAdd(&cnt[1], __popcll(bc));
        atomicAdd(&cnt[2], __popcll(bb));
        atomicAdd(&cnt[3], __popcll(bn));
    }
    int* row = a.slab + (long)blockIdx.x * (4 + 2L * NC);
    for (int c0 = 0; c0 < NC; c0 += CE_CHUNK) {
        const int n = NC - c0 < CE_CHUNK ? NC - c0 : CE_CHUNK;
        for (int i = tid; i < 2 * n; i += 256) hist[i] = 0;
        __syncthreads();
        if (counts && label >= c0 && label < c0 + n) {
            atomicAdd(&hist[(int)label - c0], 1);
            if (hit) atomicAdd(&hist[n + (int)label - c0], 1);
        }
        __syncthreads();
        for (int i = tid; i < n; i += 256) {
            row[4 + c0 + i] = hist[i];
            row[4 + NC + c0 + i] = hist[n + i];
        }
        __syncthreads();   // hist is zeroed again by the next pass
    }
    if (tid < 4) row[tid] = cnt[tid];
    if (tid == 0) a.partial[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// workgroup 0: loss; workgroups 1 ..: one wave per slab column (4 + 2 NC columns, G rows) -> int64 record slots 1 ..
__global__ __launch_bounds__(256) void ce_finish_kernel(CeArgs a, int G) {
    __shared__ double red[256];
    __shared__ long nred[256];
    const int tid = threadIdx.x;
    const long cols = 4 + 2L * a.NC;
    if (blockIdx.x == 0) {
        double s = 0.0;
        long n = 0;
        for (int i = tid; i < G; i += 256) {
            s += (double)a.partial[i];
            n += a.slab[(long)i * cols];
        }
        red[tid] = s;
        nred[tid] = n;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) { red[tid] += red[tid + o]; nred[tid] += nred[tid + o]; }
            __syncthreads();
        }
        if (tid == 0) {
            reinterpret_cast<double*>(a.record)[0] = red[0];
            *a.loss = nred[0] > 0 ? (float)(red[0] / (double)nred[0]) : __int_as_float(0x7fc00000);
        }
        return;
    }
    const long col = ((long)blockIdx.x - 1) * 4 + (tid >> 6);
    if (col >= cols) return;
    long s = 0;
    for (int i = tid & 63; i < G; i += 64) s += a.slab[(long)i * cols + col];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((tid & 63) == 0) a.record[1 + col] = s;
}

template <bool VEC>
__global__ __launch_bounds__(256) void ce_bwd_kernel(const float* d, const int64_t* record, const float* gout, float* dl, long n) {
    const long nv = record[1];
    const float inv = nv > 0 ? 1.0f / (float)nv : 0.f;   // no row counts: d is all zero, and so is the gradient
    const float g = gout ? *gout : 1.f;
    const long stride = (long)gridDim.x * 256;
    if constexpr (VEC) {
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n / 4; i += stride) {
            f32x4 q = reinterpret_cast<const f32x4*>(d)[i];
            q[0] = q[0] * inv * g; q[1] = q[1] * inv * g; q[2] = q[2] * inv * g; q[3] = q[3] * inv * g;
            reinterpret_cast<f32x4*>(dl)[i] = q;
        }
    } else {
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) dl[i] = d[i] * inv * g;
    }
}

template <bool WRITE>
void launch_fwd(const CeArgs& a, int G, hipStream_t st) {
    if (a.NC <= 8) hipLaunchKernelGGL((ce_fwd_kernel<8, WRITE>), dim3(G), dim3(256), 0, st, a);
    else if (a.NC <= 16) hipLaunchKernelGGL((ce_fwd_kernel<16, WRITE>), dim3(G), dim3(256), 0, st, a);
    else if (a.NC <= 32) hipLaunchKernelGGL((ce_fwd_kernel<32, WRITE>), dim3(G), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((ce_fwd_kernel<0, WRITE>), dim3(G), dim3(256), 0, st, a);
}

}  // namespace

int ce_workgroups(long rows) { return (int)((rows + 255) / 256); }

int launch_ce_fwd(const CeArgs& a, hipStream_t st) {
    const int G = ce_workgroups(a.rows);
    ProfScope ps(K_CE, st);
    if (a.d) launch_fwd<true>(a, G, st);
    else launch_fwd<false>(a, G, st);
    return (int)hipGetLastError();
}

int launch_ce_finish(const CeArgs& a, hipStream_t st) {
    const int G = ce_workgroups(a.rows);
    const long cols = 4 + 2L * a.NC;
    ProfScope ps(K_CE, st);
    hipLaunchKernelGGL(ce_finish_kernel, dim3((unsigned)(1 + (cols + 3) / 4)), dim3(256), 0, st, a, G);
    return (int)hipGetLastError();
}

int launch_ce_bwd(const float* d, const int64_t* record, const float* gout, float* dlogits, long n, hipStream_t st) {
    ProfScope ps(K_CE, st);
    const bool vec = n % 4 == 0 && ((uintptr_t)d % 16) == 0 && ((uintptr_t)dlogits % 16) == 0;
    long g = ((vec ? n / 4 : n) + 255) / 256;
    if (g > 2048) g = 2048;
    if (vec) hipLaunchKernelGGL(ce_bwd_kernel<true>, dim3((unsigned)g), dim3(256), 0, st, d, record, gout, dlogits, n);
    else hipLaunchKernelGGL(ce_bwd_kernel<false>, dim3((unsigned)g), dim3(256), 0, st, d, record, gout, dlogits, n);
    return (int)hipGetLastError();
}

// ---- the second forward family: class weights, label smoothing, confusion matrix (torch's CrossEntropyLoss(weight,
// label_smoothing), reduction "mean"; the DeepHyperX protocol's weighted loss and its confusion matrix).  The layout, the row
// rules and the count record are ce_fwd's.
//   ce_ext_fwd     WEIGHTED = false (no weight, eps = 0): the row arithmetic of ce_fwd, expression for expression, so that a call
//                  that only adds the confusion matrix gives the bits of ce_fwd.  WEIGHTED: with t_k = x_k - max, L = log sum exp t,
//                  W = sum_k w_k:  l = (1 - eps) w_y (L - t_y) + (eps / NC) (L W - sum_k w_k t_k),
//                  d_c = softmax_c ((1 - eps) w_y + (eps / NC) W) - (1 - eps) w_y [c == y] - (eps / NC) w_c.
//                  A workgroup leaves a second fp32 partial, of its rows' w_y (reduced in the order of the loss partial), and, when
//                  the confusion matrix is wanted, an int32 slab row [NC][NC] (label, argmax) of its counting rows: the LDS
//                  histogram again, CE_CHUNK / NC label rows per pass.
//   ce_ext_finish  workgroup 0: both partial arrays in double, in a fixed order -> sums[0] (= record slot 0) and sums[1], loss =
//                  sums[0] / sums[1] (NaN unless sums[1] > 0); then the record columns as ce_finish; then one lane per confusion
//                  column over the slab rows -> int64.
//   ce_ext_bwd     dlogits = (d / sums[1]) * gout, zeros unless sums[1] > 0.
namespace {

constexpr int CE_CONF_WORDS = 2 * CE_CHUNK;   // LDS words of a confusion pass: CE_CONF_WORDS / NC label rows at a time

template <int NR, bool WRITE, bool WEIGHTED>
__global__ __launch_bounds__(256) void ce_ext_fwd_kernel(CeExtArgs e) {
    __shared__ int hist[2 * CE_CHUNK];
    __shared__ int cnt[4];
    __shared__ float wsum[4], wwsum[4];
    const CeArgs& a = e.c;
    const int tid = threadIdx.x, NC = a.NC;
    const long r = (long)blockIdx.x * 256 + tid;
    const bool on = r < a.rows;
    if (tid < 4) cnt[tid] = 0;
    long label = a.ignore_index;
    bool skipped = false;
    long base = 0;
    if (on) {
        label = a.labels[r];
        skipped = a.skip && a.skip[r] < 0;
        const long r0 = r / a.M;
        base = r0 * NC * a.M + (r - r0 * a.M);
    }
    const bool cand = on && !skipped && label != a.ignore_index;   // would count, were its label a class
    const bool counts = cand && label >= 0 && label < NC;
    const bool bad = cand && !counts;
    const float* x = a.logits + base;
    float* d = WRITE ? a.d + base : nullptr;
    const long M = a.M;
    const float keep = 1.0f - e.eps, smooth = e.eps / (float)NC;
    float loss = 0.f, wrow = 0.f;
    bool hit = false, nonfin = false;
    int am = 0;
    if (on) {
        float mx = 0.f, sum = 0.f, xl = 0.f;
        float wy = 0.f, W = 0.f, swt = 0.f;   // WEIGHTED: w[label], sum_k w[k], sum_k w[k] (x[k] - mx); xl = x[label] - mx
        if constexpr (NR > 0) {
            float v[NR];
#pragma unroll
            for (int c = 0; c < NR; ++c) v[c] = c < NC ? x[c * M] : 0.f;
            mx = v[0];
#pragma unroll
            for (int c = 1; c < NR; ++c)
                if (c < NC && (v[c] > mx || (v[c] != v[c] && mx == mx))) { mx = v[c]; am = c; }
            if constexpr (!WEIGHTED) {
#pragma unroll
                for (int c = 0; c < NR; ++c) {
                    v[c] = c < NC ? expf(v[c] - mx) : 0.f;
                    sum += v[c];
                    if (c < NC && c == (int)label) xl = x[c * M];
                }
                if (WRITE) {
                    const float inv = 1.0f / sum;
#pragma unroll
                    for (int c = 0; c < NR; ++c)
                        if (c < NC) d[c * M] = counts ? v[c] * inv - (c == (int)label ? 1.f : 0.f) : 0.f;
                }
            } else {
#pragma unroll
                for (int c = 0; c < NR; ++c) {
                    if (c < NC) {
                        const float wk = e.w ? e.w[c] : 1.f;
                        const float t = v[c] - mx;
                        W += wk;
                        swt += wk * t;
                        if (c == (int)label) { xl = t; wy = wk; }
                        v[c] = expf(t);
                        sum += v[c];
                    }
                }
                if (WRITE) {
                    const float inv = 1.0f / sum, hot = keep * wy, coef = hot + smooth * W;
#pragma unroll
                    for (int c = 0; c < NR; ++c)
                        if (c < NC)
                            d[c * M] = counts ? v[c] * inv * coef - (c == (int)label ? hot : 0.f) - smooth * (e.w ? e.w[c] : 1.f) : 0.f;
                }
            }
        } else {
            mx = x[0];
            for (int c = 1; c < NC; ++c) {
                const float t = x[c * M];
                if (t > mx || (t != t && mx == mx)) { mx = t; am = c; }
            }
            if constexpr (!WEIGHTED) {
                for (int c = 0; c < NC; ++c) sum += expf(x[c * M] - mx);
                if (counts) xl = x[label * M];
                if (WRITE) {
                    const float inv = 1.0f / sum;
                    for (int c = 0; c < NC; ++c)
                        d[c * M] = counts ? expf(x[c * M] - mx) * inv - (c == (int)label ? 1.f : 0.f) : 0.f;
                }
            } else {
                for (int c = 0; c < NC; ++c) {
                    const float wk = e.w ? e.w[c] : 1.f;
                    const float t = x[c * M] - mx;
                    W += wk;
                    swt += wk * t;
                    sum += expf(t);
                }
                if (counts) { xl = x[label * M] - mx; wy = e.w ? e.w[label] : 1.f; }
                if (WRITE) {
                    const float inv = 1.0f / sum, hot = keep * wy, coef = hot + smooth * W;
                    for (int c = 0; c < NC; ++c)
                        d[c * M] = counts ? expf(x[c * M] - mx) * inv * coef - (c == (int)label ? hot : 0.f) - smooth * (e.w ? e.w[c] : 1.f)
                                          : 0.f;
                }
            }
        }
        if (counts) {
            if constexpr (WEIGHTED) {
                const float L = logf(sum);
                loss = keep * wy * (L - xl) + smooth * (L * W - swt);
                wrow = wy;
            } else {
                loss = logf(sum) + mx - xl;
                wrow = 1.f;
            }
            hit = am == (int)label;
            nonfin = !(fabsf(loss) <= 3.402823466e38f);   // NaN or +-inf
        }
    }
    // the workgroup's two partials, in one order: lanes of a wave by butterfly, then the waves in order
    float ls = loss, ws = wrow;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { ls += __shfl_xor(ls, o); ws += __shfl_xor(ws, o); }
    if ((tid & 63) == 0) { wsum[tid >> 6] = ls; wwsum[tid >> 6] = ws; }
    __syncthreads();   // cnt zeroed, wsum / wwsum written
    const unsigned long long bv = __ballot(counts), bc = __ballot(hit), bb = __ballot(bad), bn = __ballot(nonfin);
    if ((tid & 63) == 0) {
        atomicAdd(&cnt[0], __popcll(bv));
        atomicAdd(&cnt[1], __popcll(bc));
        atomicAdd(&cnt[2], __popcll(bb));
        atomicAdd(&cnt[3], __popcll(bn));
    }
    int* row = a.slab + (long)blockIdx.x * (4 + 2L * NC);
    for (int c0 = 0; c0 < NC; c0 += CE_CHUNK) {
        const int n = NC - c0 < CE_CHUNK ? NC - c0 : CE_CHUNK;
        for (int i = tid; i < 2 * n; i += 256) hist[i] = 0;
        __syncthreads();
        if (counts && label >= c0 && label < c0 + n) {
            atomicAdd(&hist[(int)label - c0], 1);
            if (hit) atomicAdd(&hist[n + (int)label - c0], 1);
        }
        __syncthreads();
        for (int i = tid; i < n; i += 256) {
            row[4 + c0 + i] = hist[i];
            row[4 + NC + c0 + i] = hist[n + i];
        }
        __syncthreads();   // hist is zeroed again by the next pass
    }
    if (e.cslab) {   // NC <= CE_CONF_MAX_CLASSES (the caller checked): at least CE_CONF_WORDS / NC >= 1 label rows per pass
        int* crow = e.cslab + (long)blockIdx.x * NC * NC;
        const int per = CE_CONF_WORDS / NC;
        for (int l0 = 0; l0 < NC; l0 += per) {
            const int n = (NC - l0 < per ? NC - l0 : per) * NC;   // words of this pass: label rows l0 .. of the matrix
            for (int i = tid; i < n; i += 256) hist[i] = 0;
            __syncthreads();
            if (counts && label >= l0 && (int)(label - l0) * NC < n) atomicAdd(&hist[(int)(label - l0) * NC + am], 1);
            __syncthreads();
            for (int i = tid; i < n; i += 256) crow[l0 * NC + i] = hist[i];
            __syncthreads();
        }
    }
    if (tid < 4) row[tid] = cnt[tid];
    if (tid == 0) {
        a.partial[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
        e.wpartial[blockIdx.x] = (wwsum[0] + wwsum[1]) + (wwsum[2] + wwsum[3]);
    }
}

// workgroup 0: loss and weight sums; workgroups 1 .. RB: a wave per slab column -> record (as ce_finish); the rest: a lane per
// confusion column (adjacent lanes on adjacent columns of a slab row)
__global__ __launch_bounds__(256) void ce_ext_finish_kernel(CeExtArgs e, int G, int RB) {
    __shared__ double red[256], wred[256];
    const CeArgs& a = e.c;
    const int tid = threadIdx.x;
    const long cols = 4 + 2L * a.NC;
    if (blockIdx.x == 0) {
        double s = 0.0, w = 0.0;
        for (int i = tid; i < G; i += 256) {
            s += (double)a.partial[i];
            w += (double)e.wpartial[i];
        }
        red[tid] = s;
        wred[tid] = w;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) { red[tid] += red[tid + o]; wred[tid] += wred[tid + o]; }
            __syncthreads();
        }
        if (tid == 0) {
            reinterpret_cast<double*>(a.record)[0] = red[0];
            e.sums[0] = red[0];
            e.sums[1] = wred[0];
            *a.loss = wred[0] > 0.0 ? (float)(red[0] / wred[0]) : __int_as_float(0x7fc00000);
        }
        return;
    }
    if ((int)blockIdx.x <= RB) {
        const long col = ((long)blockIdx.x - 1) * 4 + (tid >> 6);
        if (col >= cols) return;
        long s = 0;
        for (int i = tid & 63; i < G; i += 64) s += a.slab[(long)i * cols + col];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if ((tid & 63) == 0) a.record[1 + col] = s;
        return;
    }
    const long cc = (long)a.NC * a.NC;
    const long col = ((long)blockIdx.x - 1 - RB) * 256 + tid;
    if (col >= cc) return;
    long s = 0;
    for (int i = 0; i < G; ++i) s += e.cslab[(long)i * cc + col];
    e.confusion[col] = s;
}

template <bool VEC>
__global__ __launch_bounds__(256) void ce_ext_bwd_kernel(const float* d, const double* sums, const float* gout, float* dl, long n) {
    const double ws = sums[1];
    const float inv = ws > 0.0 ? 1.0f / (float)ws : 0.f;   // nothing counts, or only rows of weight 0: the gradient is zero
    const float g = gout ? *gout : 1.f;
    const long stride = (long)gridDim.x * 256;
    if constexpr (VEC) {
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n / 4; i += stride) {
            f32x4 q = reinterpret_cast<const f32x4*>(d)[i];
            q[0] = q[0] * inv * g; q[1] = q[1] * inv * g; q[2] = q[2] * inv * g; q[3] = q[3] * inv * g;
            reinterpret_cast<f32x4*>(dl)[i] = q;
        }
    } else {
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) dl[i] = d[i] * inv * g;
    }
}

template <bool WRITE, bool WEIGHTED>
void launch_ext_fwd(const CeExtArgs& e, int G, hipStream_t st) {
    const int NC = e.c.NC;
    if (NC <= 8) hipLaunchKernelGGL((ce_ext_fwd_kernel<8, WRITE, WEIGHTED>), dim3(G), dim3(256), 0, st, e);
    else if (NC <= 16) hipLaunchKernelGGL((ce_ext_fwd_kernel<16, WRITE, WEIGHTED>), dim3(G), dim3(256), 0, st, e);
    else if (NC <= 32) hipLaunchKernelGGL((ce_ext_fwd_kernel<32, WRITE, WEIGHTED>), dim3(G), dim3(256), 0, st, e);
    else hipLaunchKernelGGL((ce_ext_fwd_kernel<0, WRITE, WEIGHTED>), dim3(G), dim3(256), 0, st, e);
}

}  // namespace

static_assert(CE_CONF_MAX_CLASSES <= CE_CONF_WORDS, "a confusion pass holds at least one label row");

int launch_ce_ext_fwd(const CeExtArgs& e, hipStream_t st) {
    const int G = ce_workgroups(e.c.rows);
    const bool weighted = e.w != nullptr || e.eps != 0.f;
    ProfScope ps(K_CE, st);
    if (e.c.d) {
        if (weighted) launch_ext_fwd<true, true>(e, G, st);
        else launch_ext_fwd<true, false>(e, G, st);
    } else {
        if (weighted) launch_ext_fwd<false, true>(e, G, st);
        else launch_ext_fwd<false, false>(e, G, st);
    }
    return (int)hipGetLastError();
}

int launch_ce_ext_finish(const CeExtArgs& e, hipStream_t st) {
    const int G = ce_workgroups(e.c.rows);
    const long cols = 4 + 2L * e.c.NC;
    const int RB = (int)((cols + 3) / 4);
    const long CB = e.cslab ? ((long)e.c.NC * e.c.NC + 255) / 256 : 0;
    ProfScope ps(K_CE, st);
    hipLaunchKernelGGL(ce_ext_finish_kernel, dim3((unsigned)(1 + RB + CB)), dim3(256), 0, st, e, G, RB);
    return (int)hipGetLastError();
}

int launch_ce_ext_bwd(const float* d, const double* sums, const float* gout, float* dlogits, long n, hipStream_t st) {
    ProfScope ps(K_CE, st);
    const bool vec = n % 4 == 0 && ((uintptr_t)d % 16) == 0 && ((uintptr_t)dlogits % 16) == 0;
    long g = ((vec ? n / 4 : n) + 255) / 256;
    if (g > 2048) g = 2048;
    if (vec) hipLaunchKernelGGL(ce_ext_bwd_kernel<true>, dim3((unsigned)g), dim3(256), 0, st, d, sums, gout, dlogits, n);
    else hipLaunchKernelGGL(ce_ext_bwd_kernel<false>, dim3((unsigned)g), dim3(256), 0, st, d, sums, gout, dlogits, n);
    return (int)hipGetLastError();
}

}  // namespace msst
