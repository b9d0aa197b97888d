// Softmax cross entropy with ignore_index over class-major logits, with the gradient and every count the finetune training and
// validation loops need from one pass (reference src/utils.py:645-658: CrossEntropyLoss(ignore_index) forward and backward, the
// pixel accuracy on valid labels, the NaN check; finetune.py:144-146: macro accuracy; src/utils.py:531-541 in validation), and
// optionally with class weights, label smoothing and a confusion matrix (torch's CrossEntropyLoss(weight, label_smoothing),
// reduction "mean"; the DeepHyperX protocol's weighted loss and its confusion matrix).  ONE kernel family: the plain entry points
// (msst_ce_stats_fwd / msst_ce_bwd) launch its unweighted instances with no confusion slab and no sums.
//
// Logits [R0][NC][M] fp32 ([B, nc, H, W]: R0 = B, M = H W; [B, nc]: M = 1), labels [R0][M] int64.  A row is one (sample, pixel).
//   ce_fwd      one lane per row; adjacent lanes take adjacent pixels, so each of the NC loads of a wave (stride M floats per
//               lane step c) is one coalesced segment when M > 1.  Row maximum and argmax (ties: lowest index; a NaN is the
//               maximum, as torch.argmax), sum of exp(x - max).  NC <= 32: the row stays in registers (buckets 8 / 16 / 32);
//               above: three passes over the row, the second and third out of L2.
//               Unweighted (no weight, eps = 0): loss = log sum + max - x[label], d = softmax - onehot.
//               Weighted: with t_k = x_k - max, L = log sum exp t, W = sum_k w_k:
//                 l = (1 - eps) w_y (L - t_y) + (eps / NC) (L W - sum_k w_k t_k),
//                 d_c = softmax_c ((1 - eps) w_y + (eps / NC) W) - (1 - eps) w_y [c == y] - (eps / NC) w_c.
//               d is written in the logits' layout (zeros for rows that do not count).  A workgroup leaves ONE fp32 partial of its
//               rows' losses (wave shuffles, then the four waves in a fixed order); weighted, a second one, of its rows' w_y, in the
//               same order; one int32 slab row [n_valid, n_correct, bad_labels, nonfinite, support[NC], correct[NC]] (LDS integer
//               atomics, 1024 classes per pass: any NC); and, when the confusion matrix is wanted, an int32 slab row [NC][NC]
//               (label, argmax) of its counting rows: the LDS histogram again, CE_CONF_WORDS / NC label rows per pass.  Nothing needs
//               zeroing: every slab word is written.
//   ce_finish   workgroup 0: the loss partials and the denominator's (weighted: the w_y partials; unweighted: the slab's n_valid
//               column, the same exact integer) in double, in a fixed order (the pattern of loss_reduce) -> record slot 0, the mean
//               loss (NaN unless the denominator is > 0) and, where wanted, sums[0] (= record slot 0) and sums[1], the denominator;
//               a wave per slab column -> the int64 slots of the record; a lane per confusion column over the slab rows -> int64.
//   ce_bwd      dlogits = (d / den[1]) * gout, zeros unless den[1] > 0; den is the int64 record (n_valid) or the double sums, and
//               gout is read on the device.
// Integer sums are exact in any order, the float sums have one order: loss, record, sums and gradient are bit-reproducible.
#include "msst_dev.h"
#include "msst_kernels.h"

#include <type_traits>

namespace msst {

namespace {

constexpr int CE_CHUNK = 1024;                // classes per histogram pass (2 * CE_CHUNK ints of LDS)
constexpr int CE_CONF_WORDS = 2 * CE_CHUNK;   // LDS words of a confusion pass: CE_CONF_WORDS / NC label rows at a time

// a call with class weights or label smoothing: the second partial, the weighted row arithmetic, sums[1] from the w_y partials
inline bool ce_weighted(const CeArgs& a) { return a.w != nullptr || a.eps != 0.f; }

// ---- the lane's row
struct CeLane {
    long label, base;          // base: the row's class 0 in logits / d
    bool on, counts, bad;      // a row of the input; it counts; it would count, were its label a class
};

__device__ __forceinline__ CeLane ce_lane(const CeArgs& a) {
    CeLane r;
    const long row = (long)blockIdx.x * 256 + threadIdx.x;
    r.on = row < a.rows;
    r.label = a.ignore_index;
    r.base = 0;
    bool skipped = false;
    if (r.on) {
        r.label = a.labels[row];
        skipped = a.skip && a.skip[row] < 0;
        const long r0 = row / a.M;
        r.base = r0 * a.NC * a.M + (row - r0 * a.M);
    }
    const bool cand = r.on && !skipped && r.label != a.ignore_index;
    r.counts = cand && r.label >= 0 && r.label < a.NC;
    r.bad = cand && !r.counts;
    return r;
}

// lanes of a wave by butterfly: every lane ends with the same sum.  Several values go through one loop, so that their shuffles
// overlap (one after the other, the weighted forward takes 0.3 us longer)
template <class... T>
__device__ __forceinline__ void ce_wave_sum(T&... v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ((v += __shfl_xor(v, o)), ...);
}

// ---- row arithmetic.  NR > 0: NC <= NR and the row lives in registers (v); NR == 0: any NC, the row is re-read.  WRITE: d is wanted
template <int NR>
using CeRegs = float[NR > 0 ? NR : 1];

// the row's maximum; am: its index
template <int NR>
__device__ __forceinline__ float ce_row_max(const float* x, long M, int NC, CeRegs<NR>& v, int& am) {
    float mx;
    if constexpr (NR > 0) {
#pragma unroll
        for (int c = 0; c < NR; ++c) v[c] = c < NC ? x[c * M] : 0.f;
        mx = v[0];
#pragma unroll
        for (int c = 1; c < NR; ++c)
            if (c < NC && (v[c] > mx || (v[c] != v[c] && mx == mx))) { mx = v[c]; am = c; }
    } else {
        mx = x[0];
        for (int c = 1; c < NC; ++c) {
            const float t = x[c * M];
            if (t > mx || (t != t && mx == mx)) { mx = t; am = c; }
        }
    }
    return mx;
}

// -> the row's loss (0 unless it counts)
template <int NR, bool WRITE>
__device__ __forceinline__ float ce_row_unweighted(const CeArgs& a, const CeLane& r, int& am) {
    const float* x = a.logits + r.base;
    float* d = WRITE ? a.d + r.base : nullptr;
    const long M = a.M, label = r.label;
    const int NC = a.NC;
    const bool counts = r.counts;
    CeRegs<NR> v;
    const float mx = ce_row_max<NR>(x, M, NC, v, am);
    float sum = 0.f, xl = 0.f;
    if constexpr (NR > 0) {
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
        for (int c = 0; c < NC; ++c) sum += expf(x[c * M] - mx);
        if (counts) xl = x[label * M];
        if (WRITE) {
            const float inv = 1.0f / sum;
            for (int c = 0; c < NC; ++c)
                d[c * M] = counts ? expf(x[c * M] - mx) * inv - (c == (int)label ? 1.f : 0.f) : 0.f;
        }
    }
    return counts ? logf(sum) + mx - xl : 0.f;
}

// -> the row's loss; wrow: w[label], what the row adds to the denominator (both 0 unless it counts)
template <int NR, bool WRITE>
__device__ __forceinline__ float ce_row_weighted(const CeArgs& a, const CeLane& r, int& am, float& wrow) {
    const float* x = a.logits + r.base;
    float* d = WRITE ? a.d + r.base : nullptr;
    const long M = a.M, label = r.label;
    const int NC = a.NC;
    const bool counts = r.counts;
    const float keep = 1.0f - a.eps, smooth = a.eps / (float)NC;
    CeRegs<NR> v;
    const float mx = ce_row_max<NR>(x, M, NC, v, am);
    float sum = 0.f, xl = 0.f, wy = 0.f, W = 0.f, swt = 0.f;   // x[label] - mx, w[label], sum_k w[k], sum_k w[k] (x[k] - mx)
    if constexpr (NR > 0) {
#pragma unroll
        for (int c = 0; c < NR; ++c) {
            if (c < NC) {
                const float wk = a.w ? a.w[c] : 1.f;
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
                    d[c * M] = counts ? v[c] * inv * coef - (c == (int)label ? hot : 0.f) - smooth * (a.w ? a.w[c] : 1.f) : 0.f;
        }
    } else {
        for (int c = 0; c < NC; ++c) {
            const float wk = a.w ? a.w[c] : 1.f;
            const float t = x[c * M] - mx;
            W += wk;
            swt += wk * t;
            sum += expf(t);
        }
        if (counts) { xl = x[label * M] - mx; wy = a.w ? a.w[label] : 1.f; }
        if (WRITE) {
            const float inv = 1.0f / sum, hot = keep * wy, coef = hot + smooth * W;
            for (int c = 0; c < NC; ++c)
                d[c * M] = counts ? expf(x[c * M] - mx) * inv * coef - (c == (int)label ? hot : 0.f) - smooth * (a.w ? a.w[c] : 1.f)
                                  : 0.f;
        }
    }
    if (!counts) return 0.f;
    const float L = logf(sum);
    wrow = wy;
    return keep * wy * (L - xl) + smooth * (L * W - swt);
}

// ---- the workgroup's count row: [n_valid, n_correct, bad_labels, nonfinite] by ballots into cnt (zeroed before the caller's last
// barrier; complete when this returns, the caller stores it), support[NC] and correct[NC] by LDS histogram passes of CE_CHUNK
// classes (NC >= 1: at least one).  Ends on a barrier: hist is free again
__device__ __forceinline__ void ce_count_row(const CeArgs& a, const CeLane& r, bool hit, bool nonfin, int* hist, int* cnt) {
    const int tid = threadIdx.x, NC = a.NC;
    const long label = r.label;
    const unsigned long long bv = __ballot(r.counts), bc = __ballot(hit), bb = __ballot(r.bad), bn = __ballot(nonfin);
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
        if (r.counts && label >= c0 && label < c0 + n) {
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
}

// the workgroup's confusion row.  NC <= CE_CONF_MAX_CLASSES (the caller checked): at least CE_CONF_WORDS / NC >= 1 label rows per pass
__device__ __forceinline__ void ce_confusion_row(const CeArgs& a, const CeLane& r, int am, int* hist) {
    const int tid = threadIdx.x, NC = a.NC;
    const long label = r.label;
    int* crow = a.cslab + (long)blockIdx.x * NC * NC;
    const int per = CE_CONF_WORDS / NC;
    for (int l0 = 0; l0 < NC; l0 += per) {
        const int n = (NC - l0 < per ? NC - l0 : per) * NC;   // words of this pass: label rows l0 .. of the matrix
        for (int i = tid; i < n; i += 256) hist[i] = 0;
        __syncthreads();
        if (r.counts && label >= l0 && (int)(label - l0) * NC < n) atomicAdd(&hist[(int)(label - l0) * NC + am], 1);
        __syncthreads();
        for (int i = tid; i < n; i += 256) crow[l0 * NC + i] = hist[i];
        __syncthreads();
    }
}

template <int NR, bool WRITE, bool WEIGHTED>
__global__ __launch_bounds__(256) void ce_fwd_kernel(CeArgs a) {
    __shared__ int hist[2 * CE_CHUNK];
    __shared__ int cnt[4];
    __shared__ float wsum[4], wwsum[4];
    const int tid = threadIdx.x;
    if (tid < 4) cnt[tid] = 0;
    const CeLane r = ce_lane(a);
    float loss = 0.f, wrow = 0.f;
    int am = 0;
    if (r.on) {
        if constexpr (WEIGHTED) loss = ce_row_weighted<NR, WRITE>(a, r, am, wrow);
        else loss = ce_row_unweighted<NR, WRITE>(a, r, am);
    }
    const bool hit = r.counts && am == (int)r.label;
    const bool nonfin = r.counts && !(fabsf(loss) <= 3.402823466e38f);   // NaN or +-inf
    // the workgroup's partials, in one order: lanes of a wave by butterfly, then the waves in order
    float ls = loss, ws = wrow;
    if constexpr (WEIGHTED) ce_wave_sum(ls, ws);
    else ce_wave_sum(ls);
    if ((tid & 63) == 0) {
        wsum[tid >> 6] = ls;
        if constexpr (WEIGHTED) wwsum[tid >> 6] = ws;
    }
    __syncthreads();   // cnt zeroed, wsum / wwsum written
    ce_count_row(a, r, hit, nonfin, hist, cnt);
    if (a.cslab) ce_confusion_row(a, r, am, hist);
    // the four counts go last: stored right behind the histogram passes, every instance takes 64 VGPRs or more (the scheduler then
    // hoists the 16 LDS reads of the unrolled copy loops) and three weighted ones fall from 8 waves per SIMD to 7
    if (tid < 4) a.slab[(long)blockIdx.x * (4 + 2L * a.NC) + tid] = cnt[tid];
    if (tid == 0) {
        a.partial[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
        if constexpr (WEIGHTED) a.wpartial[blockIdx.x] = (wwsum[0] + wwsum[1]) + (wwsum[2] + wwsum[3]);
    }
}

// one wave per slab column (4 + 2 NC columns, G rows) -> int64 record slot 1 + col
__device__ __forceinline__ void ce_record_column(const CeArgs& a, int G, long cols, long col) {
    const int tid = threadIdx.x;
    if (col >= cols) return;
    long s = 0;
    for (int i = tid & 63; i < G; i += 64) s += a.slab[(long)i * cols + col];
    ce_wave_sum(s);
    if ((tid & 63) == 0) a.record[1 + col] = s;
}

// workgroup 0: loss sum and denominator; workgroups 1 .. RB: the record columns; the rest (launched with a confusion slab only): a
// lane per confusion column (adjacent lanes on adjacent columns of a slab row).  WEIGHTED is a template argument: worked out from
// a.w and a.eps in workgroup 0, it cost a second round of scalar loads there and the kernel 0.2 us
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void ce_finish_kernel(CeArgs a, int G, int RB) {
    __shared__ double red[256], dred[256];
    const int tid = threadIdx.x;
    const long cols = 4 + 2L * a.NC;
    if (blockIdx.x == 0) {
        double s = 0.0, w = 0.0;
        for (int i = tid; i < G; i += 256) {
            s += (double)a.partial[i];
            w += WEIGHTED ? (double)a.wpartial[i] : (double)a.slab[(long)i * cols];   // unweighted: n_valid, exact
        }
        red[tid] = s;
        dred[tid] = w;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) { red[tid] += red[tid + o]; dred[tid] += dred[tid + o]; }
            __syncthreads();
        }
        if (tid == 0) {
            reinterpret_cast<double*>(a.record)[0] = red[0];
            if (a.sums) { a.sums[0] = red[0]; a.sums[1] = dred[0]; }
            *a.loss = dred[0] > 0.0 ? (float)(red[0] / dred[0]) : __int_as_float(0x7fc00000);
        }
        return;
    }
    if ((int)blockIdx.x <= RB) {
        ce_record_column(a, G, cols, ((long)blockIdx.x - 1) * 4 + (tid >> 6));
        return;
    }
    const long cc = (long)a.NC * a.NC;
    const long col = ((long)blockIdx.x - 1 - RB) * 256 + tid;
    if (col >= cc) return;
    long s = 0;
    for (int i = 0; i < G; ++i) s += a.cslab[(long)i * cc + col];
    a.confusion[col] = s;
}

// Den: int64_t (the record: den[1] = n_valid) or double (sums: den[1] = the sum of w[label])
template <bool VEC, class Den>
__global__ __launch_bounds__(256) void ce_bwd_kernel(const float* d, const Den* den, const float* gout, float* dl, long n) {
    const Den ws = den[1];
    const float inv = ws > 0 ? 1.0f / (float)ws : 0.f;   // nothing counts, or only rows of weight 0: d's part in the gradient is zero
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

// f(std::integral_constant<int, NR>) for the register bucket of NC (0: the row is re-read)
template <class F>
void ce_dispatch_nr(int NC, F&& f) {
    if (NC <= 8) f(std::integral_constant<int, 8>{});
    else if (NC <= 16) f(std::integral_constant<int, 16>{});
    else if (NC <= 32) f(std::integral_constant<int, 32>{});
    else f(std::integral_constant<int, 0>{});
}

template <int NR, bool WRITE>
void ce_fwd_launch(const CeArgs& a, int G, hipStream_t st) {
    if (ce_weighted(a)) hipLaunchKernelGGL((ce_fwd_kernel<NR, WRITE, true>), dim3(G), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((ce_fwd_kernel<NR, WRITE, false>), dim3(G), dim3(256), 0, st, a);
}

template <class Den>
int ce_bwd_launch(const float* d, const Den* den, const float* gout, float* dlogits, long n, hipStream_t st) {
    ProfScope ps(K_CE, st);
    const bool vec = n % 4 == 0 && ((uintptr_t)d % 16) == 0 && ((uintptr_t)dlogits % 16) == 0;
    long g = ((vec ? n / 4 : n) + 255) / 256;
    if (g > 2048) g = 2048;
    if (vec) hipLaunchKernelGGL((ce_bwd_kernel<true, Den>), dim3((unsigned)g), dim3(256), 0, st, d, den, gout, dlogits, n);
    else hipLaunchKernelGGL((ce_bwd_kernel<false, Den>), dim3((unsigned)g), dim3(256), 0, st, d, den, gout, dlogits, n);
    return (int)hipGetLastError();
}

}  // namespace

static_assert(CE_CONF_MAX_CLASSES <= CE_CONF_WORDS, "a confusion pass holds at least one label row");

int ce_workgroups(long rows) { return (int)((rows + 255) / 256); }

int launch_ce_fwd(const CeArgs& a, hipStream_t st) {
    const int G = ce_workgroups(a.rows);
    ProfScope ps(K_CE, st);
    ce_dispatch_nr(a.NC, [&](auto nr) {
        constexpr int NR = decltype(nr)::value;
        if (a.d) ce_fwd_launch<NR, true>(a, G, st);
        else ce_fwd_launch<NR, false>(a, G, st);
    });
    return (int)hipGetLastError();
}

int launch_ce_finish(const CeArgs& a, hipStream_t st) {
    const int G = ce_workgroups(a.rows);
    const long cols = 4 + 2L * a.NC;
    const int RB = (int)((cols + 3) / 4);
    const long CB = a.cslab ? ((long)a.NC * a.NC + 255) / 256 : 0;
    ProfScope ps(K_CE, st);
    if (ce_weighted(a)) hipLaunchKernelGGL(ce_finish_kernel<true>, dim3((unsigned)(1 + RB + CB)), dim3(256), 0, st, a, G, RB);
    else hipLaunchKernelGGL(ce_finish_kernel<false>, dim3((unsigned)(1 + RB + CB)), dim3(256), 0, st, a, G, RB);
    return (int)hipGetLastError();
}

int launch_ce_bwd(const float* d, const int64_t* record, const float* gout, float* dlogits, long n, hipStream_t st) {
    return ce_bwd_launch(d, record, gout, dlogits, n, st);
}

int launch_ce_ext_bwd(const float* d, const double* sums, const float* gout, float* dlogits, long n, hipStream_t st) {
    return ce_bwd_launch(d, sums, gout, dlogits, n, st);
}

}  // namespace msst
