// kNN evaluation of frozen per-pixel features (msst_knn_topk, msst_knn_vote; maskedsst_amd/knn.py): for every query the k bank
// rows of largest similarity s(q, m) = sum_d q[d] bank[m][d] (d = 0 .. 95) under ONE total order -- similarity descending, then bank
// index ascending -- and the weighted vote of their labels.  No Q x M score matrix and no permuted copy of an encode_scene map
// exist; no atomics; every output has the same bits for every `splits`, every run and every batch a query sits in.
//
// knn_topk    grid (query tiles of 64, bank slices), 256 threads = 4 waves, LDS 25,088 + 512 k bytes (k = 20: 35 KB, four
//             workgroups per CU; k = 64: 57 KB, two) -- two or more waves per SIMD cover the 40-cycle dependent MFMA latency on
//             top of the four independent accumulators of a wave.
//   queries   wave w owns queries 16 w .. 16 w + 15 of the tile as the A operand of v_mfma_f32_16x16x4_f32: lane l holds
//             q[l & 15][4 ks + (l >> 4)] for the 24 k-steps in 24 registers, loaded once -- layout 0 from rows [Q][96], layout 1
//             straight from the map [Bs][96][plane] (query b plane + p reads (b 96 + d) plane + p: the 16 lanes of a k-slice
//             read 16 adjacent pixels).  Rows past Q read as zero and are never stored.
//   bank      the slice is walked in tiles of 64 rows with the rows-layout tile loader of msst_feat.h (one tile ahead in registers,
//             LDS [64][98]); rows past the slice's end are zero and masked by index below.
//   scores    per tile 24 k-steps x 4 column tiles: c[jt] = mma(q_ks, bank[16 jt + (l & 15)][4 ks + (l >> 4)], c[jt]), ks
//             ascending from a zero accumulator, so s(q, m) is the fp32 fmaf chain over d = 0 .. 95 in order whatever tile,
//             wave, workgroup or slice the pair lands in.  Lane l then holds s for queries 4 (l >> 4) + r, bank rows 16 jt + (l & 15).
//   select    per query a sorted list of k (similarity, index) pairs in LDS, entry j on lane j.  A lane tests its 16 scores
//             against the k-th entries of its four queries (kept in registers, refreshed after a tile that inserted); the
//             rare passers are inserted one at a time by the whole wave: position = number of entries ahead of the candidate
//             (one ballot), entries behind it move down one lane (a shuffle), the last one falls off.  A candidate is compared
//             under the total order, so the list does not depend on the order in which candidates arrive.  A NaN score (a query
//             with a NaN channel) passes no test: the list keeps its initial (-inf, -1) entries, which is also what M < k leaves.
//   output    splits == 1: the lists are the result.  Otherwise slice s writes its list to scratch [s][query][k] and
// knn_merge   one thread per (query, slice, entry) counts the entries of all slices ahead of its own under the same order
//             (absent entries rank last, by slice and place) and stores it at that rank if below k: every output slot is written
//             exactly once, nothing is initialised.  The order is msst_feat.h's feat_ahead.
// knn_vote    64 queries per workgroup, one thread per query: votes in LDS [64][n_classes + 1], w_j = exp((s_j - s_1) / temperature)
//             (temperature 0: 1) added in rank order j = 1 .. k in fp32, argmax with ties to the lowest class (-1 without
//             neighbours); the table is stored by all threads, rows [Q][n_classes] or the map [Bs][n_classes][plane] (msst_feat.h).
// Queries are processed in chunks of 32,768 inside the call (grids stay small, the scratch is one chunk's).
// No inline assembly.
#include "../../include/msst.h"
#include "msst_feat.h"
#include "msst_kernels.h"

namespace msst {

namespace {

constexpr int KNN_BP = 98;             // LDS pitch of a bank row
constexpr long KNN_QCHUNK = 32768;     // queries per launch
constexpr int KNN_MAX_SPLITS = 64;
constexpr int KNN_AUTO_MAX_SPLITS = 32;

// the LDS of knn_topk_kernel, offsets in floats
struct KnnTopkLds {
    static constexpr int bank = 0;                                             // [64][KNN_BP]
    static constexpr int sim = bank + 64 * KNN_BP;                             // [64][k]
    __host__ __device__ static constexpr int idx(int k) { return sim + 64 * k; }   // [64][k] int
    static constexpr size_t bytes(int k) { return (size_t)4 * (idx(k) + 64 * k); }
};

struct KnnTopkArgs {
    const float* bank;
    const float* queries;
    float* out_sim;       // [nq][k] (splits == 1: the result; else scratch [splits][nq][k])
    int32_t* out_idx;
    long M, q0, Q, plane, tiles_per_split;
    int nq, k, q_layout;
};

__global__ __launch_bounds__(256) void knn_topk_kernel(KnnTopkArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float* smem = reinterpret_cast<float*>(smem_raw);
    float *sbank = smem + KnnTopkLds::bank, *lsim = smem + KnnTopkLds::sim;
    int* lidx = reinterpret_cast<int*>(smem + KnnTopkLds::idx(a.k));
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cg = lane >> 4, cc = lane & 15;
    const int k = a.k;
    const int split = blockIdx.y;
    const long mbeg = (long)split * a.tiles_per_split * 64;
    const long mend = min(a.M, mbeg + a.tiles_per_split * 64);
    const long ntiles = mend > mbeg ? (mend - mbeg + 63) / 64 : 0;

    // ---- the wave's queries: A fragments of the 24 k-steps
    float qf[24];
    {
        const long ql = (long)blockIdx.x * 64 + 16 * wave + cc;      // within the chunk
        const long q = a.q0 + ql;
        const bool valid = ql < a.nq;
        const float* src;
        long kstride;
        if (a.q_layout == 0) {
            src = a.queries + q * FEAT_D;
            kstride = 1;
        } else {
            const long b = q / a.plane, p = q - b * a.plane;
            src = a.queries + b * FEAT_D * a.plane + p;
            kstride = a.plane;
        }
#pragma unroll
        for (int ks = 0; ks < 24; ++ks) qf[ks] = valid ? src[(4 * ks + cg) * kstride] : 0.f;
    }
    // ---- the lists of the wave's 16 queries
    for (int e = lane; e < 16 * k; e += 64) {
        lsim[16 * wave * k + e] = -INFINITY;
        lidx[16 * wave * k + e] = -1;
    }
    float thr_s[4];
    int thr_i[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { thr_s[r] = -INFINITY; thr_i[r] = -1; }

    f32x4 pre[6];
    if (ntiles > 0) feat_rows_prefetch(pre, a.bank, mbeg, mend, tid);

    for (long t = 0; t < ntiles; ++t) {
        const long m0 = mbeg + t * 64;
        __syncthreads();   // the previous tile's operand reads are done
        feat_rows_store<KNN_BP>(sbank, pre, tid);
        __syncthreads();
        if (t + 1 < ntiles) feat_rows_prefetch(pre, a.bank, m0 + 64, mend, tid);
        // ---- scores of 16 queries x 64 bank rows
        f32x4 c[4];
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) c[jt] = zero4();
#pragma unroll
        for (int ks = 0; ks < 24; ++ks) {
#pragma unroll
            for (int jt = 0; jt < 4; ++jt)
                c[jt] = PF32::mma(qf[ks], sbank[(16 * jt + cc) * KNN_BP + 4 * ks + cg], c[jt]);
        }
        // ---- candidates that beat the k-th entry of their query
        bool inserted = false;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int jt = 0; jt < 4; ++jt) {
                const float s = c[jt][r];
                const long m = m0 + 16 * jt + cc;
                const bool pass = m < mend && feat_ahead(s, (int)m, thr_s[r], thr_i[r]);
                unsigned long long b = __ballot(pass);
                while (b) {   // wave-uniform
                    const int leader = __ffsll(b) - 1;
                    b &= b - 1;
                    const float cs = __shfl(s, leader);
                    const int ci = (int)(m0 + 16 * jt + (leader & 15));
                    const int row = 16 * wave + 4 * (leader >> 4) + r;
                    float* ls = lsim + row * k;
                    int* li = lidx + row * k;
                    const bool mine = lane < k;
                    const float es = mine ? ls[lane] : 0.f;
                    const int ei = mine ? li[lane] : 0;
                    const int pos = __popcll(__ballot(mine && !feat_ahead(cs, ci, es, ei)));   // entries ahead: a prefix of the sorted list
                    if (pos >= k) continue;
                    const float ps = __shfl_up(es, 1);
                    const int pi = __shfl_up(ei, 1);
                    if (mine && lane >= pos) {
                        ls[lane] = lane == pos ? cs : ps;
                        li[lane] = lane == pos ? ci : pi;
                    }
                    inserted = true;
                }
            }
        }
        if (inserted) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                thr_s[r] = lsim[(16 * wave + 4 * cg + r) * k + k - 1];
                thr_i[r] = lidx[(16 * wave + 4 * cg + r) * k + k - 1];
            }
        }
    }
    // ---- the wave's lists: consecutive lanes on consecutive floats of the 16 k outputs
    __syncthreads();   // (an empty slice: the initial entries were written by other lanes)
    {
        const long ql0 = (long)blockIdx.x * 64 + 16 * wave;
        const long rows = min((long)16, a.nq - ql0);
        const long base = ((long)split * a.nq + ql0) * k;
        for (long e = lane; e < rows * k; e += 64) {
            a.out_sim[base + e] = lsim[16 * wave * k + e];
            a.out_idx[base + e] = lidx[16 * wave * k + e];
        }
    }
}

struct KnnMergeArgs {
    const float* part_sim;   // [splits][nq][k]
    const int32_t* part_idx;
    float* out_sim;          // [nq][k]
    int32_t* out_idx;
    int nq, k, splits;
};

__global__ __launch_bounds__(256) void knn_merge_kernel(KnnMergeArgs a) {
    const int per = a.splits * a.k;
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= (long)a.nq * per) return;
    const long q = g / per;
    const int e = (int)(g - q * per);
    const int sp = e / a.k, j = e - sp * a.k;
    const float s = a.part_sim[((long)sp * a.nq + q) * a.k + j];
    const int i = a.part_idx[((long)sp * a.nq + q) * a.k + j];
    int rank = 0;
    for (int s2 = 0; s2 < a.splits; ++s2) {
        const float* ps = a.part_sim + ((long)s2 * a.nq + q) * a.k;
        const int32_t* pi = a.part_idx + ((long)s2 * a.nq + q) * a.k;
        for (int j2 = 0; j2 < a.k; ++j2) {
            const float es = ps[j2];
            const int ei = pi[j2];
            const int e2 = s2 * a.k + j2;
            bool ahead;
            if (ei < 0) ahead = i < 0 && e2 < e;       // absent entries rank last, by slice and place
            else ahead = i < 0 || feat_ahead(es, ei, s, i);
            rank += ahead ? 1 : 0;
        }
    }
    if (rank < a.k) {
        a.out_sim[q * a.k + rank] = i < 0 ? -INFINITY : s;
        a.out_idx[q * a.k + rank] = i < 0 ? -1 : i;
    }
}

struct KnnVoteArgs {
    const int32_t* nbr_idx;
    const float* nbr_sim;
    const int32_t* labels;
    float* votes;
    int64_t* classes;
    long Q, plane;
    float temperature;
    int k, nc, vote_layout;
};

__global__ __launch_bounds__(64) void knn_vote_kernel(KnnVoteArgs a) {
    __shared__ float sv[64 * 129];
    const int tid = threadIdx.x;
    const int nc = a.nc, pitch = nc + 1;
    const long q0 = (long)blockIdx.x * 64;
    const long q = q0 + tid;
    float* v = sv + tid * pitch;
    for (int c = 0; c < nc; ++c) v[c] = 0.f;
    if (q < a.Q) {
        const int32_t* ni = a.nbr_idx + q * a.k;
        const float* ns = a.nbr_sim + q * a.k;
        const float s1 = ns[0];
        bool any = false;
        for (int j = 0; j < a.k; ++j) {
            const int m = ni[j];
            if (m < 0) break;
            any = true;
            const int c = a.labels[m];
            const float w = a.temperature > 0.f ? expf((ns[j] - s1) / a.temperature) : 1.0f;
            if ((unsigned)c < (unsigned)nc) v[c] += w;   // a label outside [0, n_classes) votes for nothing
        }
        int best = -1;
        if (any) {
            best = 0;
            float bv = v[0];
            for (int c = 1; c < nc; ++c)
                if (v[c] > bv) { bv = v[c]; best = c; }
        }
        a.classes[q] = best;
    }
    __syncthreads();
    const long nq = min((long)64, a.Q - q0);
    feat_store_table<64>(sv, pitch, a.votes, a.vote_layout, q0, nq, nc, a.plane, tid);
}

int knn_splits_for(long nq, long M, int splits) {
    const long mtiles = (M + 63) / 64;
    long s = splits;
    if (s <= 0) {
        const long qtiles = (nq + 63) / 64;
        s = (FEAT_MAX_WGS + qtiles - 1) / qtiles;
        if (s > KNN_AUTO_MAX_SPLITS) s = KNN_AUTO_MAX_SPLITS;
    }
    if (s > mtiles) s = mtiles;   // a slice is whole tiles; more slices than tiles would be empty ones
    return (int)(s < 1 ? 1 : s);
}

}  // namespace

long knn_scratch_bytes(long Q, long M, int k, int splits) {
    (void)M;
    const long nq = Q < KNN_QCHUNK ? Q : KNN_QCHUNK;
    if (splits == 1) return 0;
    // splits = 0: the automatic choice takes at most ceil(512 / ceil(nq / 64)) <= 512 * 64 / nq + 1 slices, so nq + 32768 rows hold it
    const long rows = splits > 0 ? nq * splits : nq + FEAT_MAX_WGS * 64;
    return rows * k * 8;
}

int launch_knn_topk(const float* bank, long M, const float* queries, int q_layout, long Q, long plane, int k, int splits,
                    int32_t* nbr_idx, float* nbr_sim, void* scratch, hipStream_t st) {
    const size_t lds = KnnTopkLds::bytes(k);
    for (long q0 = 0; q0 < Q; q0 += KNN_QCHUNK) {
        const int nq = (int)(Q - q0 < KNN_QCHUNK ? Q - q0 : KNN_QCHUNK);
        const int sp = knn_splits_for(nq, M, splits);
        const long mtiles = (M + 63) / 64;
        KnnTopkArgs a;
        a.bank = bank; a.queries = queries; a.M = M; a.q0 = q0; a.Q = Q; a.plane = plane;
        a.tiles_per_split = (mtiles + sp - 1) / sp;
        a.nq = nq; a.k = k; a.q_layout = q_layout;
        float* part_sim = reinterpret_cast<float*>(scratch);
        int32_t* part_idx = reinterpret_cast<int32_t*>(part_sim + (long)sp * nq * k);
        a.out_sim = sp == 1 ? nbr_sim + q0 * k : part_sim;
        a.out_idx = sp == 1 ? nbr_idx + q0 * k : part_idx;
        hipLaunchKernelGGL(knn_topk_kernel, dim3((unsigned)((nq + 63) / 64), (unsigned)sp), dim3(256), lds, st, a);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
        if (sp > 1) {
            KnnMergeArgs m;
            m.part_sim = part_sim; m.part_idx = part_idx; m.out_sim = nbr_sim + q0 * k; m.out_idx = nbr_idx + q0 * k;
            m.nq = nq; m.k = k; m.splits = sp;
            const long threads = (long)nq * sp * k;
            hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, m);
            e = hipGetLastError();
            if (e != hipSuccess) return (int)e;
        }
    }
    return 0;
}

int launch_knn_vote(const int32_t* nbr_idx, const float* nbr_sim, const int32_t* labels, long Q, int k, int n_classes,
                    float temperature, float* votes, int vote_layout, long plane, int64_t* classes, hipStream_t st) {
    KnnVoteArgs a;
    a.nbr_idx = nbr_idx; a.nbr_sim = nbr_sim; a.labels = labels; a.votes = votes; a.classes = classes;
    a.Q = Q; a.plane = plane; a.temperature = temperature; a.k = k; a.nc = n_classes; a.vote_layout = vote_layout;
    hipLaunchKernelGGL(knn_vote_kernel, dim3((unsigned)((Q + 63) / 64)), dim3(64), 0, st, a);
    return (int)hipGetLastError();
}

}  // namespace msst
