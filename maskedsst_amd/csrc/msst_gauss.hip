// Class-conditional Gaussian scores of frozen per-pixel features (msst_gauss_score; maskedsst_amd/gaussian.py): for every row of
// x [Q][96], or of an encode_scene map [Bs][96][plane] read in place, the squared Mahalanobis distance to every class, the log joint
// density, its argmax under the one total order, and the distance to that class.  fp32, no atomics; a row's outputs have the same
// bits whatever batch or layout it sits in, with or without the scores output.
//
// The table form (one kernel for full and tied covariances; nothing says which):  T <= nc tables, each a centre [96] and A_t [96][96];
// per class a table id, an offset m_c [96] in the table's whitened coordinates and a constant.
//     z_t = A_t (x - centre_t)          the subtraction in fp32 first (feat_centre_*), then the fmaf chain over d = 0 .. 95 (feat_scores)
//     zz  = |z_t|^2                     the lane's own 6 entries ascending by fmaf, then the 16 lanes of the group (feat_group_sum)
//     dot = z_t . m_c                   the fmaf chain over j = 0 .. 95 from zero (feat_scores again: the class stage runs on the matrix
//                                       cores against the offsets of the table's classes, 16 classes a tile)
//     d2_c = max((zz + |m_c|^2) - 2 dot, 0),  |m_c|^2 the fmaf chain over j from zero;   score_c = fmaf(-0.5, d2_c, const_c)
// Every order depends on nothing but 96.  Full covariances: T = nc, m = 0, so d2_c = zz exactly.
//
// gauss_score  grid = workgroups of whole 64-row tiles (feat_partition), 256 threads = 4 waves, walked in blocks of R tiles (R = 2; 1
//             where a table owns more than 16 of more than 64 classes).  The loops are  block { table { tile } }: a table is read from
//             L2 once per block, not once per tile -- and with one table (T = 1) once per workgroup: it, its centre and the offsets
//             of its classes are stored before the first block and stay.
//   registers   the block's R raw tiles (24 floats a thread each) and the next block's, fetched while this one is computed; the next
//               table (9 f32x4 a thread), fetched while this one is used.
//   LDS         A_t [96][98] | work [64][98] | the offsets of the table's classes [16 NCTC][98] | d2, then scores [R][64][16 NCT + 1] |
//               centre [96] | |m|^2 [128] | consts [128] | the class order [128] | flags [R][64].  78 KB at 16 classes, 134 KB at 128 full,
//               145 KB at 128 tied.  One workgroup per CU at every size: about 350 registers a thread (256 VGPRs and 92 .. 129 AGPRs)
//               leave one wave per SIMD, so at 16 classes the registers, not the LDS, decide it.
//   work        the centred tile, then -- a wave reads and writes only its own 16 rows -- z in its place, the A operand of the class stage.
//   end         16 lanes per row walk the row's d2 in class order, write the scores in their place and keep the first under the order
//               (feat_ahead, feat_group_argmax); the lane that owns the winner writes the class (-1: a channel not finite, -2: farther
//               than max_d2) and the distance; feat_store_table writes the scores as rows or as a map.
// No inline assembly.
#include "../../include/msst.h"
#include "msst_feat.h"
#include "msst_kernels.h"

namespace msst {

namespace {

constexpr int GS_P = 98;                         // LDS pitch of a feature row, a table row and an offset row
constexpr int GS_TAB_PIECES = FEAT_D * 24 / 256; // 9: 16-byte pieces of a table per thread

// the LDS of gauss_score_kernel<NCT, NCTC>, offsets in floats
template <int NCT, int NCTC>
struct GaussLds {
    static constexpr int R = (NCT == 8 && NCTC == 8) ? 1 : 2;   // row tiles per block: what 160 KB allows
    static constexpr int LP = 16 * NCT + 1;                     // pitch of a d2 row
    static constexpr int tab = 0;                               // [96][GS_P]
    static constexpr int work = tab + FEAT_D * GS_P;            // [64][GS_P]
    static constexpr int off = work + 64 * GS_P;                // [16 NCTC][GS_P]
    static constexpr int d2 = off + 16 * NCTC * GS_P;           // [R][64][LP]
    static constexpr int cen = d2 + R * 64 * LP;                // [96]
    static constexpr int mm = cen + FEAT_D;                     // [128]
    static constexpr int cst = mm + 128;                        // [128]
    static constexpr int perm = cst + 128;                      // [128] int
    static constexpr int flag = perm + 128;                     // [R][64] int
    static constexpr size_t bytes = (size_t)4 * (flag + R * 64);
    static_assert(cen % 4 == 0, "the centre is read 16 bytes at a time");
    static_assert(bytes <= 160 * 1024, "the LDS of a CU");
};

struct GaussArgs {
    const float* x;
    const float* centres;   // [T][96]
    const float* tables;    // [T][96][96]
    const float* offsets;   // [nc][96]
    const float* consts;    // [nc]
    int32_t* classes;       // [rows]
    float* distance;        // [rows]
    float* scores;          // null: not wanted
    long rows, plane, tiles_per_wg;
    int nc, T, x_layout, out_layout;
    float max_d2;
    unsigned char perm[128];    // the classes ordered by table, ascending inside a table
    unsigned char first[129];   // table t owns perm[first[t] .. first[t + 1])
};

__device__ __forceinline__ void gauss_table_prefetch(f32x4 (&an)[GS_TAB_PIECES], const float* tables, int t, int tid) {
    const f32x4* src = reinterpret_cast<const f32x4*>(tables + (long)t * FEAT_D * FEAT_D);
#pragma unroll
    for (int i = 0; i < GS_TAB_PIECES; ++i) an[i] = src[tid + 256 * i];
}

__device__ __forceinline__ void gauss_table_store(float* stab, const f32x4 (&an)[GS_TAB_PIECES], int tid) {
#pragma unroll
    for (int i = 0; i < GS_TAB_PIECES; ++i) {
        const int e = tid + 256 * i;
        const int row = e / 24, c4 = e - row * 24;
        float* d = stab + row * GS_P + 4 * c4;
        *reinterpret_cast<float2*>(d) = make_float2(an[i][0], an[i][1]);
        *reinterpret_cast<float2*>(d + 2) = make_float2(an[i][2], an[i][3]);
    }
}

template <int NCT, int NCTC>
__global__ __launch_bounds__(256, 1) void gauss_score_kernel(GaussArgs a) {
    using L = GaussLds<NCT, NCTC>;
    constexpr int R = L::R, LP = L::LP;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float* smem = reinterpret_cast<float*>(smem_raw);
    float *stab = smem + L::tab, *work = smem + L::work, *soff = smem + L::off, *sd2 = smem + L::d2, *scen = smem + L::cen;
    float *smm = smem + L::mm, *scst = smem + L::cst;
    int *sperm = reinterpret_cast<int*>(smem + L::perm), *sflag = reinterpret_cast<int*>(smem + L::flag);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cg = lane >> 4, cc = lane & 15;
    const int nc = a.nc;

    // ---- once: the class order, the constants and |m_c|^2
    if (tid < 128) {
        float mm = 0.f;
        if (tid < nc) {
            const float* m = a.offsets + tid * FEAT_D;
#pragma unroll 8
            for (int d = 0; d < FEAT_D; ++d) mm = fmaf(m[d], m[d], mm);
        }
        smm[tid] = mm;
        scst[tid] = tid < nc ? a.consts[tid] : -__builtin_inff();
        sperm[tid] = tid < nc ? (int)a.perm[tid] : 0;
    }

    const long rbeg = (long)blockIdx.x * a.tiles_per_wg * 64;
    const long rend = min(a.rows, rbeg + a.tiles_per_wg * 64);
    const long ntiles = rend > rbeg ? (rend - rbeg + 63) / 64 : 0;
    const long nblocks = (ntiles + R - 1) / R;

    f32x4 raw[R][6], nxt[R][6];
    auto load_block = [&](f32x4 (&dst)[R][6], long b0) {   // a tile past rend comes as zeros
#pragma unroll
        for (int i = 0; i < R; ++i) {
            if (a.x_layout == 0) feat_rows_prefetch(dst[i], a.x, b0 + 64 * i, rend, tid);
            else feat_map_prefetch(dst[i], a.x, a.plane, b0 + 64 * i, rend, tid);
        }
    };
    if (nblocks > 0) load_block(raw, rbeg);
    f32x4 an[GS_TAB_PIECES];

    for (long blk = 0; blk < nblocks; ++blk) {
        const long b0 = rbeg + blk * R * 64;
        if (blk + 1 < nblocks) load_block(nxt, b0 + R * 64);
        const bool fill = a.T > 1 || blk == 0;   // uniform.  One table: it, its centre and its offsets stay in LDS for the whole walk
        if (fill) gauss_table_prefetch(an, a.tables, 0, tid);

        for (int t = 0; t < a.T; ++t) {
            const int c0 = a.first[t], ncls = a.first[t + 1] - c0;
            __syncthreads();   // the table before (and, first, the block before) is done with
            if (fill) {
                gauss_table_store(stab, an, tid);
                if (tid < FEAT_D) scen[tid] = a.centres[t * FEAT_D + tid];
                for (int e = tid; e < 16 * NCTC * FEAT_D; e += 256) {
                    const int j = e / FEAT_D, d = e - j * FEAT_D;
                    soff[j * GS_P + d] = j < ncls ? a.offsets[sperm[c0 + j] * FEAT_D + d] : 0.f;
                }
            }
            if (t + 1 < a.T) gauss_table_prefetch(an, a.tables, t + 1, tid);
            __syncthreads();

#pragma unroll
            for (int i = 0; i < R; ++i) {
                const long r0 = b0 + 64 * i;
                if (r0 < rend) {   // uniform
                    f32x4 c[6];
#pragma unroll
                    for (int k = 0; k < 6; ++k) c[k] = raw[i][k];
                    if (a.x_layout == 0) {
                        feat_centre_rows(c, scen, tid);
                        feat_rows_store<GS_P>(work, c, tid);
                    } else {
                        feat_centre_map(c, scen, tid);
                        feat_map_store<GS_P>(work, c, tid);
                    }
                    __syncthreads();
                    feat_flag_rows<GS_P>(work, sflag + 64 * i, r0, rend, tid);
                    __syncthreads();
                    // ---- z = A_t (x - centre_t): the wave's 16 rows x 96
                    f32x4 z[6];
#pragma unroll
                    for (int jt = 0; jt < 6; ++jt) z[jt] = zero4();
                    feat_scores<6, GS_P, GS_P>(work, stab, wave, cc, cg, z);
                    float zz[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float ss = 0.f;
#pragma unroll
                        for (int jt = 0; jt < 6; ++jt) ss = fmaf(z[jt][r], z[jt][r], ss);
                        zz[r] = feat_group_sum(ss);
                    }
                    __syncthreads();   // (a wave reads and writes its own 16 rows only)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
#pragma unroll
                        for (int jt = 0; jt < 6; ++jt) work[(16 * wave + 4 * cg + r) * GS_P + 16 * jt + cc] = z[jt][r];
                    }
                    __syncthreads();
                    // ---- the class stage: z . m_c for the table's classes
                    f32x4 acc[NCTC];
#pragma unroll
                    for (int jt = 0; jt < NCTC; ++jt) acc[jt] = zero4();
                    feat_scores<NCTC, GS_P, GS_P>(work, soff, wave, cc, cg, acc);
                    float* tab = sd2 + i * 64 * LP;
#pragma unroll
                    for (int jt = 0; jt < NCTC; ++jt) {
                        const int j = 16 * jt + cc;
                        if (j < ncls) {
                            const int cls = sperm[c0 + j];
                            const float mm = smm[cls];
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                tab[(16 * wave + 4 * cg + r) * LP + cls] = fmaxf((zz[r] + mm) - 2.f * acc[jt][r], 0.f);
                        }
                    }
                    __syncthreads();   // work is free for the next tile
                }
            }
        }

        // ---- the block's rows: scores in place of d2, the first class under the order, the distance to it
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const long r0 = b0 + 64 * i;
            if (r0 < rend) {   // uniform
                const long nq = min((long)64, rend - r0);
                float* tab = sd2 + i * 64 * LP;
#pragma unroll
                for (int pass = 0; pass < 4; ++pass) {
                    const int rl = 16 * pass + (tid >> 4);
                    const bool bad = sflag[64 * i + rl] == 1;
                    float bv = -__builtin_inff(), bd = 0.f;
                    int bi = 0x7fffffff;
                    for (int cls = cc; cls < nc; cls += 16) {
                        const float d = tab[rl * LP + cls];
                        const float s = bad ? __builtin_nanf("") : fmaf(-0.5f, d, scst[cls]);
                        tab[rl * LP + cls] = s;
                        if (feat_ahead(s, cls, bv, bi)) { bv = s; bi = cls; bd = d; }
                    }
                    const int own = bi;
                    feat_group_argmax(bv, bi);
                    if (rl < nq && (bad ? cc == 0 : own == bi)) {
                        a.classes[r0 + rl] = bad ? -1 : bd > a.max_d2 ? -2 : bi;
                        a.distance[r0 + rl] = bad ? __builtin_nanf("") : bd;
                    }
                }
                if (a.scores) {   // uniform
                    __syncthreads();
                    feat_store_table<256>(tab, LP, a.scores, a.out_layout, r0, nq, nc, a.plane, tid);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < R; ++i) {
#pragma unroll
            for (int k = 0; k < 6; ++k) raw[i][k] = nxt[i][k];
        }
    }
}

template <int NCT, int NCTC>
int gauss_score_launch(GaussArgs& a, hipStream_t st) {
    constexpr size_t lds = GaussLds<NCT, NCTC>::bytes;
    if (int e = feat_allow_lds<&gauss_score_kernel<NCT, NCTC>>(lds)) return e;
    int nwg;
    feat_partition(a.rows, &a.tiles_per_wg, &nwg);
    hipLaunchKernelGGL((gauss_score_kernel<NCT, NCTC>), dim3((unsigned)nwg), dim3(256), lds, st, a);
    return (int)hipGetLastError();
}

}  // namespace

int launch_gauss_score(const float* x, int x_layout, long rows, long plane, const float* centres, const float* tables, int n_tables,
                       const int32_t* class_table, const float* offsets, const float* consts, int nc, float max_d2, int32_t* classes,
                       float* distance, float* scores, int out_layout, hipStream_t st) {
    GaussArgs a;
    a.x = x; a.centres = centres; a.tables = tables; a.offsets = offsets; a.consts = consts; a.classes = classes; a.distance = distance;
    a.scores = scores; a.rows = rows; a.plane = plane; a.nc = nc; a.T = n_tables; a.x_layout = x_layout; a.out_layout = out_layout;
    a.max_d2 = max_d2;
    // the classes ordered by table (the caller has checked the ids): a counting sort, stable
    int count[129] = {0};
    for (int c = 0; c < nc; ++c) ++count[class_table[c] + 1];
    int most = 0;
    for (int t = 0; t < n_tables; ++t) {
        most = count[t + 1] > most ? count[t + 1] : most;
        count[t + 1] += count[t];
    }
    for (int t = 0; t <= 128; ++t) a.first[t] = (unsigned char)(t <= n_tables ? count[t] : nc);
    for (int c = 0; c < 128; ++c) a.perm[c] = 0;
    for (int c = 0; c < nc; ++c) a.perm[count[class_table[c]]++] = (unsigned char)c;
    // a table with at most 16 classes needs one tile of offsets; otherwise room for all the classes
    const bool one = most <= 16;
    switch (feat_nct(nc)) {
        case 1: return gauss_score_launch<1, 1>(a, st);
        case 2: return one ? gauss_score_launch<2, 1>(a, st) : gauss_score_launch<2, 2>(a, st);
        case 4: return one ? gauss_score_launch<4, 1>(a, st) : gauss_score_launch<4, 4>(a, st);
        default: return one ? gauss_score_launch<8, 1>(a, st) : gauss_score_launch<8, 8>(a, st);
    }
}

}  // namespace msst
