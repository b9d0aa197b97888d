// SimMIM masks drawn on the device (msst_draw_masks): the token mask, the gather indices and the token-CSR of the gather for rows
// row0 .. row0 + rows - 1 of a conceptually unbounded global batch, in one launch, one workgroup of 256 threads per row.
//
// Randomness   32-bit keys from a stateless counter hash (the style of drop_bits, msst_dev.h) of (seed, stream, global row, spectral
//             block, element): two row words ra, rb = three murmur finalisers each over (seed ^ (2 stream + salt + 1) golden, row low
//             word, row high word); key = the finaliser of ((block << 12) | element) ^ ra with rb added after its first round.  Every
//             step is a bijection of the counter, so the keys of one (row, stream) are distinct.  stream = mode + 1.  Nothing depends
//             on row0, rows or the launch geometry.  Selection is always "the m elements with the smallest (key, index) pairs".
// Modes        TOPK: T = S N keys (block 0, element t), the K smallest are masked.  BLOCK: per spectral block c the rand_size^2 cell
//             keys (block c, element cell), the mask_count smallest cells are masked and each cell covers scale x scale positions of
//             the side x side grid.  TUBE: as BLOCK with the one draw (block 0) repeated over the S blocks.
//             A row's mask is held as S words of N bits (bit n of word c = token c N + n).
// Indices      The row-major list of the true columns of the global mask, cut into chunks of K (the reference's
//             bool_mask_to_indices).  Every row holds R trues (TOPK: R = K), so list position K g + k lies in source row
//             q = (K g + k) / R at rank j = (K g + k) % R: an index row is the tail of source row q0 from rank j0 on (lenA entries)
//             followed by the head of row q0 + 1 (K - lenA entries); the workgroup regenerates both rows' words from the counter.
//             The list rank of a true token is base[c] + popcount(word c below bit n), base = the exclusive prefix of the words'
//             popcounts (one thread, ascending c).  Both pieces ascend in the token, so a token occurs at most twice in an index row,
//             and the CSR of the gather is: csr_ptr[t] = the entries with a token below t, csr_pos = per token the position in piece A,
//             then the one in piece B (ascending k).  Tokens are walked in chunks of 256, ascending; inside a chunk the prefix is
//             ballot + popcount per wave and the four wave totals through LDS, added in wave order; integers only.
// Ranking      TOPK: keys in LDS (padded to a multiple of four with (0xFFFFFFFF, index >= T), which no real pair exceeds), every
//             thread counts the pairs below its own against 16-byte broadcast reads.  BLOCK / TUBE: one wave per (row, block), lane =
//             cell, the other cells' keys by lane shuffles.
// No atomics, nothing to zero beforehand, every output element written exactly once and nothing beyond; plain C++ and vector stores.
// Launch bound (a few thousand integer operations per row): it does not appear in a roofline and is not tuned.
#include "msst_dev.h"
#include "msst_kernels.h"

namespace msst {

namespace {

constexpr int MASK_MAX_T = 4096;   // S <= 64, N <= 64

__device__ __forceinline__ unsigned mask_mix(unsigned x) {
    x *= 0x9E3779B1U; x ^= x >> 15;
    x *= 0x85EBCA6BU; x ^= x >> 13;
    x *= 0xC2B2AE35U; x ^= x >> 16;
    return x;
}
__device__ __forceinline__ unsigned mask_row_word(unsigned seed, unsigned stream, unsigned long long row, unsigned salt) {
    unsigned h = mask_mix(seed ^ ((stream * 2U + salt + 1U) * 0x9E3779B9U));
    h = mask_mix(h ^ (unsigned)row);
    return mask_mix(h ^ (unsigned)(row >> 32));
}
__device__ __forceinline__ unsigned mask_key(unsigned ra, unsigned rb, unsigned block, unsigned elem) {
    unsigned x = ((block << 12) | elem) ^ ra;
    x *= 0x9E3779B1U; x ^= x >> 15;
    x += rb;
    x *= 0x85EBCA6BU; x ^= x >> 13;
    x *= 0xC2B2AE35U; x ^= x >> 16;
    return x;
}
__device__ __forceinline__ int pair_below(unsigned kj, int j, unsigned k, int i) { return (kj < k || (kj == k && j < i)) ? 1 : 0; }

__global__ __launch_bounds__(256) void draw_masks_kernel(MaskDrawArgs a) {
    __shared__ uint4 keys4[MASK_MAX_T / 4];
    __shared__ uint8_t flag[MASK_MAX_T];
    __shared__ unsigned long long words[3][64];   // slot 0: this row; slots 1, 2: the source rows of its index row
    __shared__ int base[3][64];
    __shared__ int wave_total[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = a.S, N = a.N, K = a.K, T = S * N;
    const unsigned long long g = (unsigned long long)a.row0 + blockIdx.x;
    const unsigned stream = (unsigned)a.mode + 1U;
    int R, j0, sA, sB, nslots;

    if (a.mode == MSST_MASK_TOPK) {
        unsigned* keys = reinterpret_cast<unsigned*>(keys4);
        const unsigned ra = mask_row_word(a.seed, stream, g, 0), rb = mask_row_word(a.seed, stream, g, 1);
        const int T4 = (T + 3) & ~3;
        for (int t = tid; t < T4; t += 256) keys[t] = t < T ? mask_key(ra, rb, 0, (unsigned)t) : 0xFFFFFFFFU;
        __syncthreads();
        for (int t = tid; t < T; t += 256) {
            const unsigned k = keys[t];
            int below = 0;
            for (int j4 = 0; j4 < T4 / 4; ++j4) {
                const uint4 v = keys4[j4];
                const int j = 4 * j4;
                below += pair_below(v.x, j, k, t) + pair_below(v.y, j + 1, k, t) + pair_below(v.z, j + 2, k, t) + pair_below(v.w, j + 3, k, t);
            }
            flag[t] = below < K ? 1 : 0;
        }
        __syncthreads();
        if (tid < S) {
            unsigned long long w = 0;
            for (int n = 0; n < N; ++n) w |= (unsigned long long)flag[tid * N + n] << n;
            words[0][tid] = w;
        }
        R = K; j0 = 0; sA = sB = 0; nslots = 1;
    } else {
        const int tube = a.mode == MSST_MASK_TUBE;
        const int tc = a.rand_size * a.rand_size, per = a.mask_count * a.scale * a.scale;
        R = S * per;
        const unsigned long long p0 = (unsigned long long)K * g;
        const unsigned long long q0 = p0 / (unsigned)R;
        j0 = (int)(p0 - q0 * (unsigned)R);
        const unsigned long long q1 = (p0 + (unsigned)(K - 1)) / (unsigned)R;   // q0 or q0 + 1 (K <= R)
        sA = 1; sB = 2; nslots = 3;
        const int nblk = tube ? 1 : S;
        for (int job = wave; job < 3 * nblk; job += 4) {   // wave uniform
            const int slot = job / nblk, c = job - slot * nblk;
            const unsigned long long row = slot == 0 ? g : slot == 1 ? q0 : q1;
            const unsigned ra = mask_row_word(a.seed, stream, row, 0), rb = mask_row_word(a.seed, stream, row, 1);
            const unsigned k = mask_key(ra, rb, (unsigned)c, (unsigned)lane);
            int below = 0;
            for (int j = 0; j < tc; ++j) below += pair_below((unsigned)__shfl((int)k, j), j, k, lane);
            const unsigned long long cells = __ballot(lane < tc && below < a.mask_count);
            int on = 0;
            if (lane < N) {
                const int y = lane / a.side, x = lane - y * a.side;
                on = (int)((cells >> ((y / a.scale) * a.rand_size + x / a.scale)) & 1ULL);
            }
            const unsigned long long w = __ballot(on);
            if (tube) {
                if (lane < S) words[slot][lane] = w;
            } else if (lane == 0) {
                words[slot][c] = w;
            }
        }
    }
    __syncthreads();
    if (tid < nslots) {
        int acc = 0;
        for (int c = 0; c < S; ++c) {
            base[tid][c] = acc;
            acc += __popcll(words[tid][c]);
        }
    }
    __syncthreads();

    const int lenA = K < R - j0 ? K : R - j0, lenB = K - lenA;
    uint8_t* mask = a.mask + (long)blockIdx.x * T;
    int32_t* idx = a.idx + (long)blockIdx.x * K;
    int32_t* ptr = a.csr_ptr + (long)blockIdx.x * (T + 1);
    int32_t* pos = a.csr_pos + (long)blockIdx.x * K;
    const unsigned long long lanes_below = (1ULL << lane) - 1ULL;
    int run = 0;
    for (int t0 = 0; t0 < T; t0 += 256) {   // workgroup uniform
        const int t = t0 + tid;
        int inA = 0, inB = 0, kA = 0, kB = 0;
        if (t < T) {
            const int c = t / N, n = t - c * N;
            const unsigned long long below = (1ULL << n) - 1ULL;
            mask[t] = (uint8_t)((words[0][c] >> n) & 1ULL);
            const unsigned long long wA = words[sA][c];
            if ((wA >> n) & 1ULL) {
                const int r = base[sA][c] + __popcll(wA & below);
                if (r >= j0 && r - j0 < lenA) { inA = 1; kA = r - j0; }
            }
            if (lenB > 0) {
                const unsigned long long wB = words[sB][c];
                if ((wB >> n) & 1ULL) {
                    const int r = base[sB][c] + __popcll(wB & below);
                    if (r < lenB) { inB = 1; kB = lenA + r; }
                }
            }
        }
        const unsigned long long bA = __ballot(inA), bB = __ballot(inB);
        if (lane == 0) wave_total[wave] = __popcll(bA) + __popcll(bB);
        __syncthreads();
        int e = run + __popcll(bA & lanes_below) + __popcll(bB & lanes_below);
        for (int w = 0; w < 4; ++w) {
            if (w < wave) e += wave_total[w];
            run += wave_total[w];
        }
        if (t < T) {
            ptr[t] = e;
            if (inA) { idx[kA] = t; if (e < K) pos[e] = kA; }
            if (inB) { idx[kB] = t; if (e + inA < K) pos[e + inA] = kB; }
        }
        __syncthreads();
    }
    if (tid == 0) ptr[T] = run;
}

}  // namespace

int launch_draw_masks(const MaskDrawArgs& a, hipStream_t st) {
    if (a.N > 64 || a.S > 64) return MSST_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(draw_masks_kernel, dim3((unsigned)a.rows), dim3(256), 0, st, a);
    return (int)hipGetLastError();
}

}  // namespace msst
