// Feature-guided CRF refinement of class maps (msst_crf_affinity, msst_crf_step; maskedsst_amd/crf.py): a local dense CRF (ConvCRF) over
// the score maps [Bs][nc][Hs][Ws] every scene classifier writes, with the pairwise term taken from the encode_scene feature map
// [Bs][96][Hs][Ws], read in place.  fp32, no inline assembly, no float atomics.
//
// From msst_feat.h: the feature width, the `scores` rule (a dot is the fp32 fmaf chain over d = 0 .. 95 on v_mfma_f32_16x16x4_f32, operands
// at LDS pitch 98), the one total order (feat_ahead) and feat_allow_lds.  Its 64-row tile walk does not apply: the tiles here are spatial.
//
// Neighbours: radius R in 1 .. 3, the K = (2R+1)^2 - 1 offsets (dy, dx) numbered j = 0 .. K-1 with dy ascending, then dx ascending, the
// centre skipped.
//
// crf_affinity   k[p, j] = fmaf(a[j], expf(-(d2 g)), s[j]) for p and q = p + o_j live and q in p's scene, else exactly 0;
//                d2 = max(0, 2 (1 - dot(f_p, f_q) (rn_p rn_q))).  A pixel is live when its 96 features are finite, the fp32 fmaf chain
//                ss = sum_d f_d^2 (d ascending from zero) is positive and finite and cover (when given) is > 0; rn = 1 / sqrtf(ss).
//   grid         one workgroup of 256 threads = 4 waves per tile of 8 x 16 pixels of one scene.
//   LDS          the tile with its halo, (8 + 2R) x (16 + 2R) pixels x 96 channels at pitch 98 (feat_scores' operand pitch), loaded
//                ONCE: 69 KB at R = 1, 94 KB at R = 2, 118 KB at R = 3; rn of the halo pixels; the dots [128][K + 1].
//   dots         wave w owns tile rows 2 w, 2 w + 1.  For a row y and a dy the 16 pixels of the row are the A operand, the halo row
//                y + dy, 16 + 2R pixels in two blocks of 16, the B operand of v_mfma_f32_16x16x4_f32, 24 k-steps ascending from zero:
//                every dot is the fp32 fmaf chain over d = 0 .. 95 (the `scores` rule of msst_feat.h), and a product is commutative,
//                so dot(p, q) has the same bits in whatever tile, and from whichever side, it is formed.  The band |dx| <= R of the
//                16 x 32 block is kept.
//   end          thread = (j, pixel), the 16 pixels of a tile row on adjacent lanes: 64-byte stores of k [Bs][K][Hs][Ws].
//
// crf_step       one mean-field step.  U[c] = scale * score[c] (unary 0) or scale * logf(max(score[c], 1e-30)) (unary 1);
//                x[c] = U[c] + sum_j k[p, j] Q_in[c, p + o_j], the sum one fmaf chain in j order from zero that SKIPS (a test, not a
//                product with zero) every neighbour whose Q_in is NaN -- a dead pixel's probabilities are NaN, and the halo outside
//                the scene is loaded as NaN; Q_out = softmax(x) with the maximum subtracted, the sum in class order.  Without Q_in:
//                Q_out = softmax(U).  A pixel that the affinity's live map marks dead, that has a NaN score or no score above -inf
//                gets NaN probabilities and class -1.
//   grid         one workgroup of 256 threads per tile of 8 x 32 pixels of one scene, thread = pixel; k[p, :] in K registers.
//   LDS          x [nc][256] | Q_in of 8 classes at a time, the tile with its halo (8 + 2R) x (32 + 2R): at most 128 KB + 17 KB.
//   classes      the argmax of Q_out under the one total order (feat_ahead); `changed` counts, with one integer atomic per wave, the
//                live pixels whose class differs from prev_classes (which may be the classes buffer itself: a pixel reads its own
//                entry before it writes it).
#include "../../include/msst.h"
#include "msst_feat.h"
#include "msst_kernels.h"

namespace msst {

namespace {

constexpr int CA_TH = 8, CA_TW = 16;     // the affinity's tile
constexpr int CA_P = 98;                 // LDS pitch of a pixel's 96 features
constexpr int CS_TH = 8, CS_TW = 32;     // the step's tile: one pixel per thread
constexpr int CS_CC = 8;                 // classes of Q_in per LDS chunk

template <int R>
struct CrfGeo {
    static constexpr int S = 2 * R + 1;
    static constexpr int K = S * S - 1;
    static constexpr int CEN = R * S + R;                  // the centre's place in the (dy, dx) raster
    static constexpr int AHH = CA_TH + 2 * R, AHW = CA_TW + 2 * R, ANH = AHH * AHW;
    static constexpr int KP = K + 1;                       // odd: the end's reads of one j over 64 pixels fall on 64 banks
    static constexpr int a_feat = 0;                       // [ANH][CA_P]
    static constexpr int a_rn = a_feat + ANH * CA_P;       // [ANH]
    static constexpr int a_dot = a_rn + ANH;               // [128][KP]
    static constexpr size_t a_bytes = (size_t)4 * (a_dot + CA_TH * CA_TW * KP);
    static constexpr int SHH = CS_TH + 2 * R, SHW = CS_TW + 2 * R, SNH = SHH * SHW;
    static_assert(a_bytes <= 160 * 1024, "the LDS of a CU");
};

struct CrfAffArgs {
    const float* feat;
    const int32_t* cover;
    float* k;
    uint8_t* live;
    int Bs, Hs, Ws, tiles_y, tiles_x;
    float g;
    float a[48], s[48];
};

template <int R>
__global__ __launch_bounds__(256) void crf_affinity_kernel(CrfAffArgs a) {
    using G = CrfGeo<R>;
    constexpr int HW = G::AHW, NH = G::ANH, K = G::K, KP = G::KP, S = G::S;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float* smem = reinterpret_cast<float*>(smem_raw);
    float *sfeat = smem + G::a_feat, *srn = smem + G::a_rn, *sdot = smem + G::a_dot;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cg = lane >> 4, cc = lane & 15;

    int t = blockIdx.x;
    const int tx = t % a.tiles_x;
    t /= a.tiles_x;
    const int ty = t % a.tiles_y, b = t / a.tiles_y;
    const int y0 = ty * CA_TH, x0 = tx * CA_TW;
    const long plane = (long)a.Hs * a.Ws;
    const float* fb = a.feat + (long)b * FEAT_D * plane;

    // ---- the tile with its halo, once; a pixel outside the scene comes as zeros (and is dead by its norm)
    for (int e = tid; e < FEAT_D * NH; e += 256) {
        const int d = e / NH, h = e - d * NH;
        const int hy = h / HW, hx = h - hy * HW;
        const int gy = y0 - R + hy, gx = x0 - R + hx;
        const bool in = gy >= 0 && gy < a.Hs && gx >= 0 && gx < a.Ws;
        sfeat[h * CA_P + d] = in ? fb[d * plane + (long)gy * a.Ws + gx] : 0.f;
    }
    __syncthreads();

    // ---- rn = 1 / |f| of a live pixel, 0 of a dead one
    for (int h = tid; h < NH; h += 256) {
        const float* f = sfeat + h * CA_P;
        float ss = 0.f;
        bool bad = false;
#pragma unroll 8
        for (int d = 0; d < FEAT_D; ++d) {
            const float v = f[d];
            bad |= !(fabsf(v) <= 3.4028234e38f);
            ss = fmaf(v, v, ss);
        }
        const int hy = h / HW, hx = h - hy * HW;
        const int gy = y0 - R + hy, gx = x0 - R + hx;
        const bool in = gy >= 0 && gy < a.Hs && gx >= 0 && gx < a.Ws;
        bool ok = in && !bad && ss > 0.f && ss <= 3.4028234e38f;
        if (ok && a.cover) ok = a.cover[(long)b * plane + (long)gy * a.Ws + gx] > 0;
        srn[h] = ok ? 1.0f / sqrtf(ss) : 0.f;
    }

    // ---- dots: the wave's rows against the halo rows y + dy, on the matrix cores
#pragma unroll 1
    for (int yi = 0; yi < 2; ++yi) {
        const int y = 2 * wave + yi;
        const float* pa = sfeat + ((y + R) * HW + R + cc) * CA_P + cg;
        float af[24];
#pragma unroll
        for (int ks = 0; ks < 24; ++ks) af[ks] = pa[4 * ks];
#pragma unroll 1
        for (int dyi = 0; dyi < S; ++dyi) {
            const int c1 = 16 + cc < HW ? 16 + cc : HW - 1;   // the second block holds 2R pixels; the rest repeats the last (never kept)
            const float* pb0 = sfeat + ((y + dyi) * HW + cc) * CA_P + cg;
            const float* pb1 = sfeat + ((y + dyi) * HW + c1) * CA_P + cg;
            f32x4 c0 = zero4(), c1v = zero4();
#pragma unroll
            for (int ks = 0; ks < 24; ++ks) {
                c0 = PF32::mma(af[ks], pb0[4 * ks], c0);
                c1v = PF32::mma(af[ks], pb1[4 * ks], c1v);
            }
            // lane holds pixels x = 4 cg + r against halo columns cc (c0) and 16 + cc (c1v)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int x = 4 * cg + r;
#pragma unroll
                for (int jb = 0; jb < 2; ++jb) {
                    const int dxi = 16 * jb + cc - x;          // dx + R
                    const int o = dyi * S + dxi;
                    if (dxi >= 0 && dxi < S && o != G::CEN) sdot[(y * CA_TW + x) * KP + (o > G::CEN ? o - 1 : o)] = jb ? c1v[r] : c0[r];
                }
            }
        }
    }
    __syncthreads();

    // ---- the end: k and the live map
    for (int e = tid; e < K * CA_TH * CA_TW; e += 256) {
        const int j = e >> 7, pix = e & 127;
        const int y = pix >> 4, x = pix & 15;
        const int gy = y0 + y, gx = x0 + x;
        if (gy < a.Hs && gx < a.Ws) {
            const int o = j >= G::CEN ? j + 1 : j;
            const int dyi = o / S, dxi = o - dyi * S;
            const float rp = srn[(y + R) * HW + x + R], rq = srn[(y + dyi) * HW + x + dxi];
            float v = 0.f;
            if (rp > 0.f && rq > 0.f) {
                const float cs = sdot[pix * KP + j] * (rp * rq);
                const float d2 = fmaxf(0.f, 2.f * (1.f - cs));
                v = fmaf(a.a[j], expf(-(d2 * a.g)), a.s[j]);
            }
            a.k[((long)b * K + j) * plane + (long)gy * a.Ws + gx] = v;
            if (j == 0) a.live[(long)b * plane + (long)gy * a.Ws + gx] = rp > 0.f ? 1 : 0;
        }
    }
}

template <int R>
int crf_affinity_launch(CrfAffArgs& a, hipStream_t st) {
    constexpr size_t lds = CrfGeo<R>::a_bytes;
    if (int e = feat_allow_lds<&crf_affinity_kernel<R>>(lds)) return e;
    const long n = (long)a.Bs * a.tiles_y * a.tiles_x;
    hipLaunchKernelGGL((crf_affinity_kernel<R>), dim3((unsigned)n), dim3(256), lds, st, a);
    return (int)hipGetLastError();
}

struct CrfStepArgs {
    const float* scores;
    const float* q_in;
    const float* k;
    const uint8_t* live;
    float* q_out;
    int32_t* classes;
    const int32_t* prev;
    int32_t* changed;
    int Bs, nc, Hs, Ws, tiles_y, tiles_x, unary;
    float scale;
};

template <int R>
__global__ __launch_bounds__(256) void crf_step_kernel(CrfStepArgs a) {
    using G = CrfGeo<R>;
    constexpr int HW = G::SHW, NH = G::SNH, K = G::K, S = G::S;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float* sx = reinterpret_cast<float*>(smem_raw);   // [nc][256]
    float* sq = sx + a.nc * 256;                      // [CS_CC][NH]
    const int tid = threadIdx.x;
    const int nc = a.nc;

    int t = blockIdx.x;
    const int tx = t % a.tiles_x;
    t /= a.tiles_x;
    const int ty = t % a.tiles_y, b = t / a.tiles_y;
    const int y0 = ty * CS_TH, x0 = tx * CS_TW;
    const int ly = tid >> 5, lx = tid & 31;
    const int gy = y0 + ly, gx = x0 + lx;
    const bool in = gy < a.Hs && gx < a.Ws;
    const long plane = (long)a.Hs * a.Ws;
    const long p = (long)gy * a.Ws + gx;
    const float* sb = a.scores + (long)b * nc * plane;

    // ---- the unaries, and whether the pixel is live
    bool lv = in && a.live[(long)b * plane + p] != 0;
    bool any = false, nan = false;
    for (int c = 0; c < nc; ++c) {
        const float v = in ? sb[c * plane + p] : 0.f;
        nan |= v != v;
        any |= v > -__builtin_inff();
        sx[c * 256 + tid] = a.unary == 0 ? a.scale * v : a.scale * logf(fmaxf(v, 1e-30f));
    }
    lv = lv && any && !nan;

    if (a.q_in) {   // uniform
        float kv[K];
#pragma unroll
        for (int j = 0; j < K; ++j) kv[j] = lv ? a.k[((long)b * K + j) * plane + p] : 0.f;
        const float* qb = a.q_in + (long)b * nc * plane;
        for (int c0 = 0; c0 < nc; c0 += CS_CC) {
            const int ncc = min(CS_CC, nc - c0);
            __syncthreads();   // the chunk before is done with
            for (int e = tid; e < ncc * NH; e += 256) {
                const int cl = e / NH, h = e - cl * NH;
                const int hy = h / HW, hx = h - hy * HW;
                const int qy = y0 - R + hy, qx = x0 - R + hx;
                const bool qin = qy >= 0 && qy < a.Hs && qx >= 0 && qx < a.Ws;
                sq[e] = qin ? qb[(c0 + cl) * plane + (long)qy * a.Ws + qx] : __builtin_nanf("");
            }
            __syncthreads();
            for (int cl = 0; cl < ncc; ++cl) {
                const float* q = sq + cl * NH + ly * HW + lx;
                float msg = 0.f;
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    const int o = j >= G::CEN ? j + 1 : j;
                    const float qv = q[(o / S) * HW + (o % S)];
                    if (qv == qv) msg = fmaf(kv[j], qv, msg);   // a dead neighbour sends nothing
                }
                sx[(c0 + cl) * 256 + tid] += msg;
            }
        }
    }

    // ---- softmax over the classes, the argmax of the probabilities under the total order
    float m = -__builtin_inff();
    for (int c = 0; c < nc; ++c) m = fmaxf(m, sx[c * 256 + tid]);
    float sum = 0.f;
    for (int c = 0; c < nc; ++c) {
        const float e = lv ? expf(sx[c * 256 + tid] - m) : 0.f;
        sx[c * 256 + tid] = e;
        sum += e;
    }
    float bv = -__builtin_inff();
    int bi = 0x7fffffff;
    float* ob = a.q_out + (long)b * nc * plane;
    for (int c = 0; c < nc; ++c) {
        const float q = lv ? sx[c * 256 + tid] / sum : __builtin_nanf("");
        if (in) ob[c * plane + p] = q;
        if (feat_ahead(q, c, bv, bi)) { bv = q; bi = c; }
    }
    const int cls = lv && bi != 0x7fffffff ? bi : -1;
    bool diff = false;
    if (in && a.prev) diff = lv && a.prev[(long)b * plane + p] != cls;
    if (in && a.classes) a.classes[(long)b * plane + p] = cls;
    if (a.changed && a.prev) {   // uniform
        const int n = __popcll(__ballot(diff));
        if ((tid & 63) == 0 && n) atomicAdd(a.changed, n);
    }
}

template <int R>
int crf_step_launch(CrfStepArgs& a, hipStream_t st) {
    const size_t lds = (size_t)4 * ((size_t)a.nc * 256 + (a.q_in ? CS_CC * CrfGeo<R>::SNH : 0));
    if (int e = feat_allow_lds<&crf_step_kernel<R>>((size_t)4 * (128 * 256 + CS_CC * CrfGeo<R>::SNH))) return e;
    const long n = (long)a.Bs * a.tiles_y * a.tiles_x;
    hipLaunchKernelGGL((crf_step_kernel<R>), dim3((unsigned)n), dim3(256), lds, st, a);
    return (int)hipGetLastError();
}

}  // namespace

int launch_crf_affinity(const float* feat, const int32_t* cover, int Bs, int Hs, int Ws, int R, const float* a_tab, const float* s_tab, float g,
                        float* k, uint8_t* live, hipStream_t st) {
    CrfAffArgs a;
    a.feat = feat; a.cover = cover; a.k = k; a.live = live; a.Bs = Bs; a.Hs = Hs; a.Ws = Ws; a.g = g;
    a.tiles_y = (Hs + CA_TH - 1) / CA_TH;
    a.tiles_x = (Ws + CA_TW - 1) / CA_TW;
    const int K = (2 * R + 1) * (2 * R + 1) - 1;
    for (int j = 0; j < 48; ++j) {
        a.a[j] = j < K ? a_tab[j] : 0.f;
        a.s[j] = j < K ? s_tab[j] : 0.f;
    }
    switch (R) {
        case 1: return crf_affinity_launch<1>(a, st);
        case 2: return crf_affinity_launch<2>(a, st);
        default: return crf_affinity_launch<3>(a, st);
    }
}

long crf_tiles(int Bs, int Hs, int Ws, int which) {   // which 0: the affinity's grid, 1: the step's
    const int th = which ? CS_TH : CA_TH, tw = which ? CS_TW : CA_TW;
    return (long)Bs * ((Hs + th - 1) / th) * ((Ws + tw - 1) / tw);
}

int launch_crf_step(const float* scores, int unary, float unary_scale, const float* q_in, const float* k, const uint8_t* live, int Bs, int nc,
                    int Hs, int Ws, int R, float* q_out, int32_t* classes, const int32_t* prev_classes, int32_t* changed, hipStream_t st) {
    CrfStepArgs a;
    a.scores = scores; a.q_in = q_in; a.k = k; a.live = live; a.q_out = q_out; a.classes = classes; a.prev = prev_classes; a.changed = changed;
    a.Bs = Bs; a.nc = nc; a.Hs = Hs; a.Ws = Ws; a.unary = unary; a.scale = unary_scale;
    a.tiles_y = (Hs + CS_TH - 1) / CS_TH;
    a.tiles_x = (Ws + CS_TW - 1) / CS_TW;
    switch (R) {
        case 1: return crf_step_launch<1>(a, st);
        case 2: return crf_step_launch<2>(a, st);
        default: return crf_step_launch<3>(a, st);
    }
}

}  // namespace msst
