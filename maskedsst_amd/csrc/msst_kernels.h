// Internal kernel argument blocks + launcher prototypes (C++ side of the C-ABI in include/msst.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "msst_dev.h"

#define MSST_PREC_F32 0
#define MSST_PREC_BF16 1
#define MSST_ERR_UNSUPPORTED (-2)
#define MSST_ERR_BADARG (-3)
#define MSST_ADAM_MAX_GROUPS 64
#define MSST_GRAD_MAX_RANGES 64
#define MSST_MASK_TOPK 0
#define MSST_MASK_BLOCK 1
#define MSST_MASK_TUBE 2

namespace msst {

// Per-block weights.  The big matrices are "prepped" copies in the operand element type
// (fp32 or bf16), each also in transposed form for the backward GEMMs; the small vectors are fp32.
struct BlockWeights {
    const void* wqkv;   // [3*H*64][96]   rows: q heads | k heads | v heads (reference chunk order)
    const void* wout;   // [96][H*64]
    const void* w1;     // [64][96]
    const void* w2;     // [96][64]
    const void* wqkvT;  // [96][3*H*64]
    const void* woutT;  // [H*64][96]
    const void* w1T;    // [96][64]
    const void* w2T;    // [64][96]
    const float* ln1_g; const float* ln1_b; const float* bo;
    const float* ln2_g; const float* ln2_b; const float* b1; const float* b2;
    const void* wqkv32; const void* woutT32; const void* wqkvT32;   // bf16, 32 x 16 fragment packing (optional)
};

struct BlockArgs {
    BlockWeights w;
    const float* x;   // [tokens][96] block input (residual stream, fp32)
    float* y;         // [tokens][96] block output
    float* x1;        // [tokens][96] mid-block residual (x + attn), saved for the backward; may be null
    int x1_bf16;      // MSST_X1_BF16: x1 holds bf16 (role-split forward only)
    int half;         // MSST_FWD_HALF: the forward's GEMM operands are IEEE half (w.wqkv / wout / w1 / w2 then point at the half copies); role-split forward only
    void* xn_out;     // optional [tokens][96] bf16: LN1(x) exactly as the block used it, saved for the attention backward (head-per-wave kernel only)
    float* lse_out;   // optional [ntiles][H][64] fp32: per (tile, head, row) log2 of the softmax denominator of the scaled scores, max folded in
                      // (p = exp2(s scale log2 e - lse)): the attention backward then skips max / sum / 1 / x (role-split kernel only)
    TileMap tm;
    int ntiles, max_grid, H;
    float scale;      // dim_head^-0.5
    int dbg;          // ablation switches for kernel studies (0 in production)
    unsigned long long* stamps;  // dbg & 8: s_memtime stamps of one wave (kernel studies)
    Drop drop;
};

// A run of blocks of ONE stack (same mode) as one launch of the role-split forward (msst_fwd3.hip, STACK): per-block operands
#define MSST_MAX_STACK 16
struct StackBlk {
    const void* wqkv; const void* wout; const void* w1; const void* w2;
    const float* ln1_g; const float* ln1_b; const float* bo; const float* ln2_g; const float* ln2_b; const float* b1; const float* b2;
    const float* x; float* y; float* x1; void* xn_out; float* lse_out;
    int layer, pad_;
};
struct StackStride {   // byte distance of every per-block operand from one block of the run to the next (the caller's arrays are affine in the block index)
    int wqkv, wout, w1, w2, ln1_g, ln1_b, bo, ln2_g, ln2_b, b1, b2, x, y, x1, xn_out, lse_out;
};
struct StackArgs {
    BlockArgs base;   // what does not depend on the block: tile map, heads, scale, dropout stream (its `layer` is per block below), x1_bf16
    int nblk;
    StackBlk b0;      // block 0 of the run
    StackStride st;
    const float* x_rest;   // y of block 0 minus one y stride: block j >= 1 reads x_rest + j x st.y
};
static_assert(sizeof(StackArgs) <= 4096, "StackArgs travels as a kernel argument");

// Where the samples of a tokenizer or SimMIM-head launch lie: THE one description, embedded once in TokArgs, TokBwdArgs, TokInArgs and
// HeadArgs, filled by fill_src (msst_api.hip) and read only through the win_* accessors below.  A kernel is compiled per kind:
//   WIN_BATCH            sample b is cube b of a batch [B][C][N]; of the fields only `base` is read
//   WIN_GRID             base is scenes [Bs][C][Hs][Ws]; sample b is window win0 + b of the grid (win, stride), row-major over (scene, window
//                        row, window column), origin (r * stride, q * stride), win x win pixels
//   WIN_LISTED           ... the window of scene origins[b][0] with its top-left pixel at row origins[b][1], column origins[b][2]; of the grid
//                        fields only Hs, Ws and win are read
//   WIN_LISTED_ORIENTED  ... that window in orientation orient[b] (window_steps): token n is pixel n of the ORIENTED window, so position row,
//                        mask byte, dropout element and gradient row are those of the oriented copy -- only the address of the read differs
enum { WIN_BATCH = 0, WIN_GRID = 1, WIN_LISTED = 2, WIN_LISTED_ORIENTED = 3 };
struct WinRef {
    const float* base;       // the batch, or the scenes
    long win0;
    int Hs, Ws, win, stride, nq, wps;   // nq: windows per window row, wps: windows per scene
    const int32_t* origins;  // [B][3]
    const uint8_t* orient;   // [B], codes 0 .. 7
};

// An orientation code o = k + 4 f (k in 0 .. 3, f in 0 .. 1) names one of the eight symmetries of a win x win window w: flipped left to
// right when f, then turned k quarter turns counter-clockwise -- torch.rot90(torch.flip(w, (-1,)) if f else w, k, (-2, -1)).  It is a
// different affine map for the same read: pixel (i, j) of the oriented window lies start + i * si + j * sj floats from the window's
// origin, si and sj in {+-1, +-Ws}.  Only the low three bits of the code are looked at, so whatever the byte holds every read stays
// inside the window.
struct WinSteps { int start, si, sj; };
__device__ __forceinline__ WinSteps window_steps(int o, int win, int Ws) {
    const int k = o & 3, m = win - 1;
    // the un-flipped source pixel (y, x) = (y0 + yi i + yj j, x0 + xi i + xj j) of quarter turn k: (i, j), (j, m - i), (m - i, m - j), (m - j, i)
    const int yi = (k == 0) - (k == 2), yj = (k == 1) - (k == 3), y0 = k >= 2 ? m : 0;
    int xi = (k == 3) - (k == 1), xj = (k == 0) - (k == 2), x0 = (k == 1 || k == 2) ? m : 0;
    if (o & 4) { x0 = m - x0; xi = -xi; xj = -xj; }   // the flip: x -> m - x
    return WinSteps{y0 * Ws + x0, yi * Ws + xi, yj * Ws + xj};
}

// floats from one plane (band) of a sample to the next; N: pixels per sample (a batch's planes are N floats, and an int)
template <int KIND>
__device__ __forceinline__ auto win_plane(const WinRef& w, int N) {
    if constexpr (KIND == WIN_BATCH) return N;
    else return (long)w.Hs * w.Ws;
}
// the first band of spectral block c of sample b, at its window's first pixel, in a tensor at `base` laid out like the source: S
// blocks of P bands per cube or scene (the pixels: w.base, S, P; a gradient of their shape; a scene mask [Bs][S][Hs][Ws]: P = 1).
// 64-bit: scenes may be large.  A listed window costs one 12-byte read of its table row
template <int KIND, class T>
__device__ __forceinline__ T* win_origin(T* base, const WinRef& w, int b, int c, int S, int P, int N) {
    if constexpr (KIND == WIN_BATCH) return base + ((long)b * S + c) * P * N;
    else {
        long s, y0, x0;
        if constexpr (KIND == WIN_GRID) {
            const long i = w.win0 + b;
            s = i / w.wps;
            const int rem = (int)(i - s * w.wps), r = rem / w.nq, q = rem - r * w.nq;
            y0 = (long)r * w.stride; x0 = (long)q * w.stride;
        } else {
            const int32_t* o = w.origins + 3 * (long)b;
            s = o[0]; y0 = o[1]; x0 = o[2];
        }
        return base + (((s * S * P) * w.Hs + y0) * w.Ws + x0) + (long)c * P * win_plane<KIND>(w, N);
    }
}
// the orientation of sample b's window (oriented kind only): a workgroup that stays on one window reads it once
template <int KIND>
__device__ __forceinline__ WinSteps win_steps(const WinRef& w, int b) {
    if constexpr (KIND == WIN_LISTED_ORIENTED) return window_steps(w.orient[b], w.win, w.Ws);
    else return WinSteps{};
}
// `from` plus the floats from the first pixel of a window to its pixel n = i * win + j, for a workgroup that stays on the window and
// has read its orientation once (ws: win_steps of the window).  Oriented: 32-bit products (at most 8 Ws), added to `from` left to right
template <int KIND>
__device__ __forceinline__ long win_pixel(const WinRef& w, const WinSteps& ws, int n, long from = 0) {
    if constexpr (KIND == WIN_BATCH) return from + n;
    else if constexpr (KIND == WIN_LISTED_ORIENTED) return from + ws.start + (n / w.win) * ws.si + (n % w.win) * ws.sj;
    else return from + (long)(n / w.win) * w.Ws + n % w.win;
}
// the same for a lane that meets window b once and reads its orientation itself (64-bit products, as these callers always compiled)
template <int KIND>
__device__ __forceinline__ long win_pixel(const WinRef& w, int b, int n) {
    if constexpr (KIND == WIN_LISTED_ORIENTED) {
        const WinSteps ws = win_steps<KIND>(w, b);
        return (long)ws.start + (long)(n / w.win) * ws.si + (long)(n % w.win) * ws.sj;
    } else return win_pixel<KIND>(w, WinSteps{}, n);
}
// the byte of token (c, n) of sample b's window in a scene mask [Bs][S][Hs][Ws]: one byte per spectral block and pixel
template <int KIND>
__device__ __forceinline__ uint8_t win_scene_mask(const WinRef& w, const uint8_t* mask, int b, int c, int S, int n) {
    return win_origin<KIND>(mask, w, b, c, S, 1, 0)[win_pixel<KIND>(w, b, n)];
}

// mask policy of the tokenizer forward: nothing masked; a.mask [B][T] in sample coordinates; a.mask a scene mask [Bs][S][Hs][Ws]
enum { MASK_NONE = 0, MASK_TOKENS = 1, MASK_SCENE = 2 };
struct TokArgs {
    WinRef src;              // the pixels: [B][S*P][N], or windows of scenes
    const float* pre_g; const float* pre_b;     // [P]
    const float* w_emb;      // [S][96][P]
    const float* b_emb;      // [S][96]
    const float* post_g; const float* post_b;   // [96]
    const float* pos_a;      // pos_split == 0: learned table [T][96]; else spatial table [N][pos_split]
    const float* pos_b;      // pos_split != 0: spectral table [S][96 - pos_split]
    const float* mask_token; // [96]
    const uint8_t* mask;     // MASK_TOKENS: [B][T] (1 = masked), all-zero for the classification path; MASK_SCENE: [Bs][S][Hs][Ws]
    float* out;              // [B][T][96]
    int B, S, N, T, P, pos_split;   // B: samples = windows of the call
    Drop drop;               // embedding dropout on (token + pos) (vit_spatial_spectral.py:530), classification path only
};

// the windows covering pixel (y, x) of a scene: window rows rlo .. rhi and columns qlo .. qhi of the grid (Args: win, stride, nr, nq);
// false when no window covers it
template <class Args>
__device__ __forceinline__ bool scene_cover(const Args& a, int y, int x, int& rlo, int& rhi, int& qlo, int& qhi) {
    rlo = y < a.win ? 0 : (y - a.win) / a.stride + 1;
    rhi = min(y / a.stride, a.nr - 1);
    qlo = x < a.win ? 0 : (x - a.win) / a.stride + 1;
    qhi = min(x / a.stride, a.nq - 1);
    return rlo <= rhi && qlo <= qhi;
}

// the window grid of a batch of scenes and the windows of one call: windows win0 .. win0 + nwin - 1, row-major over (scene, window
// row, window column), nr x nq per scene, origin (r * stride, q * stride), win x win pixels.  The argument blocks of the three scene
// folds (SceneArgs, SceneReconArgs, SceneEmbedArgs) inherit it; scene_cover reads it.
struct SceneGrid {
    long win0, row0;           // row0: first flattened (scene, pixel row) row the windows of the call touch (scene_call_rows, msst_api.hip)
    int nwin, Bs, Hs, Ws, win, stride, nr, nq;
};
// The one fold of per-window planes into per-scene planes (scene_fold_kernel, msst_fwd.hip): src [nwin][C][win * win] of the call's windows is
// added into the running sums dst [Bs][C][Hs][Ws]; a launch's `pixels` start at flattened row g.row0; `group` (at most 16) consecutive
// channels per grid row y, C <= 65535 * group.  Every scene feature accumulates through it, so a split into calls leaves every bit.
int launch_scene_fold(const SceneGrid& g, const float* src, float* dst, int C, int group, long pixels, hipStream_t st);

// scene assembly (msst_scene_assemble): per-window logits -> running per-pixel sums (launch_scene_fold), then mean / argmax (finalize)
struct SceneArgs : SceneGrid {
    const float* win_logits;   // [nwin][NC][win * win] of windows win0 .. win0 + nwin - 1
    float* logits;             // [Bs][NC][Hs][Ws]: the running sums, then the means
    int64_t* classes;          // [Bs][Hs][Ws]
    int NC;
};
int launch_scene_finalize(const SceneArgs& a, hipStream_t st);

struct HeadArgs {
    WinRef src;          // the targets: [B][S*P][N], or listed windows of scenes (plain or oriented)
    const float* y;      // [B][T][96] encoder output
    const int* idx;      // [B][K] masked token indices
    const float* w_pix;  // [S or 1][P][96]
    const float* b_pix;  // [S or 1][P]
    float* dpred;        // [B][K][P] sign(pred - target)
    float* pred;         // optional [B][K][P]
    float* partial;      // [B * ceil(K/64)]
    int B, S, N, T, P, K, per_block;
};

struct HeadBwdArgs {
    const float* y; const float* dpred; const int* csr_ptr; const int* csr_pos; const float* w_pix;
    float* dy; float* slab; float gscale;
    const float* gout;   // optional device scalar: d(final)/d(loss), multiplied into gscale
    int B, S, N, T, P, K, per_block;
};

#define MSST_MLP_SLAB_N (64 * 96 + 96 * 64 + 64 + 96 + 96 + 96)
#define MSST_ATTN_SLAB_N (3 * 64 * 96 + 96 * 64)

struct MlpBwdArgs {
    BlockWeights w;
    const float* x1; const float* dy; float* dx1; float* slab;
    void* dab;   // optional [tokens][96] bf16: dx1 with the to_out dropout (site 2) applied, packed -- what the bf16 attention backward feeds its MFMAs
    long ntok;
    Drop drop;
    int x1_bf16;  // MSST_X1_BF16: x1 holds bf16 (bf16 kernel only)
};

struct AttnBwdArgs {
    BlockWeights w;
    const float* x; const float* da; void* dxn_part; float* slab;
    const void* dab;  // optional [tokens][96] bf16 pre-dropped da rows written by the MLP half (given together with xn)
    const void* xn;   // optional [tokens][96] bf16 LN1(x) saved by the forward: the bf16 kernel then neither re-reads x nor renormalises
    TileMap tm;
    int ntiles, H;
    long ntok;
    float scale;
    int dbg;
    unsigned long long* stamps;
    Drop drop;
    int* queue;       // optional (two-head kernel): one zeroed counter per head pair -> dynamic tile queue instead of the static partition
    const float* lse; // optional (two-head kernel): [ntiles][H][64] saved by the forward (BlockArgs.lse_out)
    int lse_renorm;   // MSST_LSE_RENORM: the forward's scores are not this kernel's (half-operand forward): exp2(s c - lse) rows are renormalised by their own sum
};

struct Ln1BwdArgs {
    const float* x; const float* dx1; const void* dxn_part; const float* ln1_g; float* dx; float* slab;
    long ntok;
    int H;
    Drop drop;
};

// LN1 backward of block i fused with the MLP-half backward of block i - 1 (msst_bwd5.hip)
struct LnMlpArgs {
    BlockWeights w;          // block i - 1 (MLP half: w1, w1T, w2T, ln2_g, ln2_b, b1)
    const float* ln1_g;      // block i
    const float* ln1_b;      // block i (xn path only)
    const void* xn;          // optional: [tokens][96] bf16 LN1 rows of block i as its forward used them, with
    const float* rstd;       //           [tokens] rstd of that LN1: xhat = (xn - ln1_b) / ln1_g replaces the read + renormalisation of x
    const float* x;          // [tokens][96] input of block i (= output of block i - 1)
    float* dx1;              // in: dx1 of block i (gradient at its mid residual); out: dx1 of block i - 1 (same rows, in place)
    const void* dxn_part;    // [nparts][tokens][96] bf16 partial d(LN1 out) of block i
    const float* x1;         // [tokens][96] mid residual of block i - 1 (fp32, or bf16 with x1_bf16)
    int x1_bf16;
    void* dab;               // out: [tokens][96] bf16, dx1 of block i - 1 with the to_out dropout applied (attention half's operand)
    float* slab_mlp;         // [grid][MSST_MLP_SLAB_N]
    float* slab_ln1;         // [grid][288]
    long ntok;
    int nparts;
    Drop drop_i, drop_p;     // dropout streams of block i (site 2) and of block i - 1 (sites 2, 3, 4)
    unsigned long long* stamps;   // -DMSST_STAMPS builds: cycle stamps of the eight waves of one workgroup (tools/stamps_bwd5.py)
    int* queue;                   // optional: one zeroed counter -> dynamic tile queue instead of the static partition
};

struct TokBwdArgs {
    WinRef src;
    const float* pre_g; const float* pre_b; const float* w_emb; const float* b_emb;
    const float* post_g; const float* post_b;
    const uint8_t* mask;     // [B][T] in sample coordinates; a window source may pass none (nothing masked)
    const float* dx0; float* slab;
    int B, S, N, T, P;
    Drop drop;
};

// msst_input_grad.hip: d(loss)/d(img) from dx0
struct TokInArgs {
    WinRef src;
    const float* pre_g; const float* pre_b; const float* w_emb; const float* b_emb;
    const float* post_g; const float* post_b;
    const uint8_t* mask;     // optional [B][T] (1 = masked)
    const float* dx0;        // [B][T][96]
    const float* dtarget;    // optional [B][S*P][N], added before the store
    float* dimg;             // [B][S*P][N], stacked (WIN_BATCH, WIN_LISTED); WIN_GRID: dscene [Bs][S*P][Hs][Ws], stored in place
    int B, S, N, T, P;
    Drop drop;
};
// msst_scene_fold_at: dwin [nwin][C][win * win] of windows at listed origins, summed per pixel into dscene [Bs][C][Hs][Ws] through the
// inverse index cell_ptr [Bs Hs Ws + 1] / cell_win [nwin] over origin cells (scene_fold_at_kernel, msst_input_grad.hip)
struct SceneFoldAtArgs {
    const float* dwin; const int32_t* cell_ptr; const int32_t* cell_win; float* dscene;
    int Bs, C, Hs, Ws, win, nwin, group, accumulate;
};
int launch_tokenize_bwd_input(const TokInArgs& a, int kind, hipStream_t st);   // kind: WIN_BATCH, WIN_GRID or WIN_LISTED
int launch_scene_fold_at(const SceneFoldAtArgs& a, hipStream_t st);
int launch_scene_border_zero(float* dscene, long rows, int Hs, int Ws, int rows_in, int cols_in, hipStream_t st);
int launch_head_bwd_target(const float* dpred, const int* csr_ptr, const int* csr_pos, const float* gout, float gscale, float* dtarget,
                           int B, int S, int N, int P, int K, hipStream_t st);

// ---- opt-in per-kernel timing with HIP events on the launch stream (bench.py roofline leg) ----
enum KernelId {
    K_PREP = 0, K_TOK_FWD, K_BLOCK_FWD, K_HEAD_FWD, K_LOSS_REDUCE, K_HEAD_BWD, K_REDUCE, K_BWD_MLP, K_BWD_ATTN,
    K_ATTN_REDUCE, K_BWD_LN1, K_TOK_BWD, K_POS_SPLIT, K_ADAMW, K_BWD_LN1MLP, K_LAYERNORM, K_ADAM_GROUPS, K_CE, K_RECON, K_TOK_BWD_INPUT,
    K_HEAD_BWD_TARGET, K_GRAD_ACCUM, K_GRAD_FINAL, K_COUNT
};
void prof_begin(int id, hipStream_t st);
void prof_end(hipStream_t st);
struct ProfScope {
    hipStream_t st;
    ProfScope(int id, hipStream_t s) : st(s) { prof_begin(id, s); }
    ~ProfScope() { prof_end(st); }
};

struct ClsArgs {
    const float* y; const float* ln_g; const float* ln_b; const float* w; const float* b; float* logits;
    int B, S, N, T, NC;
};
struct ClsBwdArgs {
    const float* y; const float* dlogits; const float* ln_g; const float* ln_b; const float* w;
    float* dy; float* slab;
    int B, S, N, T, NC;
};
int launch_cls_head_fwd(const ClsArgs& a, hipStream_t st);
int launch_cls_head_bwd(const ClsBwdArgs& a, hipStream_t st);
// spectral MLP head (msst_head.hip): rows R = B N of F = 96 S features; G chunks of RC rows in the weight-gradient pass,
// slab g at slab + g slab_stride, stats [R][2] (mean, rstd) written by the row backward
struct SpecHeadArgs {
    const float* y; const float* ln_g; const float* ln_b; const float* w; const float* b; const float* dlogits;
    float* logits; float* dy; float* stats; float* slab;
    long slab_stride;
    int B, S, N, T, NC, R, G, RC;
};
void spec_head_chunks(long R, int& G, int& RC);
long spec_head_bwd_slab_floats(int B, int S, int N, int NC);
int launch_spec_head_fwd(const SpecHeadArgs& a, hipStream_t st);
int launch_spec_head_bwd_rows(const SpecHeadArgs& a, hipStream_t st);
int launch_spec_head_wgrad(const SpecHeadArgs& a, hipStream_t st);
int launch_spec_head_wgrad_finish(const SpecHeadArgs& a, const float* A, const float* db, float* dw, float* dg, float* dbeta,
                                  hipStream_t st);
// pixelwise centre-pixel head (msst_pixhead.hip): K = 96 N features per sample; G = pix_head_groups(B) groups of 32 samples;
// xn [B][K] the forward's workspace; slab: pix_head_bwd_slab_floats(B, N, NC) floats of weight-gradient partials
struct PixHeadArgs {
    const float* y; const float* ln_g; const float* ln_b; const float* w; const float* b; const float* dlogits;
    float* logits; float* xn; float* dy; float* slab;
    int B, S, N, T, NC, G;
};
int pix_head_groups(int B);
long pix_head_bwd_slab_floats(int B, int N, int NC);
int launch_pix_head_fwd(const PixHeadArgs& a, hipStream_t st);
int launch_pix_head_bwd(const PixHeadArgs& a, hipStream_t st);
int launch_scene_centre_scatter(const SceneArgs& a, hipStream_t st);   // SceneArgs.win_logits: [nwin][NC]
int launch_scene_centre_fill(const SceneArgs& a, hipStream_t st);

// the seven (kind, mask) pairs that exist: (WIN_BATCH, MASK_TOKENS), (WIN_GRID, MASK_NONE / MASK_SCENE), (WIN_LISTED*, MASK_NONE / MASK_TOKENS)
int launch_tokenize_fwd(const TokArgs& a, int kind, int mask, hipStream_t st);
int launch_head_bwd(const HeadBwdArgs& a, int nchunk, hipStream_t st);
// One reduction segment: dst[(i / row_len) * row_stride + i % row_len] = sum_{k < nslab} src[k * slab_stride + i], i < n
struct RSeg {
    const float* src; float* dst;
    long slab_stride;
    int nslab, n, row_len, row_stride, blk0, vec4;
    int ny;   // batched launches (blockIdx.y = y): the segment exists for y < ny
};
#define MSST_MAX_RSEG 72
// A batched launch (ny_max > 1) reduces the same segment table for ny_max slab sets src_ystride floats apart into destinations
// dst_ystride floats apart (the deferred reduction of a run of msst_block_bwd_chain calls: one slab set and one gradient block per call).
struct RSegs { RSeg s[MSST_MAX_RSEG]; int nseg; int nblocks; int ny_max; long src_ystride, dst_ystride; };
struct RSegBuilder {
    RSegs r;
    RSegBuilder() { r.nseg = 0; r.nblocks = 0; r.ny_max = 1; r.src_ystride = 0; r.dst_ystride = 0; }
    bool add(const float* src, long slab_stride, int nslab, float* dst, int n, int row_len = 0, int row_stride = 0, int ny = 1) {
        if (r.nseg >= MSST_MAX_RSEG) return false;
        if (ny < 1) return true;   // a segment no launch of the batch wrote
        RSeg& g = r.s[r.nseg++];
        g.ny = ny;
        if (ny > r.ny_max) r.ny_max = ny;
        g.src = src; g.dst = dst; g.slab_stride = slab_stride; g.nslab = nslab; g.n = n;
        g.row_len = row_len > 0 ? row_len : n; g.row_stride = row_stride > 0 ? row_stride : n;
        g.blk0 = r.nblocks;
        // 16-byte path: a thread owns 4 consecutive outputs (one dwordx4 per slab) when every address involved is aligned
        // (batched: the y strides must keep that alignment too -- checked by the caller that sets them)
        g.vec4 = (n % 4 == 0 && g.row_len % 4 == 0 && g.row_stride % 4 == 0 && slab_stride % 4 == 0 &&
                  ((uintptr_t)src % 16) == 0 && ((uintptr_t)dst % 16) == 0) ? 1 : 0;
        const int per_block = g.vec4 ? 128 : 32;
        r.nblocks += (n + per_block - 1) / per_block;
        return true;
    }
};
static_assert(sizeof(RSegs) <= 4096, "RSegs travels as a kernel argument");
int launch_reduce_segs(const RSegs& r, hipStream_t st);
int launch_block_bwd_mlp(const MlpBwdArgs& a, int grid, int prec, hipStream_t st);
int launch_block_bwd_attn(const AttnBwdArgs& a, int nchunk, int prec, hipStream_t st, int* nparts);
int launch_block_bwd_attn_r3(const AttnBwdArgs& a, int nchunk, hipStream_t st);     // msst_bwd3.hip (bf16 throughput kernel: one GEMM per wave, 32x32x16 tiles)
int launch_block_bwd_attn_r4(const AttnBwdArgs& a, int nchunk, hipStream_t st);     // msst_bwd4.hip (the same, two heads per workgroup half a tile apart)
int launch_block_bwd_ln1(const Ln1BwdArgs& a, int grid, int prec, hipStream_t st);
int launch_block_bwd_ln1mlp(const LnMlpArgs& a, int grid, hipStream_t st);   // msst_bwd5.hip (bf16: LN1 backward of block i + MLP backward of block i - 1)
int launch_tokenize_bwd(const TokBwdArgs& a, int kind, int nchunk, hipStream_t st);
int launch_pos_split(const float* dpos, int S, int N, int split, float* dpe, float* dce, hipStream_t st);
int launch_adamw(float* p, const float* g, float* m, float* v, long n, float lr, float b1, float b2, float eps,
                 float wd, int step, float clamp, float gscale, hipStream_t st);
// grouped Adam (msst_opt.hip): the range table as the kernel receives it -- by value, constants already formed on the host
struct AdamSeg {
    long start, end;     // element range
    long a0, a1;         // its 16-byte aligned interior [a0, a1) (a0 == a1 == end: none; the whole range then moves float by float)
    float step_size, bc2_sqrt, wd, decay;   // lr / (1 - b1^t), sqrt(1 - b2^t), coupled L2 factor (0 when decoupled), 1 - lr wd (1 when coupled)
    int blk0, pad;       // first workgroup of the range
};
struct AdamTable {
    AdamSeg s[MSST_ADAM_MAX_GROUPS];
    float b2, omb1, omb2, eps, gscale;
    int nseg, nblocks;
};
constexpr int ADAM_QPB = 1024;   // float4 pieces of a range's aligned interior per workgroup (256 threads x 4)
static_assert(sizeof(AdamTable) <= 4096, "AdamTable travels as a kernel argument");
int launch_adam_groups(float* p, const float* g, float* m, float* v, const AdamTable& t, hipStream_t st);
// gradient accumulation / global-norm clip (msst_accum.hip): the range table as the kernels receive it.  A range's 16-byte aligned
// interior is walked by nblk workgroups in a strided loop (lb, lb + nblk, ... pieces of 256 U float4), its ragged ends by the first.
struct GradSeg {
    long start, end;     // element range
    long a0, a1;         // its 16-byte aligned interior (a0 == a1 == end: none; the whole range then moves float by float)
    int blk0, nblk;      // first workgroup of the range, workgroups of the range
};
struct GradTable {
    GradSeg s[MSST_GRAD_MAX_RANGES];
    int nseg, nblocks;
};
static_assert(sizeof(GradTable) <= 4096, "GradTable travels as a kernel argument");
constexpr int GRAD_GRID = 512;             // grid cap of both launches (+ at most one workgroup per range): 2 workgroups per CU ...
constexpr int GRAD_U = 4;                  // ... that keep four float4 per buffer and lane in flight per trip of the strided loop
int launch_grad_accumulate(float* acc, const float* g, float* out, float scale, int first, double* part_sum, unsigned* part_bad,
                           const GradTable& t, hipStream_t st);
int launch_grad_finalize(const float* acc, float* g, float scale, float max_norm, const double* part_sum, const unsigned* part_bad,
                         int nparts, float* record, const GradTable& t, hipStream_t st);
int launch_cu_thief(int nblocks, int us, unsigned* sink, hipStream_t st);   // msst_opt.hip (occupancy probe)
int launch_box_probe(double* out4, void* scratch, long bytes, hipStream_t st);   // msst_opt.hip (MFMA rate / shader clock / HBM read rate of this box)
int launch_block_fwd_rs(const BlockArgs& a, int grid, hipStream_t st);   // msst_fwd3.hip (bf16, 8 heads; role split: the default)
int launch_block_fwd_rs_stack(const StackArgs& a, int grid, hipStream_t st);   // the same for a run of blocks of one stack, ONE launch
int block_fwd_stack_max_steps();
int launch_block_fwd(const BlockArgs& a, int prec, hipStream_t st);
bool block_fwd_writes_xn(const BlockArgs& a, int prec);   // does the kernel launch_block_fwd selects honour a.xn_out?
bool block_fwd_writes_lse(const BlockArgs& a, int prec);  // ... a.lse_out?  (the role-split kernel: bf16, 8 heads, no selection flags)
int launch_head_fwd(const HeadArgs& a, int kind, float* loss, hipStream_t st);   // kind: WIN_BATCH, WIN_LISTED or WIN_LISTED_ORIENTED
// msst_ln.hip: stand-alone LayerNorm over the last axis (D <= 128; D = 96 vectorised)
int launch_layernorm_fwd(const float* x, const float* g, const float* b, float* y, float* mean, float* rstd, long rows, int D,
                         float eps, hipStream_t st);
int layernorm_bwd_grid(long rows, int D);   // workgroups (= slab rows of 2 D floats) the backward launch uses
int launch_layernorm_bwd(const float* x, const float* g, const float* dy, float* dx, float* slab, int grid, long rows, int D,
                         float eps, hipStream_t st);
// msst_loss.hip: softmax cross entropy with ignore_index over class-major logits [R0][NC][M], rows = R0 M (one lane per row),
// optionally with class weights, label smoothing and a confusion matrix.  One kernel family; w, eps = 0, wpartial, cslab, confusion
// and sums all null / 0 is the plain call
constexpr int CE_CONF_MAX_CLASSES = 128;   // include/msst.h: MSST_CE_CONFUSION_MAX_CLASSES (msst_api.hip asserts they agree)
struct CeArgs {
    const float* logits; const int64_t* labels; const int64_t* skip;   // skip: optional [rows], entries < 0 do not count
    float* d;             // optional [R0][NC][M]: the loss sum's gradient (unweighted: softmax - onehot; zeros for rows that do not count)
    float* loss;          // the mean over the rows that count (NaN over none, or over none of positive weight)
    int64_t* record;      // [5 + 2 NC]: loss sum (a double) | n_valid | n_correct | bad_labels | nonfinite | support[NC] | correct[NC]
    float* partial;       // [workgroups] loss partials
    int* slab;            // [workgroups][4 + 2 NC] count partials
    long rows, ignore_index;
    int NC, M;
    const float* w;       // optional [NC] class weights (null: ones)
    float eps;            // label smoothing, in [0, 1)
    float* wpartial;      // [workgroups] partials of the counting rows' w[label]; written and read only with w or eps != 0
    int* cslab;           // [workgroups][NC][NC] confusion partials, null when no confusion matrix is wanted
    int64_t* confusion;   // [NC][NC] (label, argmax) over the counting rows; null with cslab
    double* sums;         // optional [2]: the loss sum (= record slot 0) | what the mean divides by (the sum of w[label]; n_valid)
};
int ce_workgroups(long rows);   // workgroups of the forward launch = rows of its partial arrays
int launch_ce_fwd(const CeArgs& a, hipStream_t st);
int launch_ce_finish(const CeArgs& a, hipStream_t st);
int launch_ce_bwd(const float* d, const int64_t* record, const float* gout, float* dlogits, long n, hipStream_t st);   // over record[1]
int launch_ce_ext_bwd(const float* d, const double* sums, const float* gout, float* dlogits, long n, hipStream_t st);   // over sums[1]
// msst_recon.hip: to_pixels over every token into the cube layout, with the per-band |pred - img| sums over the masked pixels
struct ReconArgs {
    const float* y;        // [B][T][96] encoder output (16-byte aligned)
    const float* img;      // [B][S*P][N]
    const uint8_t* mask;   // [B][T] (1 = masked)
    const float* w_pix;    // [S or 1][P][96]
    const float* b_pix;    // [S or 1][P]
    float* recon;          // [B][S*P][N]
    double* band_err;      // optional [B][S*P] (with band_cnt)
    int32_t* band_cnt;     // optional [B][S*P]
    int B, S, N, P, per_block, blend;
};
int launch_recon_fwd(const ReconArgs& a, hipStream_t st);

// msst_scene_recon.hip (msst_scene_recon_assemble): per-window pixel predictions -> running per-pixel sums (launch_scene_fold), then the
// mean, the blend with the scene, the per-band masked |pred - scene| sums and the cover map (finalize)
struct SceneReconArgs : SceneGrid {
    const float* win_recon;      // [nwin][S*P][win * win] of windows win0 .. win0 + nwin - 1 (msst_recon_fwd, blend = 0)
    const float* scene;          // [Bs][S*P][Hs][Ws]
    const uint8_t* scene_mask;   // [Bs][S][Hs][Ws] (non-zero = masked)
    float* cube;                 // [Bs][S*P][Hs][Ws]: the running sums, then the result
    double* band_err;            // optional [Bs][S*P] (with band_cnt)
    int32_t* band_cnt;           // optional [Bs][S*P]
    int32_t* cover;              // [Bs][Hs][Ws]: windows covering the pixel
    int S, P, blend;
};
int launch_scene_recon_finalize(const SceneReconArgs& a, hipStream_t st);

// msst_scene_embed.hip (msst_pool_spectral_fwd, msst_scene_embed_assemble): encoder output -> per-window features (mean over the
// spectral tokens of a position) -> running per-pixel sums (launch_scene_fold), then the mean, the optional L2 normalisation, NaN where
// no window covers a pixel and the cover map (finalize)
struct SceneEmbedArgs : SceneGrid {
    const float* win_feat;       // [nwin][D][win * win] of windows win0 .. win0 + nwin - 1 (msst_pool_spectral_fwd)
    float* feat;                 // [Bs][D][Hs][Ws]: the running sums, then the result
    int32_t* cover;              // [Bs][Hs][Ws]: windows covering the pixel
    int D, l2norm;
};
int launch_pool_spectral(const float* y, float* out, int B, int S, int N, hipStream_t st);   // y [B][S N][96] -> out [B][96][N]
int launch_scene_embed_finalize(const SceneEmbedArgs& a, hipStream_t st);

// msst_attn_maps.hip (msst_attn_maps): the fp32 attention probabilities of one block from its input, per sequence or averaged over a
// sample's sequences; one workgroup per (sample, head)
int launch_attn_maps(const float* x, const float* ln_g, const float* ln_b, const float* wqkv, float* maps, long sample_stride,
                     int mode, int B, int S, int N, int heads, int reduce, hipStream_t st);

// msst_knn.hip (msst_knn_topk, msst_knn_vote): the k most similar bank rows of every query under a total order (fp32 MFMA similarity
// with the selection fused behind it, bank slices merged without atomics) and the weighted vote of their labels
long knn_scratch_bytes(long Q, long M, int k, int splits);
int launch_knn_topk(const float* bank, long M, const float* queries, int q_layout, long Q, long plane, int k, int splits,
                    int32_t* nbr_idx, float* nbr_sim, void* scratch, hipStream_t st);
int launch_knn_vote(const int32_t* nbr_idx, const float* nbr_sim, const int32_t* labels, long Q, int k, int n_classes,
                    float temperature, float* votes, int vote_layout, long plane, int64_t* classes, hipStream_t st);

// msst_probe.hip (msst_probe_grad, msst_probe_update, msst_probe_fwd): the linear probe on cached features -- LayerNorm(96) -> Linear
// -> weighted cross entropy, per-workgroup gradient partials without atomics, torch.optim.Adam on the device, and the forward
long probe_scratch_floats(long rows, int nc);
int launch_probe_grad(const float* x, const int32_t* labels, const float* class_w, const float* theta, long row0, long rows, int nc,
                      float* slab, hipStream_t st);
int launch_probe_update(const float* slab, long rows, int nc, float* theta, float* m, float* v, int32_t* step, double lr, double beta1,
                        double beta2, double eps, double weight_decay, float* history_row, float* grad_out, int apply, hipStream_t st);
int launch_probe_fwd(const float* x, int x_layout, long Q, long plane, const float* theta, int nc, float* logits, int out_layout,
                     int64_t* classes, hipStream_t st);

// msst_kmeans.hip (msst_kmeans_assign, msst_kmeans_update, msst_kmeans_pick): k-means on frozen features -- scores and per-cluster sums
// on the fp32 MFMA, per-workgroup partials without atomics, the centroid update, and the k-means++ draw
long kmeans_scratch_floats(long rows, int k);
int launch_kmeans_assign(const float* x, int x_layout, long rows, long plane, const float* centroids, const float* bias, int k, int metric,
                         int32_t* assign, float* dist, int64_t* classes, float* slab, hipStream_t st);
int launch_kmeans_update(const float* slab, long rows, int k, int metric, float* centroids, float* bias, int32_t* counts, float* shift,
                         float* history_row, hipStream_t st);
int launch_kmeans_pick(const float* x, long rows, const float* dist, const float* slab, int j, int metric, unsigned seed, float* centroids,
                       float* bias, int32_t* seed_rows, hipStream_t st);

// msst_pca.hip (msst_feat_moments, msst_feat_moments_finish, msst_feat_project): mean and covariance of frozen features -- x^T x on the
// fp32 MFMA with the row as the k index, per-workgroup partials without atomics, summed in double -- and the projection of rows or a
// map onto given directions with the squared norm of the result
long feat_moments_scratch_floats(long rows);
int launch_feat_moments(const float* x, int x_layout, long rows, long plane, const float* centre, float* slab, hipStream_t st);
int launch_feat_moments_finish(const float* slab, long rows, const float* centre, int ddof, int64_t* count, float* mean, float* cov,
                               float* raw, hipStream_t st);
int launch_feat_project(const float* x, int x_layout, long rows, long plane, const float* mean, const float* components, int r, float* out,
                        int out_layout, float* sumsq, hipStream_t st);

// msst_gauss.hip (msst_gauss_score): class-conditional Gaussian scores of frozen features -- per table the whitening projection on the
// fp32 MFMA, per class the squared distance to an offset in the whitened coordinates (the class stage on the MFMA too), the argmax
// under the total order and the distance to it.  class_table is a HOST array [nc] of ids in [0, n_tables), checked by the caller
int launch_gauss_score(const float* x, int x_layout, long rows, long plane, const float* centres, const float* tables, int n_tables,
                       const int32_t* class_table, const float* offsets, const float* consts, int nc, float max_d2, int32_t* classes,
                       float* distance, float* scores, int out_layout, hipStream_t st);

// msst_gmm.hip (msst_gmm_posterior, msst_gmm_moments, msst_gmm_update): Gaussian mixtures by EM on top of launch_gauss_score -- the
// posterior of a scores table, the responsibility-weighted moments about the current means (components across blockIdx.y, per-workgroup
// partials without atomics) and the per-component M-step with a double Cholesky factorisation and triangular inverse in LDS
long gmm_scratch_floats(long rows, int k);
int launch_gmm_posterior(const float* scores, int in_layout, long rows, long plane, int k, float* lse, float* probs, int out_layout,
                         hipStream_t st);
int launch_gmm_moments(const float* x, int x_layout, long rows, long plane, const float* scores, int k, const float* centres, float* slab,
                       hipStream_t st);
int launch_gmm_update(const float* slab, long rows, int k, int cov_kind, double reg_covar, double min_count, float* centres, float* tables,
                      float* covs, float* logdet, float* consts, float* weights, float* raw, float* record, hipStream_t st);

// msst_crf.hip (msst_crf_affinity, msst_crf_step): the pairwise weights of a local dense CRF from the feature map (a tile with its halo
// in LDS once, the dots on the fp32 MFMA) and one mean-field step over the score maps.  a_tab and s_tab are HOST arrays [K];
// crf_tiles is the grid of either launch (which 0: affinity, 1: step), for the caller's range check
int launch_crf_affinity(const float* feat, const int32_t* cover, int Bs, int Hs, int Ws, int R, const float* a_tab, const float* s_tab, float g,
                        float* k, uint8_t* live, hipStream_t st);
int launch_crf_step(const float* scores, int unary, float unary_scale, const float* q_in, const float* k, const uint8_t* live, int Bs, int nc,
                    int Hs, int Ws, int R, float* q_out, int32_t* classes, const int32_t* prev_classes, int32_t* changed, hipStream_t st);
long crf_tiles(int Bs, int Hs, int Ws, int which);

// msst_slic.hip (msst_slic_assign, msst_slic_update, msst_slic_pool, msst_slic_pool_finish, msst_slic_broadcast): SLIC superpixels of the
// feature map in the grid form -- an 8 x 8 pixel block against the at most 16 centres of its window on the fp32 MFMA, per-block partial
// sums without float atomics, the ordered per-centre update -- and the per-superpixel means, region classes and class map of any map.
// slic_blocks is the grid of the per-block launches, for the caller's range check; a slab holds slic_scratch_floats(.., C) floats
long slic_blocks(int Bs, int Hs, int Ws);
long slic_scratch_floats(int Bs, int Hs, int Ws, int C);
int launch_slic_assign(const float* feat, const int32_t* cover, int Bs, int Hs, int Ws, int step, float hl, const float* centroids,
                       const float* offsets, const float* bias, const int32_t* counts, int64_t* labels, const int64_t* prev_labels, int32_t* moved,
                       float* best, float* slab, hipStream_t st);
int launch_slic_update(const float* slab, int Bs, int Hs, int Ws, int step, float* centroids, float* offsets, float* bias, int32_t* counts,
                       int32_t* empty, hipStream_t st);
int launch_slic_pool(const float* map, const int64_t* labels, int Bs, int C, int Hs, int Ws, int step, float* slab, hipStream_t st);
int launch_slic_pool_finish(const float* slab, int Bs, int C, int Hs, int Ws, int step, float* table, int64_t* region_classes, hipStream_t st);
int launch_slic_broadcast(const int64_t* labels, const int64_t* region_classes, int Bs, int Hs, int Ws, int step, int64_t* classes, hipStream_t st);

// msst_regions.hip (msst_regions_label, msst_regions_merge): connected regions of an int64 map -- a union-find per 16 x 16 tile in LDS,
// unions across the tile borders with integer atomicMin on a parent array, a flatten that counts the sizes at the roots -- and one
// simultaneous merge round on top of it (the sieve; SLIC's connectivity pass).  regions_tiles is the grid of the per-tile launches, for
// the caller's range check; the scratch holds regions_scratch_bytes bytes and starts with the error word, which the launches only raise
long regions_tiles(int Bs, int Hs, int Ws);
long regions_scratch_bytes(int Bs, int Hs, int Ws);
int launch_regions_label(const int64_t* values, int Bs, int Hs, int Ws, int connectivity, int64_t* labels, int32_t* sizes, int32_t* count,
                         void* scratch, hipStream_t st);
int launch_regions_merge(const int64_t* values, const int64_t* labels, const int32_t* sizes, int Bs, int Hs, int Ws, int connectivity, int mode,
                         int min_size, int step, int64_t* values_out, int32_t* history, void* scratch, hipStream_t st);

// msst_mask.hip (msst_draw_masks): the SimMIM token mask, gather indices and the gather's token-CSR of global rows row0 .. row0 + rows - 1
// from a counter hash; one workgroup per row
struct MaskDrawArgs {
    uint8_t* mask;       // [rows][S N] (1 = masked)
    int32_t* idx;        // [rows][K]
    int32_t* csr_ptr;    // [rows][S N + 1]
    int32_t* csr_pos;    // [rows][K]
    unsigned seed;
    long row0;
    int rows, S, N, K, mode;
    int side, rand_size, scale, mask_count;   // MSST_MASK_BLOCK / MSST_MASK_TUBE: side = rand_size * scale, side * side = N
};
int launch_draw_masks(const MaskDrawArgs& a, hipStream_t st);

}  // namespace msst
