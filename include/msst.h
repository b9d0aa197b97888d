/* libmsst -- C-ABI of the MI355X-native MaskedSST masked-pretraining hot path.
 *
 * The reference (HSG-AIML/MaskedSST) is pure Python/PyTorch and has NO FFI of its own; its
 * boundary for this path is the nn.Module surface of
 *     src/vit_spatial_spectral.py:256-564  (ViTSpatialSpectral)
 *     src/vit_simmim_original.py:139-340   (SimMIMSpatialSpectral)
 * which maskedsst_amd/ mirrors in Python.  This header is the build-defined C boundary underneath
 * that mirror: every entry point states which reference lines it replaces, and
 * INTEGRATION.md shows the ctypes stub a reference maintainer would add.
 *
 * Rules: plain pointers and sizes only (no torch types); every pointer is DEVICE memory owned by
 * the caller unless marked "host"; calls only enqueue work on `stream` (a hipStream_t passed as
 * void*), never synchronise, never allocate; returns 0 or a negative MSST_ERR_* / positive
 * hipError_t code, never throws; re-entrant: the compute entry points keep no state between calls and
 * read no environment (a thread-local error string; idempotent once-flags for kernel attributes; the
 * opt-in msst_profile_* state is mutex-guarded and, when disabled, costs one relaxed atomic load).  All activations are fp32 [tokens][96] in the reference token order 'b (c h w) d'.
 * The kernels are specialised for dim = 96, dim_head = 64, mlp_dim = 64 (configs/config.yaml:19-22
 * of the reference); heads, depth, bands, batch are runtime.
 */
#ifndef MSST_H
#define MSST_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSST_VERSION 109
#define MSST_DIM 96
#define MSST_DIM_HEAD 64
#define MSST_MLP 64

#define MSST_PREC_F32 0  /* exact fp32 MFMA (parity mode)               */
#define MSST_PREC_BF16 1 /* bf16 MFMA operands, fp32 accumulate/residual */

/* Kernel-selection flags, OR-ed into the `prec` argument of msst_block_fwd / msst_block_bwd (bits 8..23).  0 selects the
 * tuned kernels; the others exist for the cross-kernel agreement tests and A/B studies.  They are explicit arguments:
 * the library never reads the environment and keeps no per-call state. */
#define MSST_KERNEL_GENERIC (16 << 8)    /* generic template kernels also in bf16 (fwd and attention bwd)   */
#define MSST_KERNEL_FWD_4WAVE (64 << 8)  /* bf16 forward: tuned 4-wave kernel instead of head-per-wave      */
#define MSST_X1_BF16 (1024 << 8)         /* the saved mid-residual rows x1 are bf16 instead of fp32: msst_block_fwd writes them so (role-split bf16 forward only:
                                            8 heads, no MSST_KERNEL_* flag; MSST_ERR_UNSUPPORTED otherwise), msst_block_bwd / _chain read x1 and x1_prev so (bf16
                                            kernels only).  A quarter of the forward's writes and 8 % of the fused row-local backward's reads less; the LN2 statistics
                                            of the backward are then those of the rounded rows (parity: tests/test_gpu_backward.py::test_bf16_x1_rows) */
#define MSST_FWD_HALF (4096 << 8)         /* msst_block_fwd / msst_block_fwd_stack, role-split bf16 forward only (MSST_VERSION 104): the forward's GEMM operands -- LN rows,
                                            weights (MsstBlockWeights.wqkv_h ...), q / k / v, probabilities, attention output, GELU output -- are rounded to IEEE
                                            half (11 significant bits) instead of bf16 (8) and multiplied by v_mfma_f32_16x16x32_f16 (same rate).  Everything
                                            else is unchanged: fp32 accumulation / softmax / LayerNorm / residual stream, bf16 rows saved for the backward, bf16
                                            backward.  Why: the bf16 forward's loss error against the fp32 reference (2.6e-4 on the Houston-shape anchor) is
                                            systematic and owned by the rounding of the WEIGHTS (tools/bf16_error_table.py); with half operands it is 7e-6.  Every
                                            operand of the forward is a LayerNorm row, a weight, a probability or a bounded activation: inside half's range */
#define MSST_LSE_RENORM (8192 << 8)       /* msst_block_bwd / _chain (MSST_VERSION 104): lse_saved comes from a forward whose scores are not the backward's own -- the
                                            half-operand forward (MSST_FWD_HALF) against the bf16 recomputation here.  The two-head attention backward then uses lse
                                            as the exponent offset only and normalises every row by its own sum (p = softmax of ITS scores exactly, one reduction
                                            more); without the flag p = exp2(s c - lse) as saved.  Always pass it for blocks run with MSST_FWD_HALF */
#define MSST_LN1_FROM_XN (2048 << 8)      /* msst_block_bwd_chain (MSST_VERSION 104): the fused LN1 + MLP launch takes xhat of LN1 from the saved bf16 LN1 rows and
                                            the saved rstd -- xhat = (xn_saved - ln1_b) / ln1_g, rstd = the tail of lse_saved (MSST_SAVED_RSTD) -- instead of
                                            re-reading and re-normalising the fp32 block input x: 192 bytes per token less of 2304.  The caller sets it only when
                                            every ln1_g is safely away from 0 and |ln1_b / ln1_g| is moderate (the division amplifies the rows' bf16 rounding by
                                            1 + |b / g| / |xhat|; maskedsst_amd/engine.py: max |b / g| <= 12); needs xn_saved and lse_saved */
#define MSST_BWD_DEFER_REDUCE (512 << 8) /* msst_block_bwd_chain: leave the partial-gradient slabs of this call unreduced (msst_block_bwd_reduce does a run of calls in one launch) */
#define MSST_KERNEL_ATTN_R3 (128 << 8)   /* bf16 attention backward: one head per workgroup (msst_bwd3.hip) instead of two (msst_bwd4.hip) */

#define MSST_MODE_SPATIAL 0  /* sequences = (b, c), N tokens each, contiguous            */
#define MSST_MODE_SPECTRAL 1 /* sequences = (b, n), S tokens each, stride N*96 floats    */

#define MSST_ERR_UNSUPPORTED (-2)
#define MSST_ERR_BADARG (-3)

int msst_version(void);
const char* msst_last_error(void);

/* One weight-prep job: dst = (elem)src, optionally transposed.  elem = float (F32) or bf16. */
typedef struct MsstPrepJob {
    const float* src; /* [rows][cols] fp32 master weight          */
    void* dst;        /* [rows][cols] or [cols][rows] (transpose) */
    int32_t rows, cols, transpose;
    int32_t pack;     /* bf16 only: 0 = 16-row x 32-k operand fragments (16x16x32 MFMA; destination rows % 16 == 0 and k % 32 == 0),
                         1 = 32-row x 16-k fragments (32x32x16 MFMA; destination rows % 32 == 0 and k % 16 == 0); + MSST_PREP_HALF (256, MSST_VERSION 104): the destination
                         elements are IEEE half instead of bf16 (same fragment layout; the fp16-operand forward, MSST_FWD_HALF).
                         Any other value: the job is skipped. */
    int32_t scale_rows; /* the first scale_rows SOURCE rows are multiplied by `scale` (0: none).  The round-3 attention backward   */
    float scale;        /* wants the q and k blocks of to_qkv^T pre-multiplied by dim_head^-0.5 (2^-3: exact in bf16).             */
} MsstPrepJob;

#define MSST_PREP_HALF 256
/* Converts / transposes all matrices of the model into operand layout in ONE launch.
 * `jobs` is a DEVICE array. max_elems = max(rows*cols) over jobs.  job_bytes = sizeof(MsstPrepJob) of the CALLER's header: a
 * table laid out by another revision is refused (MSST_ERR_BADARG) instead of being read mis-strided.  err_flag (optional, one
 * zeroed int32 in device memory): the kernel ORs in 1 for a job with a bad pack / shape and 2 for a bf16 / half job whose
 * destination is not whole fragments (pack = 0: destination rows % 16 == 0 and k % 32 == 0; pack = 1: rows % 32 == 0 and
 * k % 16 == 0; fp32 destinations take any shape) -- such jobs are skipped, their destinations stay unwritten; the host cannot
 * see the table, so a caller that builds it should read the word back once after its first call. */
int msst_prep_weights(const MsstPrepJob* jobs, int njobs, int job_bytes, int max_elems, int prec, int32_t* err_flag, void* stream);

/* Operand-layout weights of one transformer block (device pointers).
 * Replaces the parameters of reference vit_spatial_spectral.py:85-97 (one Transformer layer). */
typedef struct MsstBlockWeights {
    uint64_t struct_bytes; /* = sizeof(MsstBlockWeights): a caller built against another revision of this header is refused
                              (MSST_ERR_BADARG) instead of being read past the end of its struct */
    const void* wqkv;  /* [3*H*64][96]  to_qkv.weight, rows q|k|v, head-major */
    const void* wout;  /* [96][H*64]    to_out.0.weight                        */
    const void* w1;    /* [64][96]      net.0.weight                           */
    const void* w2;    /* [96][64]      net.3.weight                           */
    const void* wqkvT; /* [96][3*H*64]  (backward)                             */
    const void* woutT; /* [H*64][96]                                           */
    const void* w1T;   /* [96][64]                                             */
    const void* w2T;   /* [64][96]                                             */
    const float* ln1_g; const float* ln1_b; const float* bo;
    const float* ln2_g; const float* ln2_b; const float* b1; const float* b2;
    /* bf16 only, optional (null: msst_block_bwd runs the template attention backward): the three matrices the round-3
     * attention backward feeds to 32x32x16 MFMAs, fragment-packed with MsstPrepJob.pack = 1 */
    const void* wqkv32;  /* [3*H*64][96]  */
    const void* woutT32; /* [H*64][96]    */
    const void* wqkvT32; /* [96][3*H*64], pack = 1, scale_rows = 2*H*64, scale = dim_head^-0.5 (q and k blocks carry the softmax scale) */
    /* MSST_VERSION 104, bf16 only, optional (null: MSST_FWD_HALF is refused): the four forward matrices as IEEE half, pack = 0 | MSST_PREP_HALF
     * -- operands of the fp16-operand forward (same layout as wqkv / wout / w1 / w2) */
    const void* wqkv_h; const void* wout_h; const void* w1_h; const void* w2_h;
} MsstBlockWeights;

/* a1+a2+a3+a5: BlockwisePatchEmbedding.to_patch/.embed (vit_spatial_spectral.py:197-222), position
 * add and mask-token select (vit_simmim_original.py:236-249,285).
 * img [B][S*P][N]; mask [B][T] bytes (all zero for the classification path);
 * pos_split == 0: pos_a = learned table [T][96] (pos_embedding[0,:T]);
 * pos_split  > 0: pos_a = pos_embed [N][pos_split], pos_b = channel_embed [S][96-pos_split]
 *                 (get_pos_embeddings, vit_spatial_spectral.py:501-516).  out [B][T][96].
 * emb_dropout_p > 0: embedding dropout on (token + pos) (forward_features, :530; classification path). */
int msst_tokenize_fwd(const float* img, const float* pre_g, const float* pre_b, const float* w_emb,
                      const float* b_emb, const float* post_g, const float* post_b, const float* pos_a,
                      const float* pos_b, int pos_split, const float* mask_token, const uint8_t* mask,
                      float* out, int B, int S, int N, int P, float emb_dropout_p, uint32_t seed, void* stream);

/* MSST_VERSION 105: scene inference (sliding windows).  Replaces the window loops of the reference's inference_example.ipynb (cell
 * "for x in range(0, 64, eff_size): for y in range(0, 64, eff_size): ... model(img).argmax(dim=1)") and of validate_downstream
 * (src/utils.py:497-541): there every window is a .narrow() copy and a model(window) call of its own; here one tokenizer launch reads
 * any number of windows of many scenes straight out of the scene tensor, the block / head kernels run on all of them as one batch,
 * and msst_scene_assemble writes the scene-shaped maps.
 * Windows: window i of a call is window win0 + i, row-major over (scene, window row r, window column q) of the grid
 * nr = (Hs - window) / stride + 1 rows by nq = (Ws - window) / stride + 1 columns; window (r, q) has its origin at (r stride, q stride)
 * -- the notebook's origins 0, s, 2s, ... (H outer, W inner), keeping only windows with origin + window <= the scene size.
 * Where our semantics differ from the reference: overlapping windows (stride < window) are AVERAGED (mean of the logits of every
 * window covering a pixel; the notebook lets the last window's argmax overwrite); pixels no window covers get class -1 (the configs'
 * ignored_label) and logit 0 (the notebook leaves 0, a real class); every window with origin + window <= size is kept
 * (validate_downstream's `x + image_size >= 64` also drops the last window row); scenes of any size (the notebook: 64 x 64).
 *
 * msst_tokenize_scene_fwd: msst_tokenize_fwd (no mask, position table(s) added, no embedding dropout) of windows win0 .. win0 + nwin - 1
 * of scene [Bs][S*P][Hs][Ws] (fp32, contiguous): out [nwin][S*window*window][96], the values msst_tokenize_fwd gives for the copied
 * windows.  pos_a / pos_b / pos_split as there.  1 <= stride <= window <= Hs, Ws; window * window <= 64 and P <= 16
 * (MSST_ERR_UNSUPPORTED otherwise; for P != 10 or window != 8 also nwin <= 65535). */
int msst_tokenize_scene_fwd(const float* scene, const float* pre_g, const float* pre_b, const float* w_emb,
                            const float* b_emb, const float* post_g, const float* post_b, const float* pos_a,
                            const float* pos_b, int pos_split, float* out, int Bs, int Hs, int Ws, int window, int stride,
                            long win0, int nwin, int S, int P, void* stream);

/* Training on the windows of a tile (the reference's shifting_window finetuning: train_step, src/utils.py:608-613, stacks the
 * non-overlapping s x s windows of every tile along the batch axis with stack_image_batch, :451-474, and trains on all of them).
 * Additive under MSST_VERSION 109.  The stacked batch is never built: the windows, numbered as above -- stack_image_batch's
 * '(b h w)' order is that numbering with stride = window -- are read out of the resident tiles.
 *
 * msst_tokenize_scene_fwd_train: msst_tokenize_scene_fwd with the embedding dropout of msst_tokenize_fwd.  A dropout element is
 * addressed by its place in out (window i of the call is sample i of the stacked batch): for every (emb_dropout_p, seed) out is
 * bit-identical to msst_tokenize_fwd on the copied windows.
 * msst_tokenize_scene_bwd: msst_tokenize_bwd of those windows (B = nwin), dx0 [nwin][S*window*window][96]; no mask and no mask-token
 * gradient (the classification path masks nothing).  slab, nchunk, the gradient outputs, pos_split and the dropout regeneration as
 * there; for equal nchunk every gradient is bit-identical to msst_tokenize_bwd on the copied windows (same kernels, same summation
 * order, only the pixel addresses differ).  nwin >= 1.
 * Both check their arguments before anything is enqueued: MSST_ERR_BADARG for a size below 1 (nwin = 0 is an empty forward call), a
 * null required pointer (dpos_a may be null as in msst_tokenize_bwd) or windows beyond win0 + nwin <= Bs nr nq; MSST_ERR_UNSUPPORTED
 * outside 1 <= stride <= window <= Hs, Ws, window * window <= 64, P <= 16 (forward, for P != 10 or window != 8: also nwin <= 65535). */
int msst_tokenize_scene_fwd_train(const float* scene, const float* pre_g, const float* pre_b, const float* w_emb,
                                  const float* b_emb, const float* post_g, const float* post_b, const float* pos_a,
                                  const float* pos_b, int pos_split, float* out, int Bs, int Hs, int Ws, int window, int stride,
                                  long win0, int nwin, int S, int P, float emb_dropout_p, uint32_t seed, void* stream);
int msst_tokenize_scene_bwd(const float* scene, const float* pre_g, const float* pre_b, const float* w_emb,
                            const float* b_emb, const float* post_g, const float* post_b, const float* dx0, float* slab,
                            int nchunk, float* dpre_g, float* dpre_b, float* dw_emb, float* db_emb, float* dpost_g,
                            float* dpost_b, float* dpos_a, float* dpos_b, int pos_split, int Bs, int Hs, int Ws, int window,
                            int stride, long win0, int nwin, int S, int P, float emb_dropout_p, uint32_t seed, void* stream);

/* Training and prediction on windows at listed scene positions (the reference's pixelwise and random-position sampling of a
 * sparsely labelled scene, src/data_houston2018.py:303-329: one window per labelled pixel, or windows at random positions).
 * Additive under MSST_VERSION 109.  The kernels are those of msst_tokenize_scene_fwd_train / msst_tokenize_scene_bwd with the
 * origin of a window read from a table instead of computed from its number: origins is a device table [nwin][3] of int32 --
 * scene index, y0, x0 of the window's top-left pixel -- and sample i of the call is the window at origins[i].  Windows may overlap,
 * repeat and come in any order; the scene is only read.  The C layer cannot see the table's values: THE CALLER GUARANTEES
 * 0 <= scene < Bs, 0 <= y0 <= Hs - window and 0 <= x0 <= Ws - window for every row (a row outside reads outside the scene).
 *
 * msst_tokenize_at_fwd: out [nwin][S*window*window][96]; a dropout element is addressed by its place in out, so for every
 * (emb_dropout_p, seed) out is bit-identical to msst_tokenize_fwd on the copied windows, and to msst_tokenize_scene_fwd_train when
 * the table lists a regular grid in grid order.
 * msst_tokenize_at_bwd: msst_tokenize_bwd of those windows (B = nwin): slab, nchunk, the gradient outputs, pos_split and the dropout
 * regeneration as for msst_tokenize_scene_bwd; for equal nchunk every gradient is bit-identical to msst_tokenize_bwd on the copied
 * windows.  Parameter gradients only: the scene is never written.  nwin >= 1.
 * Both check their arguments before anything is enqueued: MSST_ERR_BADARG for a size below 1 (nwin = 0 is an empty forward call,
 * nwin < 0 an error) or a null required pointer (dpos_a may be null as in msst_tokenize_bwd); MSST_ERR_UNSUPPORTED outside
 * window <= Hs, Ws, window * window <= 64, P <= 16 (forward, for P != 10 or window != 8: also nwin <= 65535 per call). */
int msst_tokenize_at_fwd(const float* scene, const int32_t* origins, const float* pre_g, const float* pre_b, const float* w_emb,
                         const float* b_emb, const float* post_g, const float* post_b, const float* pos_a, const float* pos_b,
                         int pos_split, float* out, int Bs, int Hs, int Ws, int window, int nwin, int S, int P,
                         float emb_dropout_p, uint32_t seed, void* stream);
int msst_tokenize_at_bwd(const float* scene, const int32_t* origins, const float* pre_g, const float* pre_b, const float* w_emb,
                         const float* b_emb, const float* post_g, const float* post_b, const float* dx0, float* slab, int nchunk,
                         float* dpre_g, float* dpre_b, float* dw_emb, float* db_emb, float* dpost_g, float* dpost_b, float* dpos_a,
                         float* dpos_b, int pos_split, int Bs, int Hs, int Ws, int window, int nwin, int S, int P,
                         float emb_dropout_p, uint32_t seed, void* stream);

/* SimMIM pre-training on windows at listed scene positions (SimMIMSpatialSpectral.forward_at / forward_windows: the masked loss of
 * windows read straight out of resident tiles, no stacked copy).  Additive under MSST_VERSION 109: no struct and no existing
 * signature changes.  origins, the scene and THE CALLER'S GUARANTEE of the table's ranges: as for msst_tokenize_at_fwd.
 *
 * msst_tokenize_at_fwd_masked: msst_tokenize_at_fwd plus mask_token [96] and mask [nwin][T] (uint8, 1 = masked), T = S window window,
 * in WINDOW coordinates: the layout of msst_tokenize_fwd's mask.  No embedding dropout (the SimMIM path has none).  out is
 * bit-identical to msst_tokenize_fwd on the copied windows with the same mask.
 * msst_tokenize_at_bwd_masked: msst_tokenize_at_bwd plus that mask and dmask_token [96] (may be null, as in msst_tokenize_bwd): a
 * masked token's gradient goes to the mask token and the position table only.  For equal nchunk every gradient output, dmask_token
 * included, is bit-identical to msst_tokenize_bwd on the copied windows.  nwin >= 1.
 * msst_head_at_fwd: msst_head_fwd of nwin windows with its reconstruction target read from the scene:
 * target = scene[s][c P + p][y0 + n / window][x0 + n % window] for masked token idx = c N + n of the window at (s, y0, x0).  The same
 * kernel body, grid, partial sums and final reduction: loss, dpred, pred and partial have the bits of msst_head_fwd on the copied
 * windows.  msst_head_bwd takes its results as they are (it never reads the image).  nwin >= 1, 1 <= K <= T.
 * All three check their arguments before anything is enqueued, in the order of msst_tokenize_at_fwd: MSST_ERR_BADARG for a size below
 * 1 (nwin = 0 is an empty call of the forward tokenizer only, nwin < 0 always an error); MSST_ERR_UNSUPPORTED outside window <= Hs, Ws,
 * window * window <= 64, P <= 16 (the head: also nwin <= 65535; the forward tokenizer: that for P != 10 or window != 8);
 * MSST_ERR_BADARG for a null required pointer (pred, dpos_a and dmask_token may be null) or K > T. */
int msst_tokenize_at_fwd_masked(const float* scene, const int32_t* origins, const float* pre_g, const float* pre_b, const float* w_emb,
                                const float* b_emb, const float* post_g, const float* post_b, const float* pos_a, const float* pos_b,
                                int pos_split, const float* mask_token, const uint8_t* mask, float* out, int Bs, int Hs, int Ws,
                                int window, int nwin, int S, int P, void* stream);
int msst_tokenize_at_bwd_masked(const float* scene, const int32_t* origins, const float* pre_g, const float* pre_b, const float* w_emb,
                                const float* b_emb, const float* post_g, const float* post_b, const uint8_t* mask, const float* dx0,
                                float* slab, int nchunk, float* dpre_g, float* dpre_b, float* dw_emb, float* db_emb, float* dpost_g,
                                float* dpost_b, float* dpos_a, float* dpos_b, int pos_split, float* dmask_token, int Bs, int Hs, int Ws,
                                int window, int nwin, int S, int P, void* stream);
int msst_head_at_fwd(const float* y, const float* scene, const int32_t* origins, const int32_t* idx, const float* w_pix,
                     const float* b_pix, int per_block, float* dpred, float* pred /*optional*/, float* partial, float* loss, int Bs,
                     int Hs, int Ws, int window, int nwin, int S, int P, int K, void* stream);

/* D4 augmentation of listed windows: flips and quarter turns applied where the window's address is formed (forward_at(..., orient=),
 * SimMIMSpatialSpectral.forward_at(..., orient=), predict_at(..., tta="d4")).  Additive under MSST_VERSION 109: no struct and no
 * existing signature changes; the five entry points above launch the kernels they launched before.
 *
 * orient is a device table [nwin] of uint8, one orientation code per row of origins: o = k + 4 f, k in 0 .. 3, f in 0 .. 1.  Sample i
 * of the call is the window w at origins[i] flipped left to right when f, then turned k quarter turns counter-clockwise --
 * torch.rot90(torch.flip(w, (-1,)) if f else w, k, (-2, -1)); code 0 is the window as it lies.  Pixel (i, j) of the oriented window is
 * read at origin + start + i * step_i + j * step_j with the steps in {+-1, +-Ws}: no copy, no further launch, the same arithmetic.
 * Everything else sees the ORIENTED window: token n is its pixel n, so position row, mask byte (window coordinates of the oriented
 * window), dropout element, dx0 row and idx entry are those of the oriented copy, and every output is bit-identical to the
 * un-oriented entry point's counterpart (msst_tokenize_fwd / _bwd / msst_head_fwd) on the oriented copies.  THE CALLER GUARANTEES codes
 * 0 .. 7 as it does the origins' ranges (the kernels look at the low three bits only: another value reads inside the window all the same).
 *
 * Each is its namesake without _orient plus the table, after origins; arguments, limits, outputs and the order of the argument checks
 * (before anything is enqueued) are the namesake's: MSST_ERR_BADARG for a size below 1; MSST_ERR_UNSUPPORTED outside window <= Hs, Ws,
 * window * window <= 64, P <= 16 (the head: also nwin <= 65535; the forward tokenizers: that for P != 10 or window != 8);
 * MSST_ERR_BADARG for a null required pointer, a null orient included.  The codes whose steps swap the axes (k odd) read Ws floats
 * apart along j. */
int msst_tokenize_at_fwd_orient(const float* scene, const int32_t* origins, const uint8_t* orient, const float* pre_g, const float* pre_b,
                                const float* w_emb, const float* b_emb, const float* post_g, const float* post_b, const float* pos_a,
                                const float* pos_b, int pos_split, float* out, int Bs, int Hs, int Ws, int window, int nwin, int S, int P,
                                float emb_dropout_p, uint32_t seed, void* stream);
int msst_tokenize_at_bwd_orient(const float* scene, const int32_t* origins, const uint8_t* orient, const float* pre_g, const float* pre_b,
                                const float* w_emb, const float* b_emb, const float* post_g, const float* post_b, const float* dx0,
                                float* slab, int nchunk, float* dpre_g, float* dpre_b, float* dw_emb, float* db_emb, float* dpost_g,
                                float* dpost_b, float* dpos_a, float* dpos_b, int pos_split, int Bs, int Hs, int Ws, int window, int nwin,
                                int S, int P, float emb_dropout_p, uint32_t seed, void* stream);
int msst_tokenize_at_fwd_masked_orient(const float* scene, const int32_t* origins, const uint8_t* orient, const float* pre_g,
                                       const float* pre_b, const float* w_emb, const float* b_emb, const float* post_g,
                                       const float* post_b, const float* pos_a, const float* pos_b, int pos_split,
                                       const float* mask_token, const uint8_t* mask, float* out, int Bs, int Hs, int Ws, int window,
                                       int nwin, int S, int P, void* stream);
int msst_tokenize_at_bwd_masked_orient(const float* scene, const int32_t* origins, const uint8_t* orient, const float* pre_g,
                                       const float* pre_b, const float* w_emb, const float* b_emb, const float* post_g,
                                       const float* post_b, const uint8_t* mask, const float* dx0, float* slab, int nchunk, float* dpre_g,
                                       float* dpre_b, float* dw_emb, float* db_emb, float* dpost_g, float* dpost_b, float* dpos_a,
                                       float* dpos_b, int pos_split, float* dmask_token, int Bs, int Hs, int Ws, int window, int nwin,
                                       int S, int P, void* stream);
int msst_head_at_fwd_orient(const float* y, const float* scene, const int32_t* origins, const uint8_t* orient, const int32_t* idx,
                            const float* w_pix, const float* b_pix, int per_block, float* dpred, float* pred /*optional*/, float* partial,
                            float* loss, int Bs, int Hs, int Ws, int window, int nwin, int S, int P, int K, void* stream);

/* msst_scene_assemble: adds the per-window logits win_logits [nwin][n_classes][window*window] (msst_cls_head_fwd of windows
 * win0 .. win0 + nwin - 1) into the running per-pixel sums logits [Bs][n_classes][Hs][Ws] (fp32).  The calls of one scene batch
 * must cover windows 0, 1, ... in order (any split into calls); logits needs no initialisation.  finalize != 0 (the last call, after
 * its own windows): logits = the sums divided by the number of windows covering the pixel (the plain mean), classes [Bs][Hs][Ws]
 * (int64) = the argmax over classes (ties: lowest index, as torch.argmax); uncovered pixels: logits 0, class -1.  Each pixel sums
 * its windows in window order (row, then column) without atomics: bitwise reproducible, whatever the split into calls. */
int msst_scene_assemble(const float* win_logits, long win0, int nwin, float* logits, int64_t* classes, int Bs,
                        int n_classes, int Hs, int Ws, int window, int stride, int finalize, void* stream);

/* Whole-scene SimMIM reconstruction (SimMIMSpatialSpectral.reconstruct_scene).  Additive under MSST_VERSION 109: no struct and no
 * existing signature changes.  The windows of a scene, numbered as for msst_tokenize_scene_fwd, are tokenized WITH a mask given in
 * scene coordinates, run through msst_block_fwd and msst_recon_fwd (blend = 0, null statistics) as one batch, and
 * msst_scene_recon_assemble writes the scene-shaped cube: overlapping windows averaged, as msst_scene_assemble does for logits.
 *
 * msst_tokenize_scene_fwd_masked: msst_tokenize_scene_fwd plus mask_token [96] and scene_mask [Bs][S][Hs][Ws] (uint8, non-zero =
 * masked: one byte per spectral block and pixel, i.e. per token).  Token (c, n) of the window with origin (y0, x0) is masked iff
 * scene_mask[s][c][y0 + n / window][x0 + n % window] != 0; its embedding is replaced by the mask token before the position add, as
 * msst_tokenize_fwd does.  out is bit-identical to msst_tokenize_fwd on the copied windows with the copied per-window [nwin][T]
 * masks, and with an all-zero mask to msst_tokenize_scene_fwd (tested properties; both tokenizer paths).  The limits and argument
 * checks of msst_tokenize_scene_fwd, plus MSST_ERR_BADARG for a null mask_token or scene_mask. */
int msst_tokenize_scene_fwd_masked(const float* scene, const float* pre_g, const float* pre_b, const float* w_emb,
                                   const float* b_emb, const float* post_g, const float* post_b, const float* pos_a,
                                   const float* pos_b, int pos_split, const float* mask_token, const uint8_t* scene_mask, float* out,
                                   int Bs, int Hs, int Ws, int window, int stride, long win0, int nwin, int S, int P, void* stream);

/* msst_scene_recon_assemble: the counterpart of msst_scene_assemble for pixels.  Adds the per-window predictions
 * win_recon [nwin][S P][window*window] (msst_recon_fwd with blend = 0 of windows win0 .. win0 + nwin - 1: the layout
 * msst_scene_assemble takes for logits) into the running fp32 sums cube [Bs][S P][Hs][Ws].  The calls of one scene batch must cover
 * windows 0, 1, ... in order (any split into calls); cube needs no initialisation.  Each pixel adds its windows in window order
 * (row, then column) without atomics.  finalize != 0 (the last call, after its own windows), with scene [Bs][S P][Hs][Ws] the input
 * cube and scene_mask [Bs][S][Hs][Ws] as above:
 *   a pixel covered by k >= 1 windows holds the prediction sum / k;
 *   blend != 0: every element whose token is not masked, and every pixel no window covers, gets scene's bits;
 *   blend == 0: covered pixels hold the prediction, uncovered pixels NaN (an absent value is never a made-up number);
 *   band_err [Bs][S P] DOUBLES: sum of |prediction - scene| over the band's pixels that are masked AND covered (whatever blend is),
 *     the difference formed in double; the plane's terms are added in one fixed order (thread t of 256 takes pixels t, t + 256, ...
 *     in turn, then a butterfly over each wave, then the four waves in order);  band_cnt [Bs][S P] int32: how many such pixels;
 *     both may be null (no statistics), one without the other is MSST_ERR_BADARG;
 *   cover [Bs][Hs][Ws] int32: k, the number of windows covering the pixel (0: uncovered).
 * band_err, band_cnt and cover are written by the finalizing call only.  No atomics, nothing to zero: two runs give the same bits in
 * every output, whatever the split into calls.
 * Checked before anything is enqueued, in this order: MSST_ERR_BADARG for a size below 1 (nwin = 0 is allowed); MSST_ERR_UNSUPPORTED
 * outside 1 <= stride <= window <= Hs, Ws, window * window <= 64, S <= 64, P <= 16; MSST_ERR_BADARG for a null required pointer
 * (win_recon when nwin > 0, scene, scene_mask, cube, cover), one statistics pointer without the other, or windows beyond
 * win0 + nwin <= Bs nr nq. */
int msst_scene_recon_assemble(const float* win_recon, long win0, int nwin, const float* scene, const uint8_t* scene_mask, float* cube,
                              double* band_err /*optional*/, int32_t* band_cnt /*optional*/, int32_t* cover, int Bs, int S, int P,
                              int Hs, int Ws, int window, int stride, int finalize, int blend, void* stream);

/* Whole-scene embedding maps (ViTSpatialSpectral.encode_scene).  Additive under MSST_VERSION 109: no struct and no existing signature
 * changes.  The windows of a scene, numbered as for msst_tokenize_scene_fwd, run through msst_tokenize_scene_fwd and msst_block_fwd as
 * one batch; msst_pool_spectral_fwd turns the encoder output into per-window features and msst_scene_embed_assemble writes the
 * scene-shaped feature map: overlapping windows averaged, as msst_scene_assemble does for logits.  No head runs.
 *
 * msst_pool_spectral_fwd: y [B][S N][96] (token c N + n) -> out [B][96][N],
 *   out[b][d][n] = (sum over c = 0 .. S - 1, in that order, of y[b][c N + n][d]) / (float)S
 * -- the mean over the spectral axis that the default and the pixelwise head normalise, in the window layout msst_scene_assemble and
 * msst_scene_embed_assemble take (96 in the place of n_classes).  y is read once with 16-byte loads (it must be 16-byte aligned), the
 * transpose goes through LDS, the stores are runs of N consecutive floats.  Two calls give the same bits.
 * Checked before anything is enqueued, in this order: MSST_ERR_BADARG for a size below 1; MSST_ERR_UNSUPPORTED for N > 64 or S > 64;
 * MSST_ERR_BADARG for a null or misaligned pointer. */
int msst_pool_spectral_fwd(const float* y, float* out, int B, int S, int N, void* stream);

/* msst_scene_embed_assemble: adds the per-window features win_feat [nwin][D][window*window] (windows win0 .. win0 + nwin - 1) into the
 * running fp32 sums feat [Bs][D][Hs][Ws].  The calls of one scene batch must cover windows 0, 1, ... in order (any split into calls);
 * feat needs no initialisation: a pixel starts from 0 in the call that holds its first window.  Each pixel adds its windows in window
 * order (row, then column) without atomics.  finalize != 0 (the last call, after its own windows):
 *   a pixel covered by k >= 1 windows holds sum / k in every channel; with l2norm != 0 that vector f is then divided by
 *     max(||f||_2, 1e-12) (torch.nn.functional.normalize), the squares added in the order d = 0 .. D - 1 in fp32: an all-zero pixel
 *     stays zero;
 *   a pixel no window covers holds NaN in every channel (an absent value is never a made-up number);
 *   cover [Bs][Hs][Ws] int32: k, the number of windows covering the pixel (0: uncovered).
 * cover is written by the finalizing call only.  No atomics, nothing to zero: two runs give the same bits, whatever the split.
 * Checked before anything is enqueued, in this order: MSST_ERR_BADARG for a size below 1 (nwin = 0 is allowed); MSST_ERR_UNSUPPORTED
 * outside stride <= window <= Hs, Ws, window * window <= 64, D <= 128; MSST_ERR_BADARG for a null required pointer (win_feat when
 * nwin > 0, feat, cover when finalize != 0) or windows beyond win0 + nwin <= Bs nr nq. */
int msst_scene_embed_assemble(const float* win_feat, long win0, int nwin, float* feat, int32_t* cover, int Bs, int D, int Hs, int Ws,
                              int window, int stride, int finalize, int l2norm, void* stream);

/* Attention maps (ViTSpatialSpectral.attention_maps).  Additive under MSST_VERSION 109: no struct and no existing signature changes.
 * The probabilities P = softmax(q k^T dim_head^-0.5) of ONE block, q = LN1(x) Wq^T, k = LN1(x) Wk^T (LayerNorm eps 1e-5), rows =
 * queries, columns = keys: the reference's `attn` (vit_spatial_spectral.py:67-74) before dropout, recomputed from the block's INPUT x
 * [B][T][96] (the residual stream, T = S N).  A sequence and its length L are those of msst_block_fwd:
 *   MSST_MODE_SPATIAL:  sequence (b, c), L = N, G = S sequences per sample;  MSST_MODE_SPECTRAL: sequence (b, n), L = S, G = N.
 *   reduce = MSST_ATTN_PER_SEQ:  maps[b sample_stride + ((g heads + h) L + i) L + j], g in that order;
 *   reduce = MSST_ATTN_MEAN_SEQ: maps[b sample_stride + (h L + i) L + j] = (sum over g = 0 .. G - 1, in that order from 0) / (float)G.
 * wqkv is the fp32 master to_qkv.weight [3 heads 64][96], rows q | k | v head-major; only the q and k rows are read.  Arithmetic is
 * fp32 throughout (v_mfma_f32_16x16x4_f32), independent of the model's precision and of msst_prep_weights.  One workgroup per
 * (sample, head): no atomics, nothing to zero, two calls give the same bits, and a sample's maps have the same bits whatever batch it
 * sits in and whatever its index there.  Floats of maps outside the samples' maps (sample_stride beyond one sample) are not written.
 * Checked before anything is enqueued, in this order: MSST_ERR_BADARG for a size below 1; MSST_ERR_UNSUPPORTED for N > 64, S > 64 or
 * heads > 16; MSST_ERR_BADARG for mode or reduce outside {0, 1}, a null pointer, x or maps not 16-byte aligned, or sample_stride
 * smaller than one sample's maps. */
#define MSST_ATTN_PER_SEQ 0
#define MSST_ATTN_MEAN_SEQ 1
int msst_attn_maps(const float* x, const float* ln_g, const float* ln_b, const float* wqkv, float* maps, long sample_stride, int mode,
                   int B, int S, int N, int heads, int reduce, void* stream);

/* kNN evaluation of frozen features (maskedsst_amd/knn.py: knn_classify, ViTSpatialSpectral.knn_predict_scene).  Additive under
 * MSST_VERSION 109: no struct and no existing signature changes.  The weighted k-nearest-neighbour classifier over a bank of
 * labelled features (Wu et al. 2018), two launches: msst_knn_topk finds every query's neighbours, msst_knn_vote turns them into votes.
 *
 * msst_knn_topk.  Similarity s(q, m) = sum over d = 0 .. 95 of query[d] * bank[m][d] on v_mfma_f32_16x16x4_f32, d ascending from a
 * zero accumulator: the fp32 fmaf chain in that order, the same bits wherever the pair lands in a tile, a workgroup or a bank slice.
 * dim is the feature width and must be 96 (the encoder's).  bank [M][96] row-major, 16-byte aligned.  Queries:
 *   q_layout = 0: rows [Q][96];
 *   q_layout = 1: the encode_scene map [Q / plane][96][plane] read in place -- query b plane + p reads queries[(b 96 + d) plane + p].
 * The neighbours of a query are the first k bank rows under ONE total order -- similarity descending, then bank index ascending --
 * stored in that order: nbr_idx [Q][k] (int32), nbr_sim [Q][k].  With M < k the tail holds index -1 and similarity -inf; a query
 * with a NaN in any channel (an uncovered pixel of encode_scene) holds that in every slot.  The bank is walked in `splits` slices of
 * whole 64-row tiles by different workgroups (splits = 0: chosen from (Q, M) only; more slices than tiles: one per tile); with more
 * than one slice the partial lists go to scratch (msst_knn_scratch_bytes(Q, M, k, splits) bytes, 16-byte aligned; 0 bytes and a null
 * pointer for splits = 1) and are merged under the same order.  The order is total and the similarities do not depend on the slice,
 * so every output has the same bits for every splits, in every call, and for a query whatever batch it sits in.  No atomics; no
 * output needs initialising.  Queries run in chunks of 32,768 inside the call, which re-use the scratch in stream order.
 * msst_knn_scratch_bytes is monotone in every argument for splits >= 1; for splits = 0 it bounds what the automatic choice needs.
 *
 * msst_knn_vote.  w_j = exp((s_j - s_1) / temperature) relative to the query's best neighbour (w_1 = 1, nothing overflows, the
 * argmax does not depend on the feature scale); temperature = 0: w_j = 1.  votes[q][c] = sum of w_j over the neighbours with
 * bank_labels[index] == c, added in fp32 in rank order j = 1 .. k (a label outside [0, n_classes) votes for nothing);
 * classes[q] (int64) = the argmax, ties to the lowest class, -1 for a query without neighbours (index -1 in slot 0), whose votes are
 * all 0.  vote_layout = 0: votes [Q][n_classes];  vote_layout = 1: votes [Q / plane][n_classes][plane], a scene's vote map in the
 * layout of predict_scene's logits.  plane is read in layout 1 only.
 *
 * Checked before anything is enqueued, in this order: MSST_ERR_BADARG for a size below 1 (M, dim, n_classes; Q < 0; splits < 0 --
 * Q = 0 is allowed and launches nothing); MSST_ERR_UNSUPPORTED outside dim == 96, 1 <= k <= 64, n_classes <= 128, splits <= 64, and
 * Q, M <= 2^31 - 1; MSST_ERR_BADARG for a layout outside {0, 1}, in layout 1 a plane below 1 or not dividing Q, a negative (or NaN)
 * temperature, a null or misaligned pointer (bank and scratch 16 bytes, classes 8, the others 4), a scratch_bytes below
 * msst_knn_scratch_bytes. */
long msst_knn_scratch_bytes(long Q, long M, int k, int splits);
int msst_knn_topk(const float* bank, long M, int dim, const float* queries, int q_layout, long Q, long plane, int k, int splits,
                  int32_t* nbr_idx, float* nbr_sim, void* scratch, long scratch_bytes, void* stream);
int msst_knn_vote(const int32_t* nbr_idx, const float* nbr_sim, const int32_t* bank_labels, long Q, int k, int n_classes,
                  float temperature, float* votes, int vote_layout, long plane, int64_t* classes, void* stream);

/* The linear probe on cached features (maskedsst_amd/probe.py: fit_linear_probe, ViTSpatialSpectral.probe_predict_scene).  Additive
 * under MSST_VERSION 109.  Multinomial logistic regression through a trainable LayerNorm(96, eps 1e-5) with torch.optim.Adam on a bank
 * x [M][96] of frozen features (encode_scene(normalize=False) rows).  theta = [gamma 96 | beta 96 | W nc x 96 | b nc] fp32: the layout
 * of the mlp_head segment of the flat parameter buffer, so a probe can train a model's head where it lies.  A step is two launches
 * and no host synchronisation; nothing uses atomics and every output has the same bits in every call.
 *
 * msst_probe_grad.  Rows [row0, row0 + rows) of x (16-byte aligned) with labels [M] (int32; a label outside [0, nc) weighs nothing)
 * and class_w [nc] (null: all 1).  Per row: two-pass fp32 LayerNorm statistics, logits on v_mfma_f32_16x16x4_f32, softmax,
 * dl = w_y (p - onehot).  Every workgroup walks whole 64-row tiles -- the partition is a function of (rows, nc) only -- and writes
 * one slab row [dgamma 96 | dbeta 96 | dW nc x 96 | db nc | sum of w_y nll, sum of w_y, rows whose argmax (ties to the lowest class)
 * equals the label, 0]: msst_probe_scratch_floats(rows, nc) floats in all (0 for arguments the calls refuse).
 *
 * msst_probe_update.  Sums the slab rows in a fixed order and divides by the weight sum -- torch's CrossEntropyLoss(weight=),
 * reduction "mean" -- writes that mean gradient to grad_out [192 + 97 nc] when it is not null, and history_row [4] = {loss, weight
 * sum, hits, rows} of the parameters as they were.  apply != 0: torch.optim.Adam semantics on theta, m, v (coupled L2: g += weight_decay
 * theta; bias correction; eps outside the square root) with the step count kept on the device: step, int32 [MSST_PROBE_STEP_INTS], zero
 * before the first step; step[0] is the number of steps applied (every workgroup keeps a copy of its own, so none reads what another
 * writes).  A launch whose weight sum is 0 is skipped whole: theta, m, v and step stay, its loss (and grad_out) is NaN.  apply = 0
 * only reduces: theta, m, v, step may be null.  lr is an argument, so a schedule costs nothing.
 *
 * msst_probe_fwd.  logits and classes (int64 argmax, ties to the lowest class) of Q rows:
 *   x_layout = 0: rows [Q][96] (16-byte aligned);  x_layout = 1: the encode_scene map [Q / plane][96][plane] read in place;
 *   out_layout = 0: logits [Q][nc];                out_layout = 1: [Q / plane][nc][plane], the layout of predict_scene's logits.
 * A row with a NaN (or infinite) channel -- a pixel no window covers -- gets NaN logits and class -1.  plane is read in layout 1 only.
 *
 * Checked before any HIP call, in this order: MSST_ERR_BADARG for a size below 1 (M, dim, rows / Q, nc), row0 < 0 or row0 + rows > M;
 * MSST_ERR_UNSUPPORTED outside dim == 96, nc <= 128 and M, Q <= 2^31 - 1; MSST_ERR_BADARG for a negative (or NaN) lr, eps or
 * weight_decay, a beta outside [0, 1), a layout outside {0, 1}, in layout 1 a plane below 1 or not dividing Q, a null or misaligned
 * pointer, a slab smaller than msst_probe_scratch_floats.  msst_last_error names the call. */
#define MSST_PROBE_STEP_INTS 512
long msst_probe_scratch_floats(long rows, int nc);
int msst_probe_grad(const float* x, const int32_t* labels, const float* class_w, const float* theta, long M, int dim, long row0, long rows,
                    int nc, float* slab, long slab_floats, void* stream);
int msst_probe_update(const float* slab, long slab_floats, long rows, int dim, int nc, float* theta, float* m, float* v, int32_t* step,
                      double lr, double beta1, double beta2, double eps, double weight_decay, float* history_row, float* grad_out,
                      int apply, void* stream);
int msst_probe_fwd(const float* x, int x_layout, long Q, long plane, const float* theta, int dim, int nc, float* logits, int out_layout,
                   int64_t* classes, void* stream);

/* k-means clustering of frozen features (maskedsst_amd/cluster.py: fit_kmeans, ViTSpatialSpectral.cluster_scene).  Additive under
 * MSST_VERSION 109: no struct and no existing signature changes.  Lloyd's iteration is two launches, msst_kmeans_assign and
 * msst_kmeans_update; the k-means++ seeding is msst_kmeans_assign against the centres chosen so far and one msst_kmeans_pick per new
 * centre.  dim == 96, 1 <= k <= 128, fp32; nothing uses atomics and every output has the same bits in every call.
 *
 * Scores.  Every row gets s_c = x . c + bias_c per centroid: the dot product is the fp32 fmaf chain over the 96 channels in order
 * (v_mfma_f32_16x16x4_f32), the bias is added behind it.  MSST_KMEANS_COSINE: bias 0, unit centroids (and unit rows, if the
 * distance is to mean anything); MSST_KMEANS_EUCLIDEAN: bias_c = -0.5 |c|^2, so argmax_c s_c = argmin_c |x - c|^2.  ONE total order:
 * score descending, then cluster index ascending.  distance = max(0, 2 (1 - s)) (cosine) or max(0, |x|^2 - 2 s) (euclidean).  A row
 * whose |x|^2 is not finite (a NaN channel: a pixel no window covers) gets assignment -1 and distance NaN and contributes to no sum.
 *
 * msst_kmeans_assign.  x_layout = 0: rows [rows][96] (16-byte aligned); x_layout = 1: the encode_scene map [rows / plane][96][plane]
 * read in place.  Writes assign [rows] (int32), dist [rows] and, when not null, classes [rows] (int64: in layout 1 that is the map
 * [rows / plane][plane]).  Fit mode (slab not null): it also reads the previous contents of assign and writes one slab row per
 * workgroup, [sums k x 96 | counts k | sum of the distances | rows whose assignment changed]; a cluster's sum is one more product
 * onehot^T x on the same MFMA.  The workgroups own whole 64-row tiles and the partition depends on `rows` alone:
 * msst_kmeans_scratch_floats(rows, k) floats in all (0 for arguments the calls refuse).
 *
 * msst_kmeans_update.  Sums the slab rows in a fixed order and writes, per cluster, the new centroid (euclidean: sum / count, an IEEE
 * division; cosine: sum / |sum|; a cluster without rows, or a cosine sum of norm 0, keeps its centroid), its bias, counts [k] (int32)
 * and shift [k], the L2 displacement of the centroid; history_row [2] = {sum of the distances, rows whose assignment changed}.  The
 * number of empty clusters and the largest displacement follow from counts and shift.  After an iteration that moved no row the next
 * one reproduces every output bit for bit.
 *
 * msst_kmeans_pick.  Centre j of the k-means++ seeding, from the dist array and the slab that msst_kmeans_assign (fit mode, k = j)
 * left: total = the workgroups' distance sums in workgroup order; u = (h >> 8) 2^-24 with h the stateless counter hash of (seed, j);
 * t = u total; the chosen row is the first whose inclusive prefix sum of dist (workgroup blocks first, then rows ascending) exceeds t.
 * Rows chosen before do not count.  total == 0: the lowest row not chosen yet.  j == 0: row floor(u rows) (dist and slab are not
 * read).  The row is copied into centroid j (divided by its norm for cosine), bias[j] is set and seed_rows[j] = the row.
 *
 * Checked before any HIP call, in this order: MSST_ERR_BADARG for a size below 1 (rows, dim, k) or j outside [0, k);
 * MSST_ERR_UNSUPPORTED outside dim == 96, k <= 128, rows <= 2^31 - 1; MSST_ERR_BADARG for a metric or layout outside {0, 1}, in
 * layout 1 a plane below 1 or not dividing rows, a null or misaligned pointer, a slab smaller than msst_kmeans_scratch_floats.
 * msst_last_error names the call. */
#define MSST_KMEANS_COSINE 0
#define MSST_KMEANS_EUCLIDEAN 1
long msst_kmeans_scratch_floats(long rows, int k);
int msst_kmeans_assign(const float* x, int x_layout, long rows, long plane, int dim, const float* centroids, const float* bias, int k,
                       int metric, int32_t* assign, float* dist, int64_t* classes, float* slab, long slab_floats, void* stream);
int msst_kmeans_update(const float* slab, long slab_floats, long rows, int dim, int k, int metric, float* centroids, float* bias,
                       int32_t* counts, float* shift, float* history_row, void* stream);
int msst_kmeans_pick(const float* x, long rows, int dim, const float* dist, const float* slab, long slab_floats, int j, int k, int metric,
                     uint32_t seed, float* centroids, float* bias, int32_t* seed_rows, void* stream);

/* Second-order statistics of frozen features (maskedsst_amd/pca.py: fit_pca, FeaturePCA, ViTSpatialSpectral.pca_scene and
 * anomaly_scene).  Additive under MSST_VERSION 109: no struct and no existing signature changes.  dim == 96, fp32; nothing uses atomics
 * and every output has the same bits in every call.  x_layout = 0: rows [rows][96] (16-byte aligned); x_layout = 1: the encode_scene
 * map [rows / plane][96][plane] read in place.
 *
 * msst_feat_moments.  One pass over x.  c = x - centre (centre [96]; null: zeros) is formed in fp32; a row with a channel that is
 * not finite (a pixel no window covers) is skipped and not counted.  Every workgroup writes one slab row [n (int32 bits) | s1 96 |
 * s2 96 x 96]: the number of counted rows, s1[d] = sum c[d] and s2[i][j] = sum c[i] c[j], the latter on v_mfma_f32_16x16x4_f32 with the
 * row as the k index, so an entry is the fp32 fmaf chain of its rows in row order; s2 is symmetric bit for bit.  The workgroups own
 * whole 64-row tiles and the partition depends on `rows` alone: msst_feat_moments_scratch_floats(rows) floats in all (0 for
 * arguments the calls refuse).
 *
 * msst_feat_moments_finish.  Sums the slab rows in workgroup order in double and writes count [1] (int64), mean[d] = centre[d] +
 * s1[d] / n, and, when not null, cov [96][96] = (s2[i][j] - s1[i] s1[j] / n) / (n - ddof), evaluated in double and rounded once, and
 * raw [96 + 96 x 96] = [s1 | s2] rounded to fp32.  `centre` is the pointer the moments call was given.  n - ddof <= 0: cov is NaN;
 * n == 0: the mean is NaN.  The centred two-pass covariance is four launches: moments (null centre), finish (the mean), moments
 * (centre = that mean), finish (cov; the residual s1 of the second pass is the correction term, not assumed zero).
 *
 * msst_feat_project.  out[q][j] = sum_d (x[q][d] - mean[d]) components[j][d], components [r][96], 1 <= r <= 96: the subtraction in
 * fp32, the sum the fmaf chain over d = 0 .. 95 in order from a zero accumulator.  out (null: not wanted) is rows [rows][r]
 * (out_layout 0) or a map [rows / plane][r][plane] (out_layout 1); sumsq [rows] (null: not wanted) = sum_j out[q][j]^2 in an order
 * that depends on r alone.  A row with a channel that is not finite gets NaN in every output; a row's outputs have the same bits
 * whatever batch or layout it sits in.
 *
 * Checked before any HIP call, in this order: MSST_ERR_BADARG for rows or dim below 1 or a negative ddof; MSST_ERR_UNSUPPORTED
 * outside dim == 96, 1 <= r <= 96, rows <= 2^31 - 1; MSST_ERR_BADARG for a layout outside {0, 1}, in layout 1 a plane below 1 or not
 * dividing rows, a null or misaligned required pointer, both outputs null, a slab smaller than msst_feat_moments_scratch_floats.
 * msst_last_error names the call. */
long msst_feat_moments_scratch_floats(long rows);
int msst_feat_moments(const float* x, int x_layout, long rows, long plane, int dim, const float* centre, float* slab, long slab_floats,
                      void* stream);
int msst_feat_moments_finish(const float* slab, long slab_floats, long rows, int dim, const float* centre, int ddof, int64_t* count,
                             float* mean, float* cov, float* raw, void* stream);
int msst_feat_project(const float* x, int x_layout, long rows, long plane, int dim, const float* mean, const float* components, int r,
                      float* out, int out_layout, float* sumsq, void* stream);

/* Class-conditional Gaussian scores of frozen features (maskedsst_amd/gaussian.py: fit_gaussian, GaussianClassifier,
 * ViTSpatialSpectral.gaussian_predict_scene).  Additive under MSST_VERSION 109.  dim == 96, 1 <= nc <= 128, fp32, no atomics.  x and
 * x_layout as in msst_feat_project.  One table form serves full and tied covariances: n_tables <= nc tables, table t a centre
 * centres[t][96] and a matrix tables[t][96][96] (16-byte aligned); class c has a table id class_table[c] -- a HOST array [nc], read
 * and checked here, before the launch -- an offset offsets[c][96] in its table's whitened coordinates and a constant consts[c].
 *   z = A_t (x - centre_t): the subtraction in fp32, then the fmaf chain over d = 0 .. 95 from zero;
 *   d2_c = max((|z|^2 + |m_c|^2) - 2 z . m_c, 0) = |A_t (x - centre_t) - m_c|^2, every sum in an order that depends on 96 alone;
 *   score_c = fmaf(-0.5, d2_c, consts[c]).
 * classes [rows] (int32) is the argmax of the score under the total order (score descending, then class ascending), distance [rows]
 * the d2 of that class; a row with a channel that is not finite gets class -1 and NaN everywhere; a row whose distance exceeds max_d2
 * (+inf: none) gets class -2, its scores and distance still written.  scores (null: not wanted) is rows [rows][nc] (out_layout 0) or
 * a map [rows / plane][nc][plane] (out_layout 1).  A row's outputs have the same bits whatever batch or layout it sits in, with or
 * without scores.
 *
 * Checked before any HIP call, in this order: MSST_ERR_BADARG for negative rows, dim or nc below 1, n_tables outside [1, nc];
 * MSST_ERR_UNSUPPORTED outside dim == 96, nc <= 128, rows <= 2^31 - 1; MSST_ERR_BADARG for a layout outside {0, 1}, with a map on
 * either side a plane below 1 or not dividing rows, max_d2 negative or NaN; rows == 0 returns 0 here; then MSST_ERR_BADARG for a null
 * or misaligned pointer and for a table id outside [0, n_tables).  msst_last_error names the call. */
int msst_gauss_score(const float* x, int x_layout, long rows, long plane, int dim, const float* centres, const float* tables, int n_tables,
                     const int32_t* class_table, const float* offsets, const float* consts, int nc, float max_d2, int32_t* classes,
                     float* distance, float* scores, int out_layout, void* stream);

/* Gaussian mixtures of frozen features by EM (maskedsst_amd/mixture.py: fit_mixture, GaussianMixture,
 * ViTSpatialSpectral.mixture_scene).  Additive under MSST_VERSION 109: no struct and no existing signature changes.  dim == 96, fp32,
 * no float atomics; every sum runs in an order that depends on (rows, k) alone and the row partition on rows alone.
 *
 * The contract.  score_c(x) = log w_c - 0.5 (d2_c(x) + logdet_c) - 48 log(2 pi), d2_c = |A_c (x - mu_c)|^2, Sigma_c = L_c L_c^T,
 * A_c = L_c^-1 (lower triangular), logdet_c = 2 sum_i log L_c[i][i]: msst_gauss_score's full-covariance table form with zero offsets
 * (table c for component c, consts[c] = log w_c - 0.5 logdet_c - 48 log(2 pi)), which is the E-step's expensive part and is not
 * changed.  Posterior of a row: m = max_c score_c, lse = m + logf(sum_c expf(score_c - m)) with c ascending in fp32, r_c =
 * expf(score_c - lse); a score of -inf contributes exactly 0.  A row with a NaN score has lse NaN and NaN probs.  A row whose scores
 * are all -inf has lse = -inf and probs 0; in msst_gmm_moments it is skipped and not counted.
 *
 * msst_gmm_posterior.  scores as rows [rows][k] (in_layout 0) or as the map [rows / plane][k][plane] that msst_gauss_score writes with
 * out_layout 1 (in_layout 1); 1 <= k <= 128.  Writes lse [rows] and, when not null, probs in either layout (out_layout).  A row's
 * outputs have the same bits whatever batch or layout it sits in.
 *
 * msst_gmm_moments.  One pass over x (x_layout as in msst_feat_moments) and scores [rows][k], 1 <= k <= 32, centres [k][96].  Per row
 * lse and r as above; a row with a channel that is not finite, and a row whose lse is not finite, is skipped and not counted, by
 * selection.  The grid is (workgroups of feat_partition, k): per workgroup and component the slab row [n | s1 96 | s2 96 x 96] about
 * centres[c] -- n = sum r_c, s1 = sum r_c (x - centre_c), s2 = sum r_c (x - centre_c)(x - centre_c)^T as the product of the rows
 * scaled by sqrt(r_c) with themselves on v_mfma_f32_16x16x4_f32, the row as the k index: symmetric bit for bit, exact for r in {0, 1}
 * -- and behind them per workgroup [counted rows (int32 bits) | sum lse of the counted rows].  msst_gmm_scratch_floats(rows, k)
 * floats in all (0 for arguments the calls refuse).
 *
 * msst_gmm_update.  One workgroup per component sums that component's slab rows in workgroup order in double, N_c = sum n (every
 * workgroup sums all k for itself), and with delta = s1 / N_c writes
 *   weights[c] = N_c / sum_c N_c (0 when the sum is 0);  centres[c] += delta;
 *   covs[c] = s2 / N_c - delta delta^T + reg_covar I (cov_kind MSST_GMM_DIAG: the off-diagonal entries 0), symmetric bit for bit;
 *   tables[c] = A_c and logdet[c] from the Cholesky factorisation and triangular inverse in double, each rounded to fp32 once;
 *   consts[c] = log w_c - 0.5 logdet_c - 48 log(2 pi);
 *   raw (null: not wanted) [k][1 + 96 + 96 x 96] = the summed slab rows [N_c | s1 | s2] rounded to fp32.
 * A component with N_c < min_count (starved), and one whose factorisation meets a pivot that is not finite or not positive (failed),
 * keeps its centre, table, covariance and logdet; its weight and constant are still written (weight 0: constant -inf).  record [4] =
 * [mean lse per counted row, float (NaN without rows) | counted rows | starved components | failed factorisations, the three as int32
 * bits]; the last is ADDED to with an integer atomic, so the caller zeroes the record before the launch.
 *
 * Checked before any HIP call, in this order: MSST_ERR_BADARG for rows, dim or k below 1, a cov_kind outside {0, 1}, reg_covar or
 * min_count negative or NaN; MSST_ERR_UNSUPPORTED outside dim == 96, k <= 32 (msst_gmm_posterior: 128), rows <= 2^31 - 1;
 * MSST_ERR_BADARG for a layout outside {0, 1}, with a map on either side a plane below 1 or not dividing rows, a null or misaligned
 * required pointer, a slab smaller than msst_gmm_scratch_floats.  msst_last_error names the call. */
#define MSST_GMM_FULL 0
#define MSST_GMM_DIAG 1
long msst_gmm_scratch_floats(long rows, int k);
int msst_gmm_posterior(const float* scores, int in_layout, long rows, long plane, int k, float* lse, float* probs, int out_layout,
                       void* stream);
int msst_gmm_moments(const float* x, int x_layout, long rows, long plane, int dim, const float* scores, int k, const float* centres,
                     float* slab, long slab_floats, void* stream);
int msst_gmm_update(const float* slab, long slab_floats, long rows, int dim, int k, int cov_kind, double reg_covar, double min_count,
                    float* centres, float* tables, float* covs, float* logdet, float* consts, float* weights, float* raw, float* record,
                    void* stream);

/* Feature-guided CRF refinement of class maps (maskedsst_amd/crf.py: crf_affinity, crf_refine, ViTSpatialSpectral.refine_scene): a
 * local dense CRF (mean field, Potts compatibility) over the score maps the scene classifiers write.  Additive under MSST_VERSION 109:
 * no struct and no existing signature changes.  dim == 96, 1 <= radius <= 3, 1 <= nc <= 128, fp32, no float atomics.  The
 * K = (2 radius + 1)^2 - 1 neighbour offsets (dy, dx) are numbered j = 0 .. K-1 with dy ascending, then dx ascending, (0, 0) skipped.
 *
 * msst_crf_affinity: feat [Bs][96][Hs][Ws] (an encode_scene map, raw or normalised, read in place), cover [Bs][Hs][Ws] int32 or null
 * -> k [Bs][K][Hs][Ws] and live [Bs][Hs][Ws] (uint8).  A pixel is live when its 96 features are finite, ss = the fp32 fmaf chain of
 * their squares over d = 0 .. 95 from zero is positive and finite, and cover is null or > 0 there; rn = 1 / sqrtf(ss).
 *   k[p, j] = fmaf(a_tab[j], expf(-(d2 g)), s_tab[j]) when p and q = p + o_j are live and q lies inside p's scene, else exactly 0;
 *   d2 = max(0, 2 (1 - dot(f_p, f_q) (rn_p rn_q))), dot the fp32 fmaf chain over d = 0 .. 95 from zero (on the fp32 MFMA).
 * a_tab and s_tab are HOST arrays [K], taken as they are.  With tables symmetric under o -> -o, k[p, j] and k[p + o_j, j'] (j' the
 * opposite offset) have the same bits.
 *
 * msst_crf_step: one mean-field step.  scores, q_in (null: step 0), q_out: [Bs][nc][Hs][Ws]; k and live from msst_crf_affinity at the
 * same radius.  U[c] = unary_scale scores[c] (unary 0) or unary_scale logf(max(scores[c], 1e-30)) (unary 1);
 *   q_out = softmax_c(U[c] + sum_j k[p, j] q_in[c, p + o_j]), the sum one fmaf chain in j order from zero, the softmax with the maximum
 *   subtracted and its sum in class order; without q_in: softmax_c(U).  The message is not divided by sum_j k.
 * A neighbour whose q_in is NaN (a dead pixel) or that lies outside the scene is skipped by a test, not multiplied by zero.  A pixel
 * that is not live, has a NaN score or no score above -inf gets NaN probabilities and class -1.  classes (int32 [Bs][Hs][Ws], may be
 * null) is the argmax of q_out under the total order (value descending, then class ascending); with prev_classes (which may be the
 * classes buffer itself) and changed, *changed (int32, zeroed by the caller) is increased by the number of live pixels whose class
 * differs from prev_classes: integer atomics, bit-reproducible.
 *
 * Both check before any HIP call, in this order: MSST_ERR_BADARG for Bs, dim / nc, Hs or Ws below 1; MSST_ERR_UNSUPPORTED outside
 * dim == 96, nc <= 128, 1 <= radius <= 3, or for more than 2^31 - 1 tiles; MSST_ERR_BADARG for a g that is negative or not finite, a
 * unary outside {0, 1}, a unary_scale that is not positive and finite; MSST_ERR_BADARG for a null or misaligned required pointer,
 * q_in == q_out, or changed without prev_classes. */
int msst_crf_affinity(const float* feat, const int32_t* cover, int Bs, int dim, int Hs, int Ws, int radius, const float* a_tab,
                      const float* s_tab, float g, float* k, uint8_t* live, void* stream);
int msst_crf_step(const float* scores, int unary, float unary_scale, const float* q_in, const float* k, const uint8_t* live, int Bs, int nc,
                  int Hs, int Ws, int radius, float* q_out, int32_t* classes, const int32_t* prev_classes, int32_t* changed, void* stream);

/* SLIC superpixels of an encode_scene feature map and object-based class maps (maskedsst_amd/superpixel.py: fit_superpixels,
 * superpixel_pool, superpixel_classify, ViTSpatialSpectral.superpixel_scene): the grid form of SLIC (Achanta et al. 2012; gSLICr).
 * Additive under MSST_VERSION 109: no struct and no existing signature changes.  dim == 96, step S in {4, 8, 16}, C <= 128, Hs, Ws <=
 * 32768, fp32, no float atomics: the same bits in every call.
 *
 * Grid: gy = ceil(Hs / S) by gx = ceil(Ws / S) cells per scene; cell (i, j) owns rows [i S, min((i + 1) S, Hs)) and columns [j S,
 * min((j + 1) S, Ws)); superpixel id = i gx + j per scene, n_sp = gy gx.  A centre is centroids [Bs][n_sp][96], offsets [Bs][n_sp][2]
 * (y, x as fp32 offsets from the centre's own cell origin, in [-S, 2 S)), bias [Bs][n_sp], counts [Bs][n_sp] int32.  Labels and classes
 * are int64 [Bs][Hs][Ws], -1 for a dead pixel.
 * Live: the 96 features are finite and cover (int32 [Bs][Hs][Ws], may be null) is > 0.  A dead pixel gets label -1 and contributes to no
 * sum.  Nothing crosses the scene border; nothing passes between the scenes of a batch.
 *
 * msst_slic_assign: a live pixel in cell (i, j) competes among the centres of cells (i + di, j + dj), di, dj in {-1, 0, 1}, that lie
 * inside the grid and have count > 0:
 *   s_c(p) = fmaf(-hl, fmaf(dy, dy, dx dx), dot(f_p, c) + bias_c), dot the fp32 fmaf chain over d = 0 .. 95 from zero (on the fp32 MFMA),
 *   dy = (float)(y_p - i_c S) - offset_y (the integer is formed from the cell difference: small and exact), dx alike;
 * ONE total order: score descending, then superpixel id ascending; no candidate: label -1.  centroids == null is the home mode
 * (iteration 0): every live pixel takes its own cell, offsets, bias, counts and hl are not read.  With prev_labels (which may be the
 * labels buffer itself) and moved, *moved (int32, zeroed by the caller) is increased by the number of pixels whose label differs from
 * prev_labels: integer atomics, bit-reproducible.  best ([Bs][Hs][Ws], may be null) receives the winning score, NaN for label -1 and in
 * the home mode.  With slab (msst_slic_scratch_floats(Bs, Hs, Ws, S, MSST_SLIC_FIT_CHANNELS) floats)
 * every block of 8 x 8 pixels writes the sums of its pixels' features, places and the counts per centre of its window.
 * msst_slic_update: per centre the slab entries that can hold it, added in an order that depends on (Hs, Ws, S) alone; count > 0:
 * centroid = sum / count, offset = sum / count (one IEEE division each), bias = -0.5 x the fp32 fmaf chain of c[d]^2 from zero; count
 * == 0: counts becomes 0, centroid, offset and bias are kept, and the centre is never a candidate from then on.  *empty (int32, zeroed
 * by the caller, may be null) is increased by the number of empty centres.
 * msst_slic_pool / msst_slic_pool_finish: map [Bs][C][Hs][Ws] and labels -> table [Bs][n_sp][C] = the mean over the pixels of each
 * superpixel, a fixed-order sum (a selection, never a product with zero: -inf pools to -inf) and one division, NaN for a superpixel
 * without pixels; region_classes (int64 [Bs][n_sp], may be null) = the first largest entry above -inf, -1 where there is none.  Labels
 * are those of a fit: a label outside the 3 x 3 cells of its pixel contributes to no sum.
 * msst_slic_broadcast: classes[p] = region_classes[labels[p]], -1 for a label outside [0, n_sp).
 * msst_slic_scratch_floats: the floats of a slab for C summed channels; 0 for arguments the calls refuse.
 *
 * All check before any HIP call, in this order: MSST_ERR_BADARG for a size below 1; MSST_ERR_UNSUPPORTED outside dim == 96, step in
 * {4, 8, 16}, C <= 128, Hs, Ws <= 32768 (or more than 2^29 blocks); MSST_ERR_BADARG for an hl that is negative or not finite; then
 * MSST_ERR_BADARG for a null or misaligned required pointer, centroids without offsets, bias and counts, moved without prev_labels, or
 * a short slab.  msst_last_error names the call. */
#define MSST_SLIC_FIT_CHANNELS 98   /* 96 feature sums and 2 place sums per centre; the count is the slab's own column */
long msst_slic_scratch_floats(int Bs, int Hs, int Ws, int step, int C);
int msst_slic_assign(const float* feat, const int32_t* cover, int Bs, int dim, int Hs, int Ws, int step, float hl, const float* centroids,
                     const float* offsets, const float* bias, const int32_t* counts, int64_t* labels, const int64_t* prev_labels, int32_t* moved,
                     float* best, float* slab, long slab_floats, void* stream);
int msst_slic_update(const float* slab, long slab_floats, int Bs, int dim, int Hs, int Ws, int step, float* centroids, float* offsets,
                     float* bias, int32_t* counts, int32_t* empty, void* stream);
int msst_slic_pool(const float* map, const int64_t* labels, int Bs, int C, int Hs, int Ws, int step, float* slab, long slab_floats,
                   void* stream);
int msst_slic_pool_finish(const float* slab, long slab_floats, int Bs, int C, int Hs, int Ws, int step, float* table, int64_t* region_classes,
                          void* stream);
int msst_slic_broadcast(const int64_t* labels, const int64_t* region_classes, int Bs, int Hs, int Ws, int step, int64_t* classes, void* stream);

/* Connected regions of an integer map (maskedsst_amd/regions.py: label_regions, region_ids, sieve_classes, enforce_connectivity):
 * connected-component labelling of a class map or a superpixel label map, and one round of merging flagged regions into a neighbour:
 * the sieve (minimum mapping unit) and SLIC's connectivity pass.  Additive under MSST_VERSION 109: no struct and no existing signature
 * changes.  Integer arithmetic throughout, integer atomics only: every output has the same bits in every call, and the same bits for a
 * scene alone or inside a batch.  Limits: Hs, Ws <= 32768, Hs * Ws < 2^31, at most 2^31 - 1 tiles of 16 x 16 pixels in the batch.
 *
 * values is int64 [Bs][Hs][Ws]; a value < 0 is dead.  connectivity is 4 (the cross) or 8 (the 3 x 3 square).  A region is a maximal set
 * of live pixels of one scene with equal value, connected under `connectivity`; nothing crosses the scene border (the last pixel of a
 * row and the first of the next are no neighbours), nothing passes between the scenes of a batch.
 *
 * msst_regions_label: labels[b][y][x] (int64) = y0 Ws + x0 of the region's first pixel in raster order (its smallest linear index: the
 * ROOT), -1 for a dead pixel; sizes[b][y][x] (int32) = the region's pixel count at the root pixel, 0 everywhere else; count[b] (int32) =
 * the regions of scene b.  Three launches, whatever the map holds.
 * msst_regions_merge: one SIMULTANEOUS round -- every decision is taken from the round's input (values with the labels and sizes that
 * msst_regions_label gave for them under the same connectivity).
 *   mode 0 (sieve): a region is flagged when size < min_size; step is not read.
 *   mode 1 (fragments): values are superpixel ids of a step S grid, gy = ceil(Hs / S), gx = ceil(Ws / S), n_sp = gy gx; a value >= n_sp
 *     is treated as dead.  Per scene and id the kept region is the one of largest size, then lowest root; every other region of the id
 *     is flagged.  min_size is not read.
 *   The candidates of a flagged region R: the regions T that are live, unflagged and different from R, with a pixel that is a neighbour
 *   (under connectivity) of a pixel of R; in mode 1 only those whose id m is eligible: with [i0, i1] x [j0, j1] the box of the cells
 *   (y / S, x / S) of R's pixels and (im, jm) = (m / gx, m % gx): im - 1 <= i0, i1 <= im + 1, jm - 1 <= j0, j1 <= jm + 1 -- so a label
 *   stays in the 3 x 3 cells of its pixel, which msst_slic_pool relies on.  The winner is the candidate of largest size, then lowest
 *   root (one 64-bit integer atomicMax of (size << 32) | (0xFFFFFFFF - root) per boundary pixel).  values_out: every pixel of R takes the
 *   winner's value; a flagged region without a candidate, an unflagged region and a dead pixel keep their value (-1 stays -1, -2 stays
 *   -2).  values_out != values.  history (four int32, zeroed by the caller) is increased by the live regions, the flagged regions, the
 *   merged regions and the changed pixels, each summed over the batch.  Three launches in mode 0, four in mode 1.
 * scratch: msst_regions_scratch_bytes(Bs, Hs, Ws) bytes (0 for arguments the calls refuse), 16-byte aligned.  Its first int32 is the
 * ERROR WORD: zeroed by the caller before the first call, never zeroed and only ever raised by the calls; everything behind it is
 * overwritten by every call.  Every device loop (the finds and unions of the labelling) terminates because it follows strictly
 * decreasing indices, and still counts its turns against a cap derived from Hs * Ws; a loop that reaches the cap, or meets a parent
 * above its child, stops and raises the error word (1: find, 2: union, 3: both).  A non-zero error word means the outputs are not to be
 * used.  No loop waits for another workgroup.
 *
 * Both check before any HIP call, in this order: MSST_ERR_BADARG for a size below 1 (Bs, Hs, Ws; min_size in mode 0, step in mode 1);
 * MSST_ERR_UNSUPPORTED over the limits; MSST_ERR_BADARG for a connectivity outside {4, 8} or a mode outside {0, 1}; MSST_ERR_BADARG for
 * a null or misaligned pointer, values_out == values, or a short scratch.  msst_last_error names the call. */
long msst_regions_scratch_bytes(int Bs, int Hs, int Ws);
int msst_regions_label(const int64_t* values, int Bs, int Hs, int Ws, int connectivity, int64_t* labels, int32_t* sizes, int32_t* count,
                       void* scratch, long scratch_bytes, void* stream);
int msst_regions_merge(const int64_t* values, const int64_t* labels, const int32_t* sizes, int Bs, int Hs, int Ws, int connectivity, int mode,
                       int min_size, int step, int64_t* values_out, int32_t* history, void* scratch, long scratch_bytes, void* stream);

/* a7-a10: one fused pre-norm transformer block (PreNorm+Attention+FeedForward+residuals,
 * vit_spatial_spectral.py:22-104) over all B*S*N tokens; mode selects the spatial or spectral
 * sequence grouping of vit_spatial_spectral.py:410-431 (no transposes are materialised).
 * x -> y (y != x); x1 (optional) receives x + attn(LN(x)) for the backward.
 * dropout_p > 0 enables the reference's four dropout sites (:38,40,57,62) with a stateless counter-based
 * mask keyed by (seed, layer, site, element); msst_block_bwd regenerates it from the same three values.
 * xn_out (optional, [tokens][96] bf16): receives LN1(x) exactly as the block used it, so that msst_block_bwd neither
 * re-reads x nor renormalises it.
 * lse_out (optional, msst_block_lse_floats(...) fp32): the block's saved STATISTICS, two arrays back to back --
 *   [msst_block_tiles(...)][heads][64]: per (64-row tile, head, row), lse = log2 of the row's softmax denominator in the exponent
 *     domain of the kernels (p = exp2(s * dim_head^-0.5 * log2 e - lse), vit_spatial_spectral.py:71-73): the attention backward
 *     then computes the probabilities directly -- no row maximum, no row sum, no reciprocal; the tile order is the forward's own
 *     (same mode / shapes on both sides);
 *   [tokens] (MSST_VERSION 104): rstd of LN1 of every token (vit_spatial_spectral.py:22-29), token order: with it and the bf16 LN1
 *     rows (xn_out) the fused row-local backward rebuilds xhat = (LN1 row - beta) / gamma and does not read the fp32 block input
 *     at all (MSST_LN1_FROM_XN).
 *   10-12 MB per block at the bench shape.
 * *saved (host, optional) tells which of them the selected kernel wrote: MSST_SAVED_XN (the two tuned bf16 kernels -- role
 * split for 8 heads, 4-wave otherwise; not fp32, not MSST_KERNEL_GENERIC), MSST_SAVED_LSE and MSST_SAVED_RSTD (the role-split
 * kernel only).  Pass xn_saved / lse_saved to msst_block_bwd only when the bit is set. */
#define MSST_SAVED_XN 1
#define MSST_SAVED_LSE 2
#define MSST_SAVED_RSTD 4
long msst_block_lse_floats(int mode, int B, int S, int N, int heads);   /* floats of the whole statistics buffer: tiles * heads * 64 + tokens */
long msst_block_tiles(int mode, int B, int S, int N);                   /* 64-row tiles of a block launch (the forward's own tiling) */
int msst_block_fwd(const MsstBlockWeights* w /*host*/, const float* x, float* y, float* x1, int mode,
                   int B, int S, int N, int heads, int prec, int max_grid, float dropout_p, uint32_t seed,
                   int layer, void* xn_out, float* lse_out, int* saved /*host*/, void* stream);

/* The same forward for a RUN of blocks of ONE stack (same mode) as ONE launch (round 5): the blocks of a stack never mix the rows
 * of different 64-row tiles (vit_spatial_spectral.py:410-431: the regroupings sit between the stacks), so a workgroup takes a tile
 * through block after block -- block j reads what block j - 1 wrote, two blocks of one tile at least three pipeline steps apart --
 * and the prologue + pipeline fill / drain of all launches but one go away (26 us each).  Bit-identical to nblk calls of
 * msst_block_fwd with layer = layer0 .. layer0 + nblk - 1: block 0 reads x0, block j > 0 reads y[j - 1].
 * w, y, x1, xn_out, lse_out: HOST arrays of nblk pointers (x1 / xn_out / lse_out may be NULL as a whole: nothing saved).
 * Every per-block operand (each member of w[j], y[j], x1[j], xn_out[j], lse_out[j]) must lie a constant byte stride (|stride| < 2 GiB,
 * one stride per operand) from block to block -- the kernel addresses block j as block 0 + j x stride instead of fetching pointers.
 * The role-split bf16 forward only (8 heads; of the prec flags only MSST_X1_BF16), at most 16 blocks, and at most 1024 (tile, block)
 * steps per workgroup: MSST_ERR_UNSUPPORTED otherwise (nothing launched) -- call msst_block_fwd per block then. */
int msst_block_fwd_stack(const MsstBlockWeights* const* w /*host*/, int nblk, const float* x0, float* const* y /*host*/,
                         float* const* x1 /*host*/, void* const* xn_out /*host*/, float* const* lse_out /*host*/, int mode,
                         int B, int S, int N, int heads, int prec, int max_grid, float dropout_p, uint32_t seed, int layer0,
                         int* saved /*host, optional*/, void* stream);

/* a12-a14: gather of masked tokens, BlockwiseToPixels (vit_simmim_original.py:9-40,314-330),
 * target gather from the raw cube (:335) and mean-L1 / K (:338).
 * idx [B][K] int32; w_pix [S or 1][P][96], b_pix [S or 1][P]; per_block = to_pixels_per_spectral_block.
 * dpred [B][K][P] receives sign(pred-target); pred optional; partial: >= B*ceil(K/64) floats scratch.
 * loss: 1 float (device). */
int msst_head_fwd(const float* y, const float* img, const int32_t* idx, const float* w_pix,
                  const float* b_pix, int per_block, float* dpred, float* pred, float* partial,
                  float* loss, int B, int S, int N, int P, int K, void* stream);

/* SimMIM reconstruction: BlockwiseToPixels / to_pixels (vit_simmim_original.py:9-40, :328-332) over EVERY token instead of the
 * gathered ones, stored transposed into the cube layout, with the per-band error over the masked pixels from the same pass.
 * Added under MSST_VERSION 109 (additive: no struct, no existing signature changes).
 *   y [B][T][96] encoder output (T = S N, token c N + n; 16-byte aligned), img [B][S P][N] the input cube, mask [B][T] as
 *   msst_tokenize_fwd (1 = masked), w_pix / b_pix / per_block as msst_head_fwd.
 *   recon [B][S P][N]:  recon[b][c P + k][n] = b_c[k] + sum_d W_c[k][d] y[b][c N + n][d]  (c -> 0 in both tables when
 *     per_block == 0); fp32, one fmaf chain per element: the bias, then d = 0 .. 95.  blend != 0: a token whose mask byte is 0
 *     gets img's P values instead, bit for bit.  Every element is written.
 *   band_err [B][S P] DOUBLES: sum over the MASKED n of |pred - img| (the difference formed in double, the N terms of a band added
 *     in one fixed order by one wave); band_cnt [B][S P] int32: the number of masked n -- both whatever blend is.  Both null:
 *     no statistics (recon has the same bits); one null and one not: MSST_ERR_BADARG.
 * No atomics, nothing to zero: two calls give the same bits.  One launch.  N <= 64, S <= 64, P <= 16 (the constructor's limits).
 * Checked before anything is enqueued, in this order: MSST_ERR_BADARG for B, S, N or P < 1; MSST_ERR_UNSUPPORTED beyond the limits;
 * MSST_ERR_BADARG for a null required pointer, one statistics pointer without the other, or a y that is not 16-byte aligned. */
int msst_recon_fwd(const float* y, const float* img, const uint8_t* mask, const float* w_pix, const float* b_pix, int per_block,
                   int blend, float* recon, double* band_err /*optional*/, int32_t* band_cnt /*optional*/, int B, int S, int N,
                   int P, void* stream);

/* ---- backward (a15: what autograd does for the reference at pretrain.py:116) ---- */

/* d(loss)/d(encoder output) through the gather + to_pixels, and the to_pixels grads.
 * csr_ptr [B][T+1], csr_pos [B][K]: for each token the positions k with idx[b][k] == token
 * (duplicates allowed -- the reference's misaligned index slicing produces them).
 * gscale = 1 / (B*K*P) / K; gout = optional device scalar d(final)/d(loss) multiplied in.
 * dy [B][T][96] is fully written.
 * slab: S * nchunk * (P*96 + P) floats of scratch.  dw_pix / db_pix laid out like w_pix / b_pix. */
int msst_head_bwd(const float* y, const float* dpred, const int32_t* csr_ptr, const int32_t* csr_pos,
                  const float* w_pix, int per_block, float gscale, const float* gout, float* dy, float* slab,
                  int nchunk, float* dw_pix, float* db_pix, int B, int S, int N, int P, int K, void* stream);

/* Gradient destinations of one transformer block (fp32, shapes of the reference parameters). */
typedef struct MsstBlockGrads {
    float* ln1_g; float* ln1_b; float* wqkv; float* wout; float* bo;
    float* ln2_g; float* ln2_b; float* w1; float* b1; float* w2; float* b2;
} MsstBlockGrads;

/* Scratch sizes (floats) for msst_block_bwd */
#define MSST_MLP_SLAB (64 * 96 + 96 * 64 + 64 + 96 + 96 + 96)
#define MSST_ATTN_SLAB (3 * 64 * 96 + 96 * 64)
#define MSST_LN1_SLAB 288

/* Backward of one fused block: given the saved block input x, the saved mid residual x1 and dy,
 * writes dx and every parameter gradient of the block.  Internally: MLP half (recompute from x1)
 * -> attention half, one workgroup per (tile chunk, head) -- or per (tile chunk, head PAIR): the default bf16 kernel for an
 * even head count -- weight grads in registers -> LN1 backward + residual; partial-gradient slabs are reduced in a fixed
 * order (deterministic).
 * Workspace (caller-owned, device): dx1 [tokens][96] f32; dxn_part heads*tokens*96 elems
 * (f32 or bf16 by prec; the head-pair kernel uses the first half); slab grid_rows*(2*MSST_MLP_SLAB + MSST_LN1_SLAB) + nchunk*heads*MSST_ATTN_SLAB
 * floats (the bf16 MLP half runs up to 2*grid_rows workgroups, one slab each). */
int msst_block_bwd(const MsstBlockWeights* w /*host*/, const MsstBlockGrads* g /*host*/, const float* x,
                   const float* x1, const float* dy, float* dx, float* dx1, void* dxn_part, float* slab,
                   int grid_rows, int nchunk, int mode, int B, int S, int N, int heads, int prec,
                   float dropout_p, uint32_t seed, int layer, const void* xn_saved /*optional, see msst_block_fwd*/,
                   const float* lse_saved /*optional, see msst_block_fwd; used together with xn_saved by the two-head attention backward*/,
                   void* dab_ws /*optional workspace [tokens][96] bf16, used together with xn_saved: the MLP half leaves the
                                  dropped bf16 copy of dx1 there for the attention half*/,
                   void* stream);

/* The same backward for a RUN of blocks (bf16 throughput path): called once per block in reverse order, it fuses the row-local
 * seam BETWEEN consecutive blocks -- the LN1 backward of block i and the MLP-half backward of block i - 1
 * (vit_spatial_spectral.py:22-44,102-103 are row-local) run as ONE launch, so dx of block i never reaches HBM:
 *   first != 0 (the last block of the model = first call): its MLP half runs on dy first (dy -> dx1, dab_ws);
 *   every call: attention half of block i on the dx1 / dab_ws rows left by the step above or by the previous call;
 *   w_prev != NULL: LN1 backward of block i + MLP half of block i - 1 (weights w_prev, saved mid residual x1_prev; its
 *       parameter gradients go to g_prev): dx1 and dab_ws are overwritten IN PLACE with block i - 1's; dx is not touched;
 *   w_prev == NULL (block 0): the LN1 backward runs alone and writes dx.
 * Gradients of block i are complete when the call for block i returns (its MLP-half gradients were written by the call
 * before).  Requires prec = MSST_PREC_BF16 (tuned kernels), xn_saved and dab_ws, and at most four d(LN1 out) partials
 * (heads <= 8 even, or heads <= 4): MSST_ERR_BADARG / MSST_ERR_UNSUPPORTED otherwise -- use msst_block_bwd then.
 * slab: grid_rows*(3*MSST_MLP_SLAB + MSST_LN1_SLAB) + nchunk*heads*MSST_ATTN_SLAB floats.  x1 is read only when first != 0.
 * tile_queue != NULL (data parallel): the attention backward and the fused LN1 + MLP launch draw their tiles from agent-scope
 * counters in this scratch (zeroed on `stream` by the call) instead of the static partition tile = workgroup + k * grid: a
 * workgroup that starts late because a communication kernel holds its CU draws fewer tiles instead of running its whole
 * share behind the others.  The partition then depends on timing, so the gradients differ from run to run in fp32 summation
 * order; NULL keeps the static, bit-reproducible partition (the single-GPU default). */
#define MSST_TILE_QUEUE_WORDS 64
int msst_block_bwd_chain(const MsstBlockWeights* w /*host*/, const MsstBlockGrads* g /*host*/,
                         const MsstBlockWeights* w_prev /*host, block i - 1 or NULL*/, const MsstBlockGrads* g_prev /*host*/,
                         const float* x, const float* x1, const float* x1_prev, const float* dy, float* dx, float* dx1,
                         void* dxn_part, float* slab, int grid_rows, int nchunk, int mode, int B, int S, int N, int heads,
                         int prec, float dropout_p, uint32_t seed, int layer, const void* xn_saved, const float* lse_saved /*optional*/,
                         void* dab_ws, int first, int32_t* tile_queue /*optional, MSST_TILE_QUEUE_WORDS int32 of device scratch*/, void* stream);

/* Deferred slab reduction for a RUN of msst_block_bwd_chain calls made with MSST_BWD_DEFER_REDUCE in `prec`: one launch instead of
 * one per block (the reduction is the only part of a block backward whose cost does not shrink with the problem: 62 MB of
 * slabs per block at the bench grid, whatever the batch).  Call y = 0 .. count - 1 of the run used the workspace slab + y *
 * slab_stride floats (same grid_rows / nchunk / mode / shapes for all of them) and reduced-gradient destinations that lie
 * grad_stride floats apart: g + y * grad_stride for the attention half and LN1 of its block, g_prev + y * grad_stride for the
 * MLP half of the block before it that its fused launch ran (the first count_prev calls of the run had one; count_prev = count
 * except for the run that ends with block 0).  first != 0: call 0 of the run was made with first != 0 (standalone MLP half of
 * its own block, reduced into g).  slab_stride and grad_stride must be multiples of 4 floats.  Deterministic: same
 * summation order as the per-call reduction. */
int msst_block_bwd_reduce(const MsstBlockGrads* g /*host*/, const MsstBlockGrads* g_prev /*host, may be NULL when count_prev == 0*/,
                          float* slab, long slab_stride, long grad_stride, int count, int count_prev, int first,
                          int grid_rows, int nchunk, int mode, int B, int S, int N, int heads, int prec, void* stream);

/* Tokenizer backward: grads of blockwise_embed, pre/post norm, position table(s), mask token.
 * slab: S * nchunk * (N*96 + 96*P + 4*96 + 32) floats + S*N*96 floats (position staging).
 * dpos_a / dpos_b follow pos_a / pos_b of msst_tokenize_fwd; dmask_token may be null. */
int msst_tokenize_bwd(const float* img, const float* pre_g, const float* pre_b, const float* w_emb,
                      const float* b_emb, const float* post_g, const float* post_b, const uint8_t* mask,
                      const float* dx0, float* slab, int nchunk, float* dpre_g, float* dpre_b,
                      float* dw_emb, float* db_emb, float* dpost_g, float* dpost_b, float* dpos_a,
                      float* dpos_b, int pos_split, float* dmask_token, int B, int S, int N, int P,
                      float emb_dropout_p, uint32_t seed, void* stream);

/* Input gradient (additive under MSST_VERSION 109): d(loss)/d(img) through the tokenizer, what torch autograd gives the reference when
 * img.requires_grad.  Separate launches that only read what the parameter backward reads; they run when somebody asks for img.grad.
 *
 * msst_tokenize_bwd_input: per (sample, spectral block) the recompute of msst_tokenize_fwd (pre-norm LN over the P pixels, W_c xn + b_c,
 * post-norm LN over 96), the embedding dropout undone on dx0 [B][T][96] with the (p, seed) element addressing of msst_tokenize_bwd (the
 * two regenerate identical masks), zero for the tokens mask [B][T] marks (optional; a masked token's output does not depend on its
 * pixels), post-norm LN backward, dxn = W_c^T de, pre-norm LN backward.  dimg [B][S*P][N] is written whole (not accumulated), with
 * dtarget [B][S*P][N] (optional) added before the one store.  fp32, no atomics: bitwise reproducible.  The position tables and the
 * mask token play no part.  MSST_ERR_BADARG for B, S, N or P < 1 or a null required pointer, MSST_ERR_UNSUPPORTED outside N <= 64,
 * S <= 64, P <= 16; checked before anything is enqueued.
 *
 * msst_head_bwd_target: the SimMIM L1 loss's direct dependence on the input (its target is the raw pixels of the masked patches):
 * dtarget[b][c P + p][n] = -g sum_{k : idx[b][k] = c N + n} dpred[b][k][p], g = 1 / (B K P) / K (the normalisation of msst_head_fwd)
 * times gout[0] when gout is given; 0 for tokens no index names.  A gather through the inverse CSR of msst_head_bwd, the sum in CSR
 * order (a row may name a token more than once): bitwise reproducible.  dtarget [B][S*P][N] is written whole.  Argument checks as above
 * (and K < 1).
 *
 * msst_tokenize_scene_bwd_input: msst_tokenize_bwd_input (no mask, no dtarget) of windows win0 .. win0 + nwin - 1 of scene
 * [Bs][S*P][Hs][Ws], numbered as for msst_tokenize_scene_fwd_train, whose backward it is: dx0 [nwin][S*window*window][96], the values go
 * to the windows' pixels of dscene [Bs][S*P][Hs][Ws], bit for bit what msst_tokenize_bwd_input gives for the copied windows.  Only
 * stride == window (every pixel in at most one window: plain stores); other strides: MSST_ERR_UNSUPPORTED.  The calls of one batch
 * (win0 = 0 first, together all Bs nr nq windows) leave all of dscene defined: the call with win0 == 0 also zeroes the trailing
 * Hs % window rows and Ws % window columns, which belong to no window.  Argument checks of msst_tokenize_scene_fwd_train. */
int msst_tokenize_bwd_input(const float* img, const float* pre_g, const float* pre_b, const float* w_emb, const float* b_emb,
                            const float* post_g, const float* post_b, const uint8_t* mask /*optional*/, const float* dx0,
                            const float* dtarget /*optional*/, float* dimg, int B, int S, int N, int P, float emb_dropout_p,
                            uint32_t seed, void* stream);
int msst_head_bwd_target(const float* dpred, const int32_t* csr_ptr, const int32_t* csr_pos, const float* gout /*optional*/,
                         float* dtarget, int B, int S, int N, int P, int K, void* stream);
int msst_tokenize_scene_bwd_input(const float* scene, const float* pre_g, const float* pre_b, const float* w_emb, const float* b_emb,
                                  const float* post_g, const float* post_b, const float* dx0, float* dscene, int Bs, int Hs, int Ws,
                                  int window, int stride, long win0, int nwin, int S, int P, float emb_dropout_p, uint32_t seed,
                                  void* stream);

/* Scene gradients through windows at listed origins (additive under MSST_VERSION 109): listed windows overlap, so d(loss)/d(scene) is a
 * per-window input gradient and a fold that sums, per pixel, the windows covering it -- in a fixed order, without atomics.
 *
 * msst_tokenize_at_bwd_input: msst_tokenize_bwd_input (no mask, no dtarget) of the windows listed in origins [nwin][3] int32 = (scene,
 * y0, x0), the table of msst_tokenize_at_bwd; the pixels are read from the scene at the listed origin, the result is stored stacked:
 * dwin [nwin][S*P][window*window], plain stores, written whole.  For every (emb_dropout_p, seed) dwin is bit-identical to
 * msst_tokenize_bwd_input on the copied windows.  Checked before anything is enqueued: MSST_ERR_BADARG for a size below 1, nwin < 0 or
 * a null pointer (nwin = 0 is an empty call that launches nothing), MSST_ERR_UNSUPPORTED outside window <= Hs, Ws, window * window <=
 * 64, P <= 16.  THE CALLER GUARANTEES the table's value ranges, as for msst_tokenize_at_fwd.
 *
 * msst_scene_fold_at: dscene [Bs][C][Hs][Ws] gets, per pixel, the sum of dwin [nwin][C][window*window] over every listed window that
 * covers it.  The windows are found through an inverse index over origin cells -- a window's cell is (scene * Hs + y0) * Ws + x0:
 * cell_ptr int32 [Bs*Hs*Ws + 1], the CSR row pointers; cell_win int32 [nwin], window numbers sorted by cell, ascending window number
 * within a cell (maskedsst_amd.scene.origins_csr builds both).  THE SUMMATION ORDER IS PART OF THE CONTRACT: pixel (s, y, x) visits
 * y0 = max(0, y - window + 1) .. min(y, Hs - window) ascending (outer), x0 likewise (inner), and a cell's list in order; its addends
 * are added one at a time in that order, ascending (y0, x0, window number).  accumulate == 0: the sum starts from 0.f and uncovered
 * pixels are written 0.f -- dscene is defined whole.  accumulate != 0: the sum starts from the value in dscene, and a pixel no window of
 * this call covers is not touched; so a table that lists a regular grid in grid order may be split into consecutive calls and every
 * bit stays.  One thread per (pixel, group of `group` <= 16 consecutive channels; group = P for the tokenizer's planes); no atomics: bitwise
 * reproducible.  MSST_ERR_BADARG for a null pointer (dwin and cell_win may be null when nwin = 0), a size below 1 or nwin < 0;
 * MSST_ERR_UNSUPPORTED for group > 16, window * window > 64, window > Hs or Ws, or a grid beyond the launch limits (Bs*Hs*Ws above
 * 2^31 * 256 pixels, more than 65535 channel groups).  The caller guarantees a consistent index (entries outside [0, nwin) are skipped). */
int msst_tokenize_at_bwd_input(const float* scene, const int32_t* origins, const float* pre_g, const float* pre_b, const float* w_emb,
                               const float* b_emb, const float* post_g, const float* post_b, const float* dx0, float* dwin, int Bs,
                               int Hs, int Ws, int window, int nwin, int S, int P, float emb_dropout_p, uint32_t seed, void* stream);
int msst_scene_fold_at(const float* dwin, const int32_t* cell_ptr, const int32_t* cell_win, float* dscene, int Bs, int C, int Hs, int Ws,
                       int window, int nwin, int group, int accumulate, void* stream);

/* a17: classification head of ViTSpatialSpectral.forward (vit_spatial_spectral.py:536-564, :481-493):
 * mean over the spectral axis -> LayerNorm(96) -> Linear(96 -> n_classes); logits [B][n_classes][N].
 * Limits: N <= 64, S <= 64, any n_classes >= 1 (MSST_VERSION 108: the backward used to refuse n_classes > 32).  Both calls check
 * their arguments before any launch: MSST_ERR_BADARG for B, S, N or n_classes < 1 or a null pointer, MSST_ERR_UNSUPPORTED beyond
 * the limits.
 * _bwd: dy [B][T][96] fully written; dln_g / dln_b [96], dw [n_classes][96], db [n_classes] fully written (not accumulated),
 * bitwise reproducible; slab B*(n_classes*97 + 192) floats.
 * dy may be NULL (MSST_VERSION 109; a frozen body: nobody consumes dy): a variant of the kernel compiled without the LayerNorm
 * backward and without the dy stores runs; the four head gradients are bit-identical to those of the call with a dy buffer (same
 * partition, same summation order). */
int msst_cls_head_fwd(const float* y, const float* ln_g, const float* ln_b, const float* w, const float* b,
                      float* logits, int B, int S, int N, int n_classes, void* stream);
int msst_cls_head_bwd(const float* y, const float* dlogits, const float* ln_g, const float* ln_b, const float* w,
                      float* dy, float* slab, float* dln_g, float* dln_b, float* dw, float* db, int B, int S,
                      int N, int n_classes, void* stream);

/* Spectral MLP head of ViTSpatialSpectral(spectral_mlp_head=True) (vit_spatial_spectral.py:440-453, :536-564; MSST_VERSION 106):
 * 'b (c h w) d -> b h w (c d)' (the S tokens of a position concatenated, feature j = c * 96 + d, NO mean over c) -> LayerNorm(96 S)
 * -> Linear(96 S -> n_classes).  A row is one position (b, n): R = B * N rows of F = 96 * S features; y [B][S*N][96].
 * ln_g / ln_b [F], w [n_classes][F], b [n_classes].  logits [B][n_classes][N] (the layout of msst_cls_head_fwd).  fp32 arithmetic,
 * two-pass LayerNorm statistics, eps 1e-5.  Limits: N <= 64, S <= 64 (F <= 6144), n_classes <= 32 (MSST_ERR_UNSUPPORTED otherwise).
 * _bwd: dy [B][S*N][96] fully written (each token receives its own slice of d(row), no 1/S factor); dln_g / dln_b [F],
 * dw [n_classes][F], db [n_classes] are fully written (not accumulated), summed without atomics over a static row partition that
 * depends on B * N only: bitwise reproducible, independent of the device.  slab: msst_spec_head_bwd_slab(B, S, N, n_classes)
 * floats of scratch (16-byte aligned).  _bwd with a null pointer other than dy: MSST_ERR_BADARG, checked before anything is enqueued.
 * dy may be NULL (MSST_VERSION 109): the row pass is then a variant compiled without dxn = W^T dl, the LayerNorm backward and the dy
 * stores (it only leaves the row statistics for the weight-gradient pass); the four head gradients are bit-identical to those of
 * the call with a dy buffer. */
int msst_spec_head_fwd(const float* y, const float* ln_g, const float* ln_b, const float* w, const float* b,
                       float* logits, int B, int S, int N, int n_classes, void* stream);
long msst_spec_head_bwd_slab(int B, int S, int N, int n_classes);
int msst_spec_head_bwd(const float* y, const float* dlogits, const float* ln_g, const float* ln_b, const float* w,
                       float* dy, float* slab, float* dln_g, float* dln_b, float* dw, float* db, int B, int S,
                       int N, int n_classes, void* stream);

/* Pixelwise centre-pixel head of ViTSpatialSpectral(pixelwise=True) (vit_spatial_spectral.py:466-478, :536-564; MSST_VERSION 107):
 * 'b (c h w) d -> b c h w d', mean over c, LayerNorm(96) per position, Flatten (feature n * 96 + d, n = h * W + w) -> Linear(96 N ->
 * n_classes): one class vector per sample (window), for its centre pixel.  y [B][S*N][96]; ln_g / ln_b [96], w [n_classes][96 N],
 * b [n_classes]; logits [B][n_classes].  fp32 arithmetic, two-pass LayerNorm statistics, eps 1e-5.  ws: msst_pix_head_fwd_ws(B, N)
 * floats of scratch (the normalised features; 16-byte aligned).  Limits: S <= 64, N <= 64, n_classes <= 32 (MSST_ERR_UNSUPPORTED);
 * sizes below 1 or a null pointer: MSST_ERR_BADARG.  Both are checked before anything is enqueued.
 * _bwd (given dlogits [B][n_classes]): dy [B][S*N][96] fully written (every token of a position receives d(mean) / S); dln_g,
 * dln_b [96], dw [n_classes][96 N], db [n_classes] fully written (not accumulated), summed without atomics over a static partition
 * of the samples into groups of 32 (depends on B only): bitwise reproducible, independent of the device.  slab:
 * msst_pix_head_bwd_slab(B, S, N, n_classes) floats of scratch (16-byte aligned); 0 for a refused shape.
 * dy may be NULL (MSST_VERSION 109): a variant of the kernel compiled without the LayerNorm backward and the dy stores runs; the
 * four head gradients are bit-identical to those of the call with a dy buffer. */
long msst_pix_head_fwd_ws(int B, int N);
int msst_pix_head_fwd(const float* y, const float* ln_g, const float* ln_b, const float* w, const float* b, float* logits,
                      float* ws, int B, int S, int N, int n_classes, void* stream);
long msst_pix_head_bwd_slab(int B, int S, int N, int n_classes);
int msst_pix_head_bwd(const float* y, const float* dlogits, const float* ln_g, const float* ln_b, const float* w, float* dy,
                      float* slab, float* dln_g, float* dln_b, float* dw, float* db, int B, int S, int N, int n_classes,
                      void* stream);

/* msst_scene_centre_assemble (MSST_VERSION 107): the scene maps of a pixelwise model.  win_logits [nwin][n_classes]
 * (msst_pix_head_fwd of windows win0 .. win0 + nwin - 1, numbered as for msst_tokenize_scene_fwd) go to the centre pixel
 * (r * stride + window / 2, q * stride + window / 2) of their window in logits [Bs][n_classes][Hs][Ws], with the argmax in
 * classes [Bs][Hs][Ws] (int64; ties: lowest index, as torch.argmax).  A pixel is the centre of at most one window: no sums, no
 * atomics, any split into calls gives the same bits.  finalize != 0: pixels that are no window's centre get logit 0 and class -1
 * (msst_scene_assemble's "uncovered" convention).  The calls of one scene batch cover every window once, in any order. */
int msst_scene_centre_assemble(const float* win_logits, long win0, int nwin, float* logits, int64_t* classes, int Bs,
                               int n_classes, int Hs, int Ws, int window, int stride, int finalize, void* stream);

/* a7: LayerNorm over the last axis as an op of its own (nn.LayerNorm of PreNorm, vit_spatial_spectral.py:25, and of the
 * tokenizer, :194-195: eps 1e-5, affine, biased variance), fp32, rows of D <= 128 contiguous floats (D = 96 vectorised; D = 10 =
 * the tokenizer's pixel rows).  On the hot path the same arithmetic runs fused into msst_tokenize_* / msst_block_*; these
 * entry points serve a caller that needs a lone LayerNorm.  Row statistics are wave-shuffle (DPP) reductions.
 * _fwd: mean / rstd [rows] are optional outputs.  _bwd: recomputes the statistics from x; dgamma / dbeta [D] are fully
 * written (fixed summation order: bit-reproducible); slab: msst_layernorm_bwd_slab(rows, D) floats of scratch. */
int msst_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean /*optional*/,
                       float* rstd /*optional*/, long rows, int D, float eps, void* stream);
long msst_layernorm_bwd_slab(long rows, int D);
int msst_layernorm_bwd(const float* x, const float* gamma, const float* dy, float* dx, float* dgamma, float* dbeta,
                       float* slab, long rows, int D, float eps, void* stream);

/* Softmax cross entropy with ignore_index, its gradient and the counts of the finetune loops in one pass (reference src/utils.py:645-658:
 * CrossEntropyLoss(ignore_index) forward / backward, pixel accuracy on valid labels, NaN check; finetune.py:144-146: macro accuracy;
 * src/utils.py:531-541 in validation).  Added under MSST_VERSION 109 (additive: no struct, no existing signature changes).
 * logits [R0][n_classes][M] fp32 contiguous ([B, nc, H, W]: R0 = B, M = H W; [B, nc]: M = 1); labels [R0][M] int64.  A row is one
 * (sample, pixel).  A row COUNTS when its label is not ignore_index, its label lies in [0, n_classes) and, if skip (optional, int64
 * [R0][M]) is given, skip[row] >= 0 (the class map of msst_scene_assemble: -1 = no window covers the pixel).  A row that is neither
 * ignored nor skipped and whose label lies outside [0, n_classes) does not count and is tallied in bad_labels.
 * msst_ce_stats_fwd writes
 *   loss [1]: the mean over the counting rows of log sum_c exp(x_c) - x_label (row maximum subtracted first); NaN when no row counts;
 *   d (optional) [R0][n_classes][M]: softmax - onehot for a counting row, zeros for every other row;
 *   record [MSST_CE_RECORD_SLOTS(n_classes)], 8-byte slots: MSST_CE_LOSS_SUM (a DOUBLE: the sum of the rows' fp32 losses, one fp32
 *     partial per 256 rows, the partials added in double, both in a fixed order), then int64: MSST_CE_N_VALID (counting rows),
 *     MSST_CE_N_CORRECT (counting rows whose argmax -- ties: lowest index, a NaN is the maximum, as torch.argmax -- is the label),
 *     MSST_CE_BAD_LABELS, MSST_CE_NONFINITE (counting rows whose loss is NaN or +-inf), from MSST_CE_SUPPORT on support[n_classes]
 *     (counting rows by label) and correct[n_classes] (the correct ones by label).
 * Every word of loss, d and record is written (nothing needs zeroing); no float atomics: two calls give the same bits.
 * scratch: msst_ce_scratch_bytes(R0, n_classes, M) bytes (4-byte aligned; 0 for a refused shape).  Two launches.
 * msst_ce_bwd: dlogits = (d / n_valid) * gout, n_valid = record[MSST_CE_N_VALID] and gout (optional device scalar, null: 1) read on
 * the device; n_valid == 0: zeros.  dlogits may be d itself.  One launch.
 * Both check their arguments before any launch: MSST_ERR_BADARG for R0, n_classes or M < 1 or a null required pointer,
 * MSST_ERR_UNSUPPORTED when R0 * M or R0 * n_classes * M is 2^31 or more.  Any n_classes >= 1. */
#define MSST_CE_LOSS_SUM 0
#define MSST_CE_N_VALID 1
#define MSST_CE_N_CORRECT 2
#define MSST_CE_BAD_LABELS 3
#define MSST_CE_NONFINITE 4
#define MSST_CE_SUPPORT 5
#define MSST_CE_RECORD_SLOTS(n_classes) (5 + 2 * (n_classes))
long msst_ce_scratch_bytes(int R0, int n_classes, int M);
int msst_ce_stats_fwd(const float* logits, const int64_t* labels, const int64_t* skip /*optional*/, long ignore_index,
                      float* d /*optional*/, float* loss, int64_t* record, void* scratch, int R0, int n_classes, int M,
                      void* stream);
int msst_ce_bwd(const float* d, const int64_t* record, const float* gout /*optional*/, float* dlogits, int R0, int n_classes,
                int M, void* stream);

/* The same loss with class weights, label smoothing and a confusion matrix: torch.nn.CrossEntropyLoss(weight, ignore_index,
 * label_smoothing) with reduction "mean", as the DeepHyperX protocol trains (reference DeepHyperX/models.py:37-72), and the matrix its
 * metrics are computed from (DeepHyperX/utils.py:331-385).  Added under MSST_VERSION 109 (additive: no struct, no existing signature
 * changes; the three calls above and their results are untouched).  Layout, the rule for a row that COUNTS, bad_labels and the record
 * are those of msst_ce_stats_fwd.  With class_weight w [n_classes] fp32 (optional; null: all ones), W = sum_k w_k, label_smoothing
 * eps in [0, 1), y a counting row's label and p its softmax:
 *   row loss  l = -(1 - eps) w_y log p_y - (eps / n_classes) sum_k w_k log p_k
 *   loss [1]  sum of l / sum of w_y over the counting rows; NaN unless that weight sum is > 0 (no row counts, or only rows of weight 0)
 *   d (optional)  p_c ((1 - eps) w_y + (eps / n_classes) W) - (1 - eps) w_y [c == y] - (eps / n_classes) w_c; zeros for other rows
 *   record    as msst_ce_stats_fwd (MSST_CE_LOSS_SUM: the sum of l; the counts do not depend on w or eps: a row of weight 0 counts)
 *   sums [2]  DOUBLES: MSST_CE_EXT_LOSS_SUM (the same value as record slot 0) and MSST_CE_EXT_WEIGHT_SUM (sum of w_y; one fp32
 *             partial per 256 rows, the partials added in double, in the order of the loss sum; without weights it equals n_valid)
 *   confusion (optional) int64 [n_classes][n_classes]: confusion[y][argmax] over the counting rows, argmax as for MSST_CE_N_CORRECT,
 *             so its diagonal is correct[] and its row sums are support[] of the same call.  n_classes <=
 *             MSST_CE_CONFUSION_MAX_CLASSES when it is asked for (beyond: MSST_ERR_UNSUPPORTED); without it any n_classes >= 1.
 * Every word of loss, d, record, sums and confusion is written; no float atomics: two calls give the same bits.  With a null
 * class_weight and eps = 0 the loss, the record and d are bit for bit those of msst_ce_stats_fwd.
 * scratch: msst_ce_ext_scratch_bytes(R0, n_classes, M, confusion != 0) bytes (4-byte aligned; 0 for a refused shape): two fp32
 * partials and an int32 row [4 + 2 n_classes] per 256 rows, and with a confusion matrix an int32 [n_classes][n_classes] per 256 rows.
 * Two launches.
 * msst_ce_ext_bwd: dlogits = (d / sums[MSST_CE_EXT_WEIGHT_SUM]) * gout, read on the device; zeros unless the weight sum is > 0.
 * dlogits may be d itself.  One launch.
 * Checked before any launch, in this order: MSST_ERR_BADARG for R0, n_classes or M < 1; MSST_ERR_UNSUPPORTED when R0 * M or
 * R0 * n_classes * M is 2^31 or more; MSST_ERR_BADARG for a label_smoothing outside [0, 1) (a NaN included); MSST_ERR_UNSUPPORTED
 * for a confusion matrix with n_classes > MSST_CE_CONFUSION_MAX_CLASSES or one whose scratch has 2^31 words or more;
 * MSST_ERR_BADARG for a null required pointer. */
#define MSST_CE_EXT_LOSS_SUM 0
#define MSST_CE_EXT_WEIGHT_SUM 1
#define MSST_CE_CONFUSION_MAX_CLASSES 128
long msst_ce_ext_scratch_bytes(int R0, int n_classes, int M, int confusion);
int msst_ce_ext_fwd(const float* logits, const int64_t* labels, const int64_t* skip /*optional*/, long ignore_index,
                    const float* class_weight /*optional*/, float label_smoothing, float* d /*optional*/, float* loss,
                    int64_t* record, double* sums, int64_t* confusion /*optional*/, void* scratch, int R0, int n_classes, int M,
                    void* stream);
int msst_ce_ext_bwd(const float* d, const double* sums, const float* gout /*optional*/, float* dlogits, int R0, int n_classes,
                    int M, void* stream);

/* Fused AdamW over a flat fp32 buffer (torch.optim.AdamW semantics, src/utils.py:36-45), with the
 * reference's value clamp of the gradient (pretrain.py:71-73) when clamp > 0. */
int msst_adamw(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2,
               float eps, float weight_decay, int step, float clamp, float gscale, void* stream);

/* Grouped Adam / AdamW (MSST_VERSION 109): ONE launch updates any number of disjoint element ranges of the flat buffers, each with
 * its own learning rate, weight decay and bias-correction step -- the finetune recipe of the reference (finetune.py:110-136:
 * torch.optim.Adam with coupled L2 decay, lr / mlp_head_lr, frozen parameters skipped).  Per element of a range, flags == 0:
 *     g' = g * gscale + wd * p;  m += (1 - b1) (g' - m);  v = b2 v + (1 - b2) g'^2;
 *     p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
 * = torch.optim.Adam(weight_decay=wd), no amsgrad.  MSST_ADAM_DECOUPLED: g' = g * gscale and p *= 1 - lr * wd before the update
 * (torch.optim.AdamW).  1 - b1, 1 - b2, the bias corrections and 1 - lr * wd are formed on the host in double, as torch does,
 * and reach the kernel as floats; that is why the betas are doubles here: the float nearest to 0.999 has a 1 - b2 that is off by
 * 1.3e-5 of itself, which v would inherit in the first steps.
 * groups: HOST array of ngroups entries sorted by start, disjoint, end >= start, step >= 1; group_bytes = sizeof(MsstAdamGroup) (a
 * table of another header revision is refused).  The table travels by value in the kernel arguments: no allocation, no copy, no
 * synchronisation.  ngroups <= MSST_ADAM_MAX_GROUPS.  Every violation returns MSST_ERR_BADARG before anything is enqueued; an
 * empty table or only empty ranges: 0, nothing launched.  Elements outside every range are neither read nor written in any of
 * the four buffers.  Range ends are arbitrary: the 16-byte aligned interior of a range moves as dwordx4, its ragged ends
 * (at most 3 + 3 elements) as single floats; buffers that are not 16-byte aligned themselves are walked float by float. */
#define MSST_ADAM_DECOUPLED 1
#define MSST_ADAM_MAX_GROUPS 64
typedef struct {
    long start, end;       /* element range [start, end) of p / g / m / v */
    float lr, weight_decay;
    int step;              /* bias-correction step of this range, >= 1 */
    int flags;             /* MSST_ADAM_DECOUPLED: AdamW decay; 0: coupled L2 (Adam) */
} MsstAdamGroup;
int msst_adam_groups(float* p, const float* g, float* m, float* v, const MsstAdamGroup* groups /*host*/, int ngroups,
                     int group_bytes, double beta1, double beta2, float eps, float gscale, void* stream);

/* Gradient accumulation over micro-batches and the global-norm clip on the flat gradient buffers (additive under MSST_VERSION 109).
 * Both entry points work over a HOST table of 1 .. MSST_GRAD_MAX_RANGES element ranges [start, end) of the flat buffers, ascending,
 * disjoint, end > start; range_bytes = sizeof(MsstGradRange).  The table travels by value in the kernel arguments.  Elements outside
 * every range are neither read nor written in any buffer.  Range ends are arbitrary: the 16-byte aligned interior of a range moves
 * as dwordx4, its ragged ends (at most 3 + 3 elements) as single floats; buffers that are not 16-byte aligned themselves are walked
 * float by float.  One launch each, 256 threads per workgroup, a capped grid and a strided loop.  No atomics, nothing to zero
 * beforehand: two calls on the same input give the same bits in every output, the scratch included.
 *
 * The accumulate call, per element of a range:  a = first ? g[i] : acc[i] + g[i] (one fp32 add);  acc[i] = a;  with out != NULL also
 * out[i] = a * scale (one fp32 multiply; out may be g itself: a lane reads its elements before it writes them; out must not be acc).
 * With scratch != NULL every workgroup also leaves, in its own slot of scratch, the double sum of (double)a * (double)a over its
 * elements and the count of its non-finite a, summed in a fixed order; which element belongs to which workgroup depends on the range
 * table alone.  scratch: msst_grad_accum_scratch_bytes(nranges) bytes of device memory, 8-byte aligned (0 for nranges outside
 * 1 .. MSST_GRAD_MAX_RANGES).
 *
 * The finalize call reads a scratch the accumulate call wrote for the SAME table.  Every workgroup re-reduces the partials in one fixed
 * order, in double, and forms   total = (float)(scale * sqrt(sum));   coef = max_norm > 0 ? min(1, max_norm / (total + 1e-6f)) : 1
 * in fp32 -- the operations of torch.nn.utils.clip_grad_norm_ on the gradient acc * scale -- then   g[i] = (acc[i] * scale) * coef,
 * two fp32 multiplies in that order.  One workgroup writes record[0..3] = {total, coef, (float)(number of non-finite a), 0} on the
 * device.  g must not be acc.
 *
 * Checked before anything is enqueued, in this order: MSST_ERR_BADARG for a null required pointer (acc, g, ranges; finalize also
 * scratch and record), for nranges < 1 and for a range_bytes of another header revision; MSST_ERR_UNSUPPORTED for nranges >
 * MSST_GRAD_MAX_RANGES; MSST_ERR_BADARG for a range with start < 0 or end <= start, for ranges that overlap or do not ascend, and for
 * a scratch that is not 8-byte aligned and for a g or an out that is acc. */
#define MSST_GRAD_MAX_RANGES 64
typedef struct {
    long start, end;       /* element range [start, end) of the flat buffers */
} MsstGradRange;
long msst_grad_accum_scratch_bytes(int nranges);
int msst_grad_accumulate(float* acc, const float* g, const MsstGradRange* ranges /*host*/, int nranges, int range_bytes, int first,
                         float* out /*optional*/, float scale, void* scratch /*optional*/, void* stream);
int msst_grad_finalize(const float* acc, float* g, const MsstGradRange* ranges /*host*/, int nranges, int range_bytes, float scale,
                       float max_norm, const void* scratch, float* record, void* stream);

/* SimMIM masks drawn on the device (additive under MSST_VERSION 109): for the rows row0 .. row0 + rows - 1 of a conceptually unbounded
 * global batch, the four arrays a SimMIM step consumes, in ONE launch (one workgroup per row), all device memory:
 *   mask    uint8 [rows][T]     1 = masked: what msst_tokenize_fwd takes            (T = S * N)
 *   idx     int32 [rows][K]     the masked-token gather: what msst_head_fwd takes   (K = int(masking_ratio * T), computed by the caller)
 *   csr_ptr int32 [rows][T + 1] } the token-CSR of that gather, exactly what msst_head_bwd takes: the positions k with idx[k] == t are
 *   csr_pos int32 [rows][K]     } csr_pos[csr_ptr[t] .. csr_ptr[t + 1] - 1], ascending
 * Keys are 32 bits of a stateless counter hash of (seed, mode, global row, spectral block, element); a row has the same bits whether it
 * is drawn alone or inside any batch, whatever row0, rows and the launch geometry are.  Selection is always "the m elements with the
 * smallest (key, index) pairs".
 *   MSST_MASK_TOPK   T keys per row, the K smallest are masked.  idx = the masked tokens ascending, csr_pos[k] = k, csr_ptr[t] = the
 *                    number of masked tokens below t.  rand_size, scale and mask_count are ignored.
 *   MSST_MASK_BLOCK  per (row, spectral block) rand_size^2 cell keys; the mask_count smallest cells are masked, each covering scale x
 *                    scale positions of the side x side position grid (side = rand_size * scale, side * side = N).
 *   MSST_MASK_TUBE   as MSST_MASK_BLOCK with one draw per row repeated over the S blocks.
 * In the last two modes every row holds R = S * mask_count * scale^2 trues and idx is the row-major list of the true columns of the
 * global mask cut into chunks of K: entry k of row g is the true of rank (K g + k) % R in mask row (K g + k) / R (a row <= g; the
 * kernel regenerates it).  Duplicates inside an index row occur and are legal.
 * No atomics, nothing to zero beforehand, every output element is written and nothing beyond; two calls give the same bits.
 * Checked before anything is enqueued, in this order: MSST_ERR_BADARG for rows, S, N or K below 1, for a negative row0 or one above
 * 2^48, and for a mode outside the three; MSST_ERR_UNSUPPORTED for N > 64 or S > 64; MSST_ERR_BADARG for K > T; in the block and tube
 * modes MSST_ERR_BADARG for rand_size or scale below 1 or (rand_size * scale)^2 != N, for mask_count outside 1 .. rand_size^2 and for
 * R < K; MSST_ERR_BADARG for a null pointer. */
#define MSST_MASK_TOPK 0
#define MSST_MASK_BLOCK 1
#define MSST_MASK_TUBE 2
int msst_draw_masks(uint8_t* mask, int32_t* idx, int32_t* csr_ptr, int32_t* csr_pos, uint32_t seed, long row0, int rows, int S, int N,
                    int K, int mode, int rand_size, int scale, int mask_count, void* stream);

/* Opt-in per-kernel timing: when enabled every kernel launch of the library is bracketed by a pair
 * of HIP events recorded on the launch stream.  msst_profile_collect synchronises on the recorded
 * events and returns, per kernel id (0 .. msst_profile_kernels()-1), the summed duration in ms and
 * the launch count since enable / the previous collect.  Thread-safe (mutex); meant for bench.py.
 * msst_debug_stamps: kernel-study builds (-DMSST_STAMPS) only; returns MSST_ERR_UNSUPPORTED otherwise. */
int msst_debug_stamps(void* device_buf /* >= 256 u64; kernel-study aid, see tools/stamps.py */);
/* Occupancy probe (diagnostic, bench.py --cu-thief): nblocks workgroups that only hold a CU each -- 256 threads and ALL 160 KB
 * of the CU's LDS, so that no workgroup that uses LDS (every MFMA kernel of this library does) fits beside one -- for `microseconds`,
 * enqueued on `stream`; sink: 4 bytes of device scratch.  Stands in for the channel workgroups of an RCCL collective when
 * the overlap of the gradient all-reduce with the backward is studied on ONE GPU. */
int msst_debug_cu_thief(int nblocks, int microseconds, void* sink, void* stream);
/* Box probe (diagnostic, bench.py `box_probe`; MSST_VERSION 104): what THIS GPU sustains right now -- out[0] = TFLOP/s of back-to-back
 * v_mfma_f32_32x32x16_bf16 on hashed full-range operands (two waves per SIMD on every CU; the chip clocks to its power budget, so this
 * differs from box to box and from the 2.5 PFLOP/s nominal), out[1] = the shader clock in MHz that stream held, out[2] = GB/s of a
 * read-only stream over the scratch buffer, out[3] = seconds spent.  scratch: device memory, >= 1 MiB (>= 1 GiB for an HBM number:
 * the memory-side cache holds 256 MB).  The one entry point that SYNCHRONISES the stream (it times with HIP events); <= 0.3 s. */
int msst_debug_box_probe(double* out4, void* scratch, long scratch_bytes, void* stream);
int msst_profile_enable(int on);
/* restrict the event pairs to the kernel ids whose bit is set (default: all); each pair costs ~10 us of stream time */
int msst_profile_select(unsigned long long mask);
/* bracket only every n-th launch of each selected kernel (default 1 = all): keeps the event pairs inside a timed region cheap */
int msst_profile_sample(int every);
int msst_profile_kernels(void);
const char* msst_profile_name(int id);
int msst_profile_collect(double* total_ms /*host*/, long* count /*host*/);

#ifdef __cplusplus
}
#endif
#endif
