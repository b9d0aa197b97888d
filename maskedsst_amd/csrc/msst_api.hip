// extern "C" boundary of libmsst (see include/msst.h).  Thin argument marshalling only.
#include "../../include/msst.h"
#include "msst_kernels.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <atomic>
#include <mutex>
#include <vector>

namespace msst {

static thread_local char g_err[256] = "";

static int fail(int code, const char* what) {
    if (code > 0) snprintf(g_err, sizeof(g_err), "%s: hip error %d (%s)", what, code, hipGetErrorString((hipError_t)code));
    else if (code < 0) snprintf(g_err, sizeof(g_err), "%s: msst error %d", what, code);
    return code;
}

// ------------------------------------------------------------------------------------------
// weight prep: fp32 master -> operand element type, optional transpose.  One launch for all jobs.
// ------------------------------------------------------------------------------------------
template <class E>
__global__ __launch_bounds__(256) void prep_weights_kernel(const MsstPrepJob* jobs, int* err_flag) {
    const MsstPrepJob j = jobs[blockIdx.y];
    // malformed jobs are skipped (the job table lives in device memory: the host entry point cannot validate it) and reported
    // through the caller's error word: 1 = bad pack / shape, 2 = a 2-byte destination that is not whole fragments (16 x 32 for
    // pack 0, 32 x 16 for pack 1)
    const bool half = sizeof(E) == 2 && (j.pack & MSST_PREP_HALF);   // destination elements IEEE half instead of bf16 (the fp16-operand forward)
    if (j.pack < 0 || (j.pack & ~MSST_PREP_HALF) > 1 || (sizeof(E) != 2 && (j.pack & MSST_PREP_HALF)) || j.rows < 1 || j.cols < 1) {
        if (err_flag && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(err_flag, 1);
        return;
    }
    const int pack = j.pack & 1;
    const int R = j.transpose ? j.cols : j.rows, K = j.transpose ? j.rows : j.cols;   // logical [R][K] destination
    const int RB = pack ? 32 : 16, KB = pack ? 16 : 32;                               // fragment = RB rows x KB k, lane = (k / 8) * RB + row
    if (sizeof(E) == 2 && ((R % RB) || (K % KB))) {
        if (err_flag && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(err_flag, 2);
        return;
    }
    const int n = j.rows * j.cols;
    E* dst = reinterpret_cast<E*>(j.dst);
    if constexpr (sizeof(E) == 2) {
        // bf16: a thread writes the 8 consecutive k of one lane of one fragment -- 16 bytes of the fragment-packed destination
        // (see PBF16::ld_w; round 4: one 16-byte store instead of eight 2-byte ones, 55 -> see DESIGN us for the launch)
        for (int i8 = blockIdx.x * 256 + threadIdx.x; i8 < n / 8; i8 += gridDim.x * 256) {
            const int f = i8 / 64, lane = i8 - f * 64;
            const int fr = f / (K / KB), fk = f - fr * (K / KB);
            const int r = fr * RB + (lane % RB), c0 = fk * KB + (lane / RB) * 8;
            s16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int c = c0 + e;
                const int src_i = j.transpose ? c * j.cols + r : r * j.cols + c;   // dst[r][c] = src[c][r] when transposed
                float v = j.src[src_i];
                // to_qkv^T for the round-3 attention backward: the q and k blocks (the first scale_rows source rows) carry the softmax
                // scale dim_head^-0.5 = 2^-3, exact in bf16 -- that kernel keeps dq / dk unscaled (reference vit_spatial_spectral.py:54,71)
                if (src_i / j.cols < j.scale_rows) v *= j.scale;
                o[e] = (short)(half ? f2h(v) : f2bf(v));
            }
            *reinterpret_cast<s16x8*>(dst + (long)i8 * 8) = o;
        }
    } else {
        for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
            // i indexes the destination (coalesced writes)
            int src_i = i;
            if (j.transpose) {
                const int c = i / j.rows, r = i - c * j.rows;  // dst[c][r] = src[r][c]
                src_i = r * j.cols + c;
            }
            float v = j.src[src_i];
            if (src_i / j.cols < j.scale_rows) v *= j.scale;
            dst[i] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------
// opt-in profiler: a pair of HIP events around each kernel launch, on the launch stream
// ------------------------------------------------------------------------------------------
// The compute entry points keep no state: with the profiler off (the default) a call reads ONE relaxed atomic flag
// and nothing else that is shared.  The opt-in profiler state below is guarded by a mutex (records) and is
// per-thread where a launch is bracketed (the open record), so enabling it never makes a compute call unsafe.
struct ProfRec { int id; hipEvent_t a, b; };
#if defined(MSST_STAMPS) || defined(MSST_LAB)
static unsigned long long* g_stamps = nullptr;   // kernel-study builds only (python -m maskedsst_amd.build --stamps; -DMSST_LAB: the scratch of tools/gate_qkv.py)
#endif
static std::atomic<bool> g_prof_on{false};
static std::atomic<unsigned long long> g_prof_mask{~0ull};   // kernels (bit = id) that get event pairs
static std::atomic<int> g_prof_every{1};                      // ... every n-th launch of each (msst_profile_sample)
static std::atomic<unsigned> g_prof_seen[K_COUNT];
static std::mutex g_prof_mu;
static std::vector<ProfRec> g_prof;
static std::vector<hipEvent_t> g_pool;
static size_t g_pool_next = 0;
static thread_local hipEvent_t g_open_end = nullptr;   // end event of the launch this thread is bracketing

static hipEvent_t pool_event() {
    if (g_pool_next == g_pool.size()) {
        hipEvent_t e;
        hipEventCreate(&e);
        g_pool.push_back(e);
    }
    return g_pool[g_pool_next++];
}

void prof_begin(int id, hipStream_t st) {
    if (!g_prof_on.load(std::memory_order_relaxed)) return;
    if (!((g_prof_mask.load(std::memory_order_relaxed) >> id) & 1ull)) return;
    const int every = g_prof_every.load(std::memory_order_relaxed);
    if (every > 1 && g_prof_seen[id].fetch_add(1u, std::memory_order_relaxed) % (unsigned)every != 0u) return;
    ProfRec r;
    {
        std::lock_guard<std::mutex> lk(g_prof_mu);
        r.id = id; r.a = pool_event(); r.b = pool_event();
        g_prof.push_back(r);
    }
    hipEventRecord(r.a, st);
    g_open_end = r.b;
}
void prof_end(hipStream_t st) {
    if (!g_open_end) return;
    hipEventRecord(g_open_end, st);
    g_open_end = nullptr;
}

static TileMap make_tilemap(int mode, int B, int S, int N) {
    TileMap tm;
    tm.mode = mode;
    tm.N = N;
    tm.nshift = -1;
    for (int sh = 0; sh < 31; ++sh) if ((1 << sh) == N) tm.nshift = sh;
    tm.T = S * N;
    tm.L = mode == MSST_MODE_SPATIAL ? N : S;
    tm.TS = 64 / tm.L;
    tm.nseq = mode == MSST_MODE_SPATIAL ? B * S : B * N;
    return tm;
}

static Drop make_drop(float p, uint32_t seed, int layer) {
    Drop d;
    d.seed = seed; d.layer = layer;
    if (p > 0.f) {
        d.thr = (unsigned)(p * 65536.0f + 0.5f);
        if (d.thr > 65535u) d.thr = 65535u;   // the kernels test whole words against thr << 16 (p >= 1 is degenerate anyway)
        d.scale = 1.0f / (1.0f - (float)d.thr / 65536.0f);   // exact inverse of the realised keep probability
    } else {
        d.thr = 0; d.scale = 1.0f;
    }
    return d;
}

static int ntiles_of(const TileMap& tm) { return (tm.nseq + tm.TS - 1) / tm.TS; }

// shape of a block call, checked before its pointers, its tile map (64 / L) or any launch: 0, MSST_ERR_BADARG (a size below 1 or a
// mode outside {spatial, spectral}) or MSST_ERR_UNSUPPORTED (a sequence longer than one 64-row tile)
static int block_shape(int mode, int B, int S, int N, int heads) {
    if (B < 1 || S < 1 || N < 1 || heads < 1 || (mode != MSST_MODE_SPATIAL && mode != MSST_MODE_SPECTRAL)) return MSST_ERR_BADARG;
    if (N > 64 || S > 64) return MSST_ERR_UNSUPPORTED;
    return 0;
}

static bool bw_ok(const MsstBlockWeights* w) { return w && w->struct_bytes == sizeof(MsstBlockWeights); }

static BlockWeights to_bw(const MsstBlockWeights* w) {
    BlockWeights b;
    b.wqkv = w->wqkv; b.wout = w->wout; b.w1 = w->w1; b.w2 = w->w2;
    b.wqkvT = w->wqkvT; b.woutT = w->woutT; b.w1T = w->w1T; b.w2T = w->w2T;
    b.ln1_g = w->ln1_g; b.ln1_b = w->ln1_b; b.bo = w->bo;
    b.ln2_g = w->ln2_g; b.ln2_b = w->ln2_b; b.b1 = w->b1; b.b2 = w->b2;
    b.wqkv32 = w->wqkv32; b.woutT32 = w->woutT32; b.wqkvT32 = w->wqkvT32;
    return b;
}

// ------------------------------------------------------------------------------------------
// the tokenizer: host-only pointer groups and window source, one argument check, and the argument blocks filled in one place each
// ------------------------------------------------------------------------------------------
// what every tokenizer entry point reads: the source tensor (a batch, tiles or scenes) and the six parameter tensors
struct TokPtrs {
    const float *img, *pre_g, *pre_b, *w_emb, *b_emb, *post_g, *post_b;
    bool all_set() const { return img && pre_g && pre_b && w_emb && b_emb && post_g && post_b; }
};
// where a parameter backward writes: the six parameter gradients, the position tables' (dpos_a null: applied by the caller) and the
// mask token's (null: none)
struct TokGradPtrs {
    float *dpre_g, *dpre_b, *dw_emb, *db_emb, *dpost_g, *dpost_b, *dpos_a, *dpos_b;
    int pos_split;
    float* dmask_token;
    bool all_set() const { return dpre_g && dpre_b && dw_emb && db_emb && dpost_g && dpost_b && (dpos_b || !pos_split || !dpos_a); }
};
// where the samples of a call lie in scenes [Bs][S*P][Hs][Ws]: sample b is window win0 + b of the grid (window, stride), row-major over
// (scene, window row, window column) -- the checks fill nq (windows per window row) and wps (windows per scene) -- or, listed, the
// window at origins[b] = (scene, y0, x0): stride = window, win0 = 0, of which the kernels read only Hs, Ws and window
struct WinSrc {
    int Bs, Hs, Ws, window, stride;
    long win0;
    int nwin;
    bool listed = false;
    const int32_t* origins = nullptr;
    int nq = 1;
    long wps = 1;
    bool oriented = false;            // listed windows, each in orientation orient[b] (the _orient entry points): the table is required
    const uint8_t* orient = nullptr;
    int kind() const { return oriented ? WIN_LISTED_ORIENTED : listed ? WIN_LISTED : WIN_GRID; }   // of the kernels (msst_kernels.h)
};
// window grid of a scene: false when the shapes are not a valid (scene, window, stride) triple
static bool scene_grid(int Bs, int Hs, int Ws, int window, int stride, int* nr, int* nq) {
    if (Bs < 1 || window < 1 || stride < 1 || stride > window || Hs < window || Ws < window) return false;
    *nr = (Hs - window) / stride + 1;
    *nq = (Ws - window) / stride + 1;
    return true;
}
// the argument check of every training entry point over a window source, in this order: sizes below 1 (BADARG), shapes outside the
// kernels' limits (UNSUPPORTED), a null required pointer (the caller's `pointers`; a listed source's tables count) or a pos_split outside
// [0, 96) (BADARG), windows beyond the scenes' grids (BADARG; the value ranges of a listed table are the caller's guarantee).
// min_nwin: 0 or 1
static int check_src(WinSrc& w, bool pointers, int min_nwin, int S, int P, int pos_split) {
    if (w.Bs < 1 || w.Hs < 1 || w.Ws < 1 || w.window < 1 || w.stride < 1 || S < 1 || P < 1 || w.nwin < min_nwin || w.win0 < 0)
        return MSST_ERR_BADARG;
    if (w.stride > w.window || w.window > w.Hs || w.window > w.Ws || w.window > 8 || P > 16) return MSST_ERR_UNSUPPORTED;   // 8: at most 64 pixels per window
    if (!pointers || (w.listed && !w.origins) || (w.oriented && !w.orient) || pos_split < 0 || pos_split >= 96) return MSST_ERR_BADARG;
    if (w.listed) return 0;
    int nr = 0;
    scene_grid(w.Bs, w.Hs, w.Ws, w.window, w.stride, &nr, &w.nq);
    w.wps = (long)nr * w.nq;
    return (w.wps > 0x7fffffffL || w.win0 + w.nwin > (long)w.Bs * w.wps) ? MSST_ERR_BADARG : 0;
}

// msst_last_error names the entry point that was called (`what`), then what it refused
static int fail(int code, const char* what, const char* suffix) {
    char buf[128];
    snprintf(buf, sizeof(buf), "%s%s", what, suffix);
    return fail(code, buf);
}

// what TokArgs, TokBwdArgs and TokInArgs share: the source tensor, the parameters, the shape, the dropout stream; the blocks come
// zeroed (no window grid, no tables: fill_src adds them)
template <class Args>
static void fill_tok_common(Args& a, const TokPtrs& p, int B, int S, int N, int P, Drop drop) {
    a.src.base = p.img; a.pre_g = p.pre_g; a.pre_b = p.pre_b; a.w_emb = p.w_emb; a.b_emb = p.b_emb; a.post_g = p.post_g; a.post_b = p.post_b;
    a.B = B; a.S = S; a.N = N; a.T = S * N; a.P = P; a.drop = drop;
}
static void fill_tok(TokArgs& a, const TokPtrs& p, const float* pos_a, const float* pos_b, int pos_split, const float* mask_token,
                     const uint8_t* mask, float* out, int B, int S, int N, int P, Drop drop) {
    fill_tok_common(a, p, B, S, N, P, drop);
    a.pos_a = pos_a; a.pos_b = pos_b; a.mask_token = mask_token; a.mask = mask; a.out = out; a.pos_split = pos_split;
}
static void fill_tok_in(TokInArgs& a, const TokPtrs& p, const uint8_t* mask, const float* dx0, const float* dtarget, float* dimg, int B,
                        int S, int N, int P, Drop drop) {
    fill_tok_common(a, p, B, S, N, P, drop);
    a.mask = mask; a.dx0 = dx0; a.dtarget = dtarget; a.dimg = dimg;
}
// where the windows lie, into the argument block's source (its base is already set)
static void fill_src(WinRef& r, const WinSrc& w) {
    r.win0 = w.win0; r.Hs = w.Hs; r.Ws = w.Ws; r.win = w.window; r.stride = w.stride; r.nq = w.nq; r.wps = (int)w.wps;
    r.origins = w.origins; r.orient = w.orient;
}

// the window grid of an assemble call into its argument block
static void fill_grid(SceneGrid& g, long win0, int nwin, int Bs, int Hs, int Ws, int window, int stride, int nr, int nq) {
    g.win0 = win0; g.row0 = 0; g.nwin = nwin; g.Bs = Bs; g.Hs = Hs; g.Ws = Ws; g.win = window; g.stride = stride; g.nr = nr; g.nq = nq;
}
// the flattened (scene, pixel row) rows the windows of a call reach: first window's top row .. last window's bottom row.  Sets
// g.row0 and returns the pixels of those rows (0 for a call without windows): the launch size of launch_scene_fold
static long scene_call_rows(SceneGrid& g, long wps) {
    if (g.nwin < 1) return 0;
    const long g0 = g.win0, g1 = g.win0 + g.nwin - 1;
    const long s0 = g0 / wps, s1 = g1 / wps;
    const long r0 = (g0 - s0 * wps) / g.nq, r1 = (g1 - s1 * wps) / g.nq;
    g.row0 = s0 * g.Hs + r0 * g.stride;
    const long rows = s1 * g.Hs + r1 * g.stride + g.win - g.row0;
    return rows * g.Ws;
}

}  // namespace msst

using namespace msst;

extern "C" {

// a kernel-study build (-DMSST_LAB: timing modes that compute wrong results can be compiled in) identifies itself with a
// negative version; maskedsst_amd/_lib.py refuses to load it
#ifdef MSST_LAB
int msst_version(void) { return -MSST_VERSION; }
#else
int msst_version(void) { return MSST_VERSION; }
#endif
const char* msst_last_error(void) { return g_err; }

int msst_debug_stamps(void* buf) {
#if defined(MSST_STAMPS) || defined(MSST_LAB)
    g_stamps = (unsigned long long*)buf;
    return 0;
#else
    (void)buf;
    return fail(MSST_ERR_UNSUPPORTED, "msst_debug_stamps (library built without -DMSST_STAMPS)");
#endif
}

int msst_debug_cu_thief(int nblocks, int microseconds, void* sink, void* stream) {
    return fail(launch_cu_thief(nblocks, microseconds, (unsigned*)sink, (hipStream_t)stream), "msst_debug_cu_thief");
}

int msst_debug_box_probe(double* out4, void* scratch, long scratch_bytes, void* stream) {
    return fail(launch_box_probe(out4, scratch, scratch_bytes, (hipStream_t)stream), "msst_debug_box_probe");
}

int msst_profile_enable(int on) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (on) { g_prof.clear(); g_pool_next = 0; }
    g_prof_on.store(on != 0);
    return 0;
}

int msst_profile_select(unsigned long long mask) { g_prof_mask.store(mask); return 0; }

int msst_profile_sample(int every) {
    if (every < 1) return fail(MSST_ERR_BADARG, "msst_profile_sample");
    g_prof_every.store(every);
    for (int i = 0; i < K_COUNT; ++i) g_prof_seen[i].store(0u);
    return 0;
}

int msst_profile_kernels(void) { return K_COUNT; }

const char* msst_profile_name(int id) {
    static const char* names[K_COUNT] = {"prep_weights", "tokenize_fwd", "block_fwd", "head_fwd", "loss_reduce",
                                         "head_bwd", "reduce_slabs", "block_bwd_mlp", "block_bwd_attn",
                                         "attn_slab_reduce", "block_bwd_ln1", "tokenize_bwd", "pos_split", "adamw", "block_bwd_ln1mlp", "layernorm", "adam_groups", "cross_entropy", "recon_fwd",
                                         "tokenize_bwd_input", "head_bwd_target", "grad_accumulate", "grad_finalize"};
    return (id >= 0 && id < K_COUNT) ? names[id] : "?";
}

int msst_profile_collect(double* total_ms, long* count) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (int i = 0; i < K_COUNT; ++i) { total_ms[i] = 0.0; count[i] = 0; }
    for (const ProfRec& r : g_prof) {
        if (hipEventSynchronize(r.b) != hipSuccess) return fail(MSST_ERR_BADARG, "msst_profile_collect");
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) continue;
        total_ms[r.id] += ms;
        count[r.id] += 1;
    }
    g_prof.clear();
    g_pool_next = 0;
    return 0;
}

int msst_prep_weights(const MsstPrepJob* jobs, int njobs, int job_bytes, int max_elems, int prec, int32_t* err_flag, void* stream) {
    // a caller built against another revision of MsstPrepJob would hand over a mis-strided table: refused on the host
    if (job_bytes != (int)sizeof(MsstPrepJob)) return fail(MSST_ERR_BADARG, "msst_prep_weights (MsstPrepJob of another header revision)");
    if (njobs <= 0) return 0;
    if (!jobs) return fail(MSST_ERR_BADARG, "msst_prep_weights");
    ProfScope ps(K_PREP, (hipStream_t)stream);
    int gx = (max_elems + 256 * 4 - 1) / (256 * 4);
    if (gx < 1) gx = 1;
    if (gx > 64) gx = 64;
    dim3 grid(gx, njobs);
    if (prec == MSST_PREC_F32) hipLaunchKernelGGL(prep_weights_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, jobs, (int*)err_flag);
    else hipLaunchKernelGGL(prep_weights_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, jobs, (int*)err_flag);
    return fail((int)hipGetLastError(), "msst_prep_weights");
}

int msst_tokenize_fwd(const float* img, const float* pre_g, const float* pre_b, const float* w_emb,
                      const float* b_emb, const float* post_g, const float* post_b, const float* pos_a,
                      const float* pos_b, int pos_split, const float* mask_token, const uint8_t* mask,
                      float* out, int B, int S, int N, int P, float emb_dropout_p, uint32_t seed, void* stream) {
    TokArgs a{};
    fill_tok(a, {img, pre_g, pre_b, w_emb, b_emb, post_g, post_b}, pos_a, pos_b, pos_split, mask_token, mask, out, B, S, N, P,
             make_drop(emb_dropout_p, seed, 255));
    return fail(launch_tokenize_fwd(a, WIN_BATCH, MASK_TOKENS, (hipStream_t)stream), "msst_tokenize_fwd");
}

// the two inference forwards over a scene's window grid (no dropout; masked: the scene mask and the mask token).  Their own precedence:
// BADARG for everything, a stride above the window included, then UNSUPPORTED for a window of more than 64 pixels
static int tokenize_scene_fwd(const char* what, bool masked, const TokPtrs& p, const float* pos_a, const float* pos_b, int pos_split,
                              const float* mask_token, const uint8_t* scene_mask, float* out, WinSrc w, int S, int P, void* stream) {
    int nr = 0;
    if (!p.img || !out || (masked && (!mask_token || !scene_mask)) || S < 1 || P < 1 || w.nwin < 0 || w.win0 < 0 ||
        !scene_grid(w.Bs, w.Hs, w.Ws, w.window, w.stride, &nr, &w.nq))
        return fail(MSST_ERR_BADARG, what);
    w.wps = (long)nr * w.nq;
    if (w.wps > 0x7fffffffL || w.win0 + w.nwin > (long)w.Bs * w.wps) return fail(MSST_ERR_BADARG, what, " (windows out of range)");
    if (w.window > 8) return fail(MSST_ERR_UNSUPPORTED, what, " (more than 64 pixels per window)");
    TokArgs a{};
    fill_tok(a, p, pos_a, pos_b, pos_split, mask_token, scene_mask, out, w.nwin, S, w.window * w.window, P, make_drop(0.f, 0, 255));
    fill_src(a.src, w);
    return fail(launch_tokenize_fwd(a, WIN_GRID, masked ? MASK_SCENE : MASK_NONE, (hipStream_t)stream), what);
}

int msst_tokenize_scene_fwd(const float* scene, const float* pre_g, const float* pre_b, const float* w_emb,
                            const float* b_emb, const float* post_g, const float* post_b, const float* pos_a,
                            const float* pos_b, int pos_split, float* out, int Bs, int Hs, int Ws, int window, int stride,
                            long win0, int nwin, int S, int P, void* stream) {
    return tokenize_scene_fwd("msst_tokenize_scene_fwd", false, {scene, pre_g, pre_b, w_emb, b_emb, post_g, post_b}, pos_a, pos_b,
                              pos_split, nullptr, nullptr, out, WinSrc{Bs, Hs, Ws, window, stride, win0, nwin}, S, P, stream);
}

int msst_tokenize_scene_fwd_masked(const float* scene, const float* pre_g, const float* pre_b, const float* w_emb,
                                   const float* b_emb, const float* post_g, const float* post_b, const float* pos_a,
                                   const float* pos_b, int pos_split, const float* mask_token, const uint8_t* scene_mask, float* out,
                                   int Bs, int Hs, int Ws, int window, int stride, long win0, int nwin, int S, int P, void* stream) {
    return tokenize_scene_fwd("msst_tokenize_scene_fwd_masked", true, {scene, pre_g, pre_b, w_emb, b_emb, post_g, post_b}, pos_a, pos_b,
                              pos_split, mask_token, scene_mask, out, WinSrc{Bs, Hs, Ws, window, stride, win0, nwin}, S, P, stream);
}

// the training forwards over a window source: a grid (no mask), listed windows, listed windows with a per-window token mask
static int tokenize_src_fwd(const char* what, bool masked, const TokPtrs& p, const float* pos_a, const float* pos_b, int pos_split,
                            const float* mask_token, const uint8_t* mask, float* out, WinSrc w, int S, int P, Drop drop, void* stream) {
    const bool pointers = p.all_set() && pos_a && (pos_b || !pos_split) && (!masked || (mask_token && mask)) && out;
    if (int rc = check_src(w, pointers, 0, S, P, pos_split)) return fail(rc, what);
    if (w.listed && (P != 10 || w.window != 8) && w.nwin > 65535) return fail(MSST_ERR_UNSUPPORTED, what, " (more than 65535 windows)");
    TokArgs a{};
    fill_tok(a, p, pos_a, pos_b, pos_split, mask_token, mask, out, w.nwin, S, w.window * w.window, P, drop);
    fill_src(a.src, w);
    return fail(launch_tokenize_fwd(a, w.kind(), masked ? MASK_TOKENS : MASK_NONE, (hipStream_t)stream), what);
}

int msst_tokenize_scene_fwd_train(const float* scene, const float* pre_g, const float* pre_b, const float* w_emb,
                                  const float* b_emb, const float* post_g, const float* post_b, const float* pos_a,
                                  const float* pos_b, int pos_split, float* out, int Bs, int Hs, int Ws, int window, int stride,
                                  long win0, int nwin, int S, int P, float emb_dropout_p, uint32_t seed, void* stream) {
    return tokenize_src_fwd("msst_tokenize_scene_fwd_train", false, {scene, pre_g, pre_b, w_emb, b_emb, post_g, post_b}, pos_a, pos_b,
                            pos_split, nullptr, nullptr, out, WinSrc{Bs, Hs, Ws, window, stride, win0, nwin}, S, P,
                            make_drop(emb_dropout_p, seed, 255), stream);
}

int msst_tokenize_at_fwd(const float* scene, const int32_t* origins, const float* pre_g, const float* pre_b, const float* w_emb,
                         const float* b_emb, const float* post_g, const float* post_b, const float* pos_a, const float* pos_b,
                         int pos_split, float* out, int Bs, int Hs, int Ws, int window, int nwin, int S, int P,
                         float emb_dropout_p, uint32_t seed, void* stream) {
    return tokenize_src_fwd("msst_tokenize_at_fwd", false, {scene, pre_g, pre_b, w_emb, b_emb, post_g, post_b}, pos_a, pos_b, pos_split,
                            nullptr, nullptr, out, WinSrc{Bs, Hs, Ws, window, window, 0, nwin, true, origins}, S, P,
                            make_drop(emb_dropout_p, seed, 255), stream);
}

int msst_tokenize_at_fwd_masked(const float* scene, const int32_t* origins, const float* pre_g, const float* pre_b, const float* w_emb,
                                const float* b_emb, const float* post_g, const float* post_b, const float* pos_a, const float* pos_b,
                                int pos_split, const float* mask_token, const uint8_t* mask, float* out, int Bs, int Hs, int Ws,
                                int window, int nwin, int S, int P, void* stream) {
    return tokenize_src_fwd("msst_tokenize_at_fwd_masked", true, {scene, pre_g, pre_b, w_emb, b_emb, post_g, post_b}, pos_a, pos_b,
                            pos_split, mask_token, mask, out, WinSrc{Bs, Hs, Ws, window, window, 0, nwin, true, origins}, S, P, make_drop(0.f, 0, 255),
                            stream);
}

int msst_tokenize_at_fwd_orient(const float* scene, const int32_t* origins, const uint8_t* orient, const float* pre_g, const float* pre_b,
                                const float* w_emb, const float* b_emb, const float* post_g, const float* post_b, const float* pos_a,
                                const float* pos_b, int pos_split, float* out, int Bs, int Hs, int Ws, int window, int nwin, int S, int P,
                                float emb_dropout_p, uint32_t seed, void* stream) {
    return tokenize_src_fwd("msst_tokenize_at_fwd_orient", false, {scene, pre_g, pre_b, w_emb, b_emb, post_g, post_b}, pos_a, pos_b,
                            pos_split, nullptr, nullptr, out, WinSrc{Bs, Hs, Ws, window, window, 0, nwin, true, origins, 1, 1, true, orient}, S, P,
                            make_drop(emb_dropout_p, seed, 255), stream);
}

int msst_tokenize_at_fwd_masked_orient(const float* scene, const int32_t* origins, const uint8_t* orient, const float* pre_g,
                                       const float* pre_b, const float* w_emb, const float* b_emb, const float* post_g,
                                       const float* post_b, const float* pos_a, const float* pos_b, int pos_split,
                                       const float* mask_token, const uint8_t* mask, float* out, int Bs, int Hs, int Ws, int window,
                                       int nwin, int S, int P, void* stream) {
    return tokenize_src_fwd("msst_tokenize_at_fwd_masked_orient", true, {scene, pre_g, pre_b, w_emb, b_emb, post_g, post_b}, pos_a, pos_b,
                            pos_split, mask_token, mask, out, WinSrc{Bs, Hs, Ws, window, window, 0, nwin, true, origins, 1, 1, true, orient}, S, P,
                            make_drop(0.f, 0, 255), stream);
}

int msst_scene_assemble(const float* win_logits, long win0, int nwin, float* logits, int64_t* classes, int Bs,
                        int n_classes, int Hs, int Ws, int window, int stride, int finalize, void* stream) {
    int nr = 0, nq = 0;
    if (!logits || (finalize && !classes) || (nwin > 0 && !win_logits) || n_classes < 1 || nwin < 0 || win0 < 0 ||
        !scene_grid(Bs, Hs, Ws, window, stride, &nr, &nq))
        return fail(MSST_ERR_BADARG, "msst_scene_assemble");
    const long wps = (long)nr * nq;
    if (win0 + nwin > (long)Bs * wps) return fail(MSST_ERR_BADARG, "msst_scene_assemble (windows out of range)");
    SceneArgs a;
    fill_grid(a, win0, nwin, Bs, Hs, Ws, window, stride, nr, nq);
    a.win_logits = win_logits; a.logits = logits; a.classes = classes; a.NC = n_classes;
    hipStream_t st = (hipStream_t)stream;
    int rc = launch_scene_fold(a, win_logits, logits, n_classes, 16, scene_call_rows(a, wps), st);
    if (!rc && finalize) rc = launch_scene_finalize(a, st);
    return fail(rc, "msst_scene_assemble");
}

int msst_scene_recon_assemble(const float* win_recon, long win0, int nwin, const float* scene, const uint8_t* scene_mask, float* cube,
                              double* band_err, int32_t* band_cnt, int32_t* cover, int Bs, int S, int P, int Hs, int Ws, int window,
                              int stride, int finalize, int blend, void* stream) {
    if (Bs < 1 || S < 1 || P < 1 || Hs < 1 || Ws < 1 || window < 1 || stride < 1 || nwin < 0 || win0 < 0)
        return fail(MSST_ERR_BADARG, "msst_scene_recon_assemble");
    if (stride > window || window > Hs || window > Ws || window * window > 64 || S > 64 || P > 16)
        return fail(MSST_ERR_UNSUPPORTED, "msst_scene_recon_assemble (1 <= stride <= window <= Hs, Ws; window * window <= 64, S <= 64, P <= 16)");
    if ((nwin > 0 && !win_recon) || !scene || !scene_mask || !cube || !cover || (band_err == nullptr) != (band_cnt == nullptr))
        return fail(MSST_ERR_BADARG, "msst_scene_recon_assemble (null argument, or one of band_err / band_cnt without the other)");
    int nr = 0, nq = 0;
    scene_grid(Bs, Hs, Ws, window, stride, &nr, &nq);
    const long wps = (long)nr * nq;
    if (win0 + nwin > (long)Bs * wps) return fail(MSST_ERR_BADARG, "msst_scene_recon_assemble (windows out of range)");
    // both launches' grids fit (so nothing is refused after the first one is enqueued)
    if (((long)Bs * Hs * Ws + 255) / 256 > 0x7fffffffL || (long)Bs * S * P > 0x7fffffffL) return fail(MSST_ERR_UNSUPPORTED, "msst_scene_recon_assemble (scene batch too large)");
    SceneReconArgs a;
    fill_grid(a, win0, nwin, Bs, Hs, Ws, window, stride, nr, nq);
    a.win_recon = win_recon; a.scene = scene; a.scene_mask = scene_mask; a.cube = cube; a.band_err = band_err; a.band_cnt = band_cnt;
    a.cover = cover; a.S = S; a.P = P; a.blend = blend != 0;
    hipStream_t st = (hipStream_t)stream;
    int rc = launch_scene_fold(a, win_recon, cube, S * P, P, scene_call_rows(a, wps), st);   // a spectral block's P bands per grid row
    if (!rc && finalize) rc = launch_scene_recon_finalize(a, st);
    return fail(rc, "msst_scene_recon_assemble");
}

int msst_pool_spectral_fwd(const float* y, float* out, int B, int S, int N, void* stream) {
    if (B < 1 || S < 1 || N < 1) return fail(MSST_ERR_BADARG, "msst_pool_spectral_fwd");
    if (N > 64 || S > 64) return fail(MSST_ERR_UNSUPPORTED, "msst_pool_spectral_fwd (N <= 64, S <= 64)");
    if (!y || !out || ((uintptr_t)y & 15)) return fail(MSST_ERR_BADARG, "msst_pool_spectral_fwd (null argument, or y not 16-byte aligned)");
    return fail(launch_pool_spectral(y, out, B, S, N, (hipStream_t)stream), "msst_pool_spectral_fwd");
}

int msst_draw_masks(uint8_t* mask, int32_t* idx, int32_t* csr_ptr, int32_t* csr_pos, uint32_t seed, long row0, int rows, int S, int N,
                    int K, int mode, int rand_size, int scale, int mask_count, void* stream) {
    if (rows < 1 || S < 1 || N < 1 || K < 1 || row0 < 0 || row0 > (1L << 48)) return fail(MSST_ERR_BADARG, "msst_draw_masks");
    if (mode != MSST_MASK_TOPK && mode != MSST_MASK_BLOCK && mode != MSST_MASK_TUBE)
        return fail(MSST_ERR_BADARG, "msst_draw_masks (mode outside {0, 1, 2})");
    if (N > 64 || S > 64) return fail(MSST_ERR_UNSUPPORTED, "msst_draw_masks (N <= 64, S <= 64)");
    if (K > S * N) return fail(MSST_ERR_BADARG, "msst_draw_masks (K > S * N)");
    MaskDrawArgs a;
    a.side = a.rand_size = a.scale = a.mask_count = 0;
    if (mode != MSST_MASK_TOPK) {
        if (rand_size < 1 || scale < 1 || rand_size > 8 || scale > 8 || rand_size * scale * rand_size * scale != N)
            return fail(MSST_ERR_BADARG, "msst_draw_masks ((rand_size * scale)^2 is not N)");
        if (mask_count < 1 || mask_count > rand_size * rand_size)
            return fail(MSST_ERR_BADARG, "msst_draw_masks (mask_count outside 1 .. rand_size^2)");
        if (S * mask_count * scale * scale < K) return fail(MSST_ERR_BADARG, "msst_draw_masks (fewer than K trues per row)");
        a.side = rand_size * scale; a.rand_size = rand_size; a.scale = scale; a.mask_count = mask_count;
    }
    if (!mask || !idx || !csr_ptr || !csr_pos) return fail(MSST_ERR_BADARG, "msst_draw_masks (null argument)");
    a.mask = mask; a.idx = idx; a.csr_ptr = csr_ptr; a.csr_pos = csr_pos; a.seed = seed; a.row0 = row0;
    a.rows = rows; a.S = S; a.N = N; a.K = K; a.mode = mode;
    return fail(launch_draw_masks(a, (hipStream_t)stream), "msst_draw_masks");
}

int msst_attn_maps(const float* x, const float* ln_g, const float* ln_b, const float* wqkv, float* maps, long sample_stride, int mode,
                   int B, int S, int N, int heads, int reduce, void* stream) {
    if (B < 1 || S < 1 || N < 1 || heads < 1) return fail(MSST_ERR_BADARG, "msst_attn_maps");
    if (N > 64 || S > 64 || heads > 16) return fail(MSST_ERR_UNSUPPORTED, "msst_attn_maps (N <= 64, S <= 64, heads <= 16)");
    if ((mode != MSST_MODE_SPATIAL && mode != MSST_MODE_SPECTRAL) || (reduce != MSST_ATTN_PER_SEQ && reduce != MSST_ATTN_MEAN_SEQ))
        return fail(MSST_ERR_BADARG, "msst_attn_maps (mode or reduce outside {0, 1})");
    if (!x || !ln_g || !ln_b || !wqkv || !maps || ((uintptr_t)x & 15) || ((uintptr_t)maps & 15))
        return fail(MSST_ERR_BADARG, "msst_attn_maps (null argument, or x / maps not 16-byte aligned)");
    const long L = mode == MSST_MODE_SPATIAL ? N : S, G = mode == MSST_MODE_SPATIAL ? S : N;
    if (sample_stride < (reduce == MSST_ATTN_PER_SEQ ? G : 1) * heads * L * L)
        return fail(MSST_ERR_BADARG, "msst_attn_maps (sample_stride smaller than one sample's maps)");
    return fail(launch_attn_maps(x, ln_g, ln_b, wqkv, maps, sample_stride, mode, B, S, N, heads, reduce, (hipStream_t)stream),
                "msst_attn_maps");
}

// ---- the entry points on frozen per-pixel features (msst_knn.hip, msst_probe.hip, msst_kmeans.hip) share two checks.
// The sizes of a call on rows [row0, row0 + rows) of M feature rows with n classes or clusters: sizes first (MSST_ERR_BADARG), then what
// the kernels do not take (MSST_ERR_UNSUPPORTED), then the metric (k-means only); pointers are the caller's next check.  `sizes` is the
// text of the first and last refusal, `n_name` and `rows_name` are what the entry point calls n and M.
static int feat_shape(const char* what, const char* sizes, const char* n_name, const char* rows_name, long M, int dim, long row0, long rows,
                      int n, int metric = MSST_KMEANS_COSINE) {
    char buf[96];
    int rc = 0;
    if (M < 1 || dim < 1 || rows < 1 || row0 < 0 || row0 > M || rows > M - row0 || n < 1) rc = MSST_ERR_BADARG;
    else if (dim != 96 || n > 128 || M > 2147483647L) rc = MSST_ERR_UNSUPPORTED;
    else if (metric != MSST_KMEANS_COSINE && metric != MSST_KMEANS_EUCLIDEAN) rc = MSST_ERR_BADARG;
    if (rc == MSST_ERR_BADARG) snprintf(buf, sizeof(buf), " (%s)", sizes);
    else snprintf(buf, sizeof(buf), " (dim == 96, %s <= 128, %s <= 2^31 - 1)", n_name, rows_name);
    return rc ? fail(rc, what, buf) : 0;
}

// A layout is 0 (rows) or 1 (an encode_scene map, whose plane must divide the row count); `arg` and `rows_name` are the entry point's names
static int feat_layout(const char* what, const char* arg, const char* rows_name, long rows, long plane, int layout, int layout2 = 0) {
    char buf[64];
    if ((layout != 0 && layout != 1) || (layout2 != 0 && layout2 != 1)) {
        snprintf(buf, sizeof(buf), " (%s outside {0, 1})", arg);
        return fail(MSST_ERR_BADARG, what, buf);
    }
    if ((layout == 1 || layout2 == 1) && (plane < 1 || rows % plane)) {
        snprintf(buf, sizeof(buf), " (plane does not divide %s)", rows_name);
        return fail(MSST_ERR_BADARG, what, buf);
    }
    return 0;
}

long msst_knn_scratch_bytes(long Q, long M, int k, int splits) {
    if (Q < 1 || M < 1 || k < 1 || splits < 0) return 0;
    return knn_scratch_bytes(Q, M, k, splits);
}

int msst_knn_topk(const float* bank, long M, int dim, const float* queries, int q_layout, long Q, long plane, int k, int splits,
                  int32_t* nbr_idx, float* nbr_sim, void* scratch, long scratch_bytes, void* stream) {
    if (M < 1 || dim < 1 || Q < 0 || splits < 0) return fail(MSST_ERR_BADARG, "msst_knn_topk");
    if (dim != 96 || k < 1 || k > 64 || splits > 64 || M > 2147483647L || Q > 2147483647L)
        return fail(MSST_ERR_UNSUPPORTED, "msst_knn_topk (dim == 96, 1 <= k <= 64, splits <= 64, Q and M <= 2^31 - 1)");
    if (int rc = feat_layout("msst_knn_topk", "q_layout", "Q", Q, plane, q_layout)) return rc;
    if (Q == 0) return 0;
    if (!bank || !queries || !nbr_idx || !nbr_sim || ((uintptr_t)bank & 15) || ((uintptr_t)queries & 3) || ((uintptr_t)nbr_idx & 3) ||
        ((uintptr_t)nbr_sim & 3))
        return fail(MSST_ERR_BADARG, "msst_knn_topk (null or misaligned argument)");
    const long need = knn_scratch_bytes(Q, M, k, splits);
    if (scratch_bytes < need || (need > 0 && (!scratch || ((uintptr_t)scratch & 15))))
        return fail(MSST_ERR_BADARG, "msst_knn_topk (scratch null, misaligned or smaller than msst_knn_scratch_bytes)");
    return fail(launch_knn_topk(bank, M, queries, q_layout, Q, plane, k, splits, nbr_idx, nbr_sim, scratch, (hipStream_t)stream),
                "msst_knn_topk");
}

int msst_knn_vote(const int32_t* nbr_idx, const float* nbr_sim, const int32_t* bank_labels, long Q, int k, int n_classes,
                  float temperature, float* votes, int vote_layout, long plane, int64_t* classes, void* stream) {
    if (Q < 0 || n_classes < 1) return fail(MSST_ERR_BADARG, "msst_knn_vote");
    if (k < 1 || k > 64 || n_classes > 128 || Q > 2147483647L)
        return fail(MSST_ERR_UNSUPPORTED, "msst_knn_vote (1 <= k <= 64, n_classes <= 128, Q <= 2^31 - 1)");
    if (int rc = feat_layout("msst_knn_vote", "vote_layout", "Q", Q, plane, vote_layout)) return rc;
    if (!(temperature >= 0.f)) return fail(MSST_ERR_BADARG, "msst_knn_vote (negative temperature)");
    if (Q == 0) return 0;
    if (!nbr_idx || !nbr_sim || !bank_labels || !votes || !classes || ((uintptr_t)nbr_idx & 3) || ((uintptr_t)nbr_sim & 3) ||
        ((uintptr_t)bank_labels & 3) || ((uintptr_t)votes & 3) || ((uintptr_t)classes & 7))
        return fail(MSST_ERR_BADARG, "msst_knn_vote (null or misaligned argument)");
    return fail(launch_knn_vote(nbr_idx, nbr_sim, bank_labels, Q, k, n_classes, temperature, votes, vote_layout, plane, classes,
                                (hipStream_t)stream), "msst_knn_vote");
}

long msst_probe_scratch_floats(long rows, int nc) {
    if (rows < 1 || nc < 1 || nc > 128) return 0;
    return probe_scratch_floats(rows, nc);
}

int msst_probe_grad(const float* x, const int32_t* labels, const float* class_w, const float* theta, long M, int dim, long row0, long rows,
                    int nc, float* slab, long slab_floats, void* stream) {
    if (int rc = feat_shape("msst_probe_grad", "a size below 1 or rows outside [0, M)", "nc", "M", M, dim, row0, rows, nc)) return rc;
    if (!x || !labels || !theta || !slab || ((uintptr_t)x & 15) || ((uintptr_t)labels & 3) || ((uintptr_t)class_w & 3) ||
        ((uintptr_t)theta & 3) || ((uintptr_t)slab & 3))
        return fail(MSST_ERR_BADARG, "msst_probe_grad (null or misaligned argument)");
    if (slab_floats < probe_scratch_floats(rows, nc)) return fail(MSST_ERR_BADARG, "msst_probe_grad (slab smaller than msst_probe_scratch_floats)");
    return fail(launch_probe_grad(x, labels, class_w, theta, row0, rows, nc, slab, (hipStream_t)stream), "msst_probe_grad");
}

int msst_probe_update(const float* slab, long slab_floats, long rows, int dim, int nc, float* theta, float* m, float* v, int32_t* step,
                      double lr, double beta1, double beta2, double eps, double weight_decay, float* history_row, float* grad_out,
                      int apply, void* stream) {
    if (int rc = feat_shape("msst_probe_update", "a size below 1", "nc", "rows", rows, dim, 0, rows, nc)) return rc;
    if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || !(weight_decay >= 0.0))
        return fail(MSST_ERR_BADARG, "msst_probe_update (lr, eps, weight_decay >= 0 and betas in [0, 1))");
    if (!slab || !history_row || ((uintptr_t)slab & 3) || ((uintptr_t)history_row & 3) || ((uintptr_t)grad_out & 3) ||
        (apply && (!theta || !m || !v || !step)) || ((uintptr_t)theta & 3) || ((uintptr_t)m & 3) || ((uintptr_t)v & 3) || ((uintptr_t)step & 3))
        return fail(MSST_ERR_BADARG, "msst_probe_update (null or misaligned argument)");
    if (slab_floats < probe_scratch_floats(rows, nc)) return fail(MSST_ERR_BADARG, "msst_probe_update (slab smaller than msst_probe_scratch_floats)");
    return fail(launch_probe_update(slab, rows, nc, theta, m, v, step, lr, beta1, beta2, eps, weight_decay, history_row, grad_out,
                                    apply ? 1 : 0, (hipStream_t)stream), "msst_probe_update");
}

int msst_probe_fwd(const float* x, int x_layout, long Q, long plane, const float* theta, int dim, int nc, float* logits, int out_layout,
                   int64_t* classes, void* stream) {
    if (int rc = feat_shape("msst_probe_fwd", "a size below 1", "nc", "Q", Q, dim, 0, Q, nc)) return rc;
    if (int rc = feat_layout("msst_probe_fwd", "layout", "Q", Q, plane, x_layout, out_layout)) return rc;
    if (!x || !theta || !logits || !classes || ((uintptr_t)x & (x_layout == 0 ? 15 : 3)) || ((uintptr_t)theta & 3) || ((uintptr_t)logits & 3) ||
        ((uintptr_t)classes & 7))
        return fail(MSST_ERR_BADARG, "msst_probe_fwd (null or misaligned argument)");
    return fail(launch_probe_fwd(x, x_layout, Q, plane, theta, nc, logits, out_layout, classes, (hipStream_t)stream), "msst_probe_fwd");
}

long msst_kmeans_scratch_floats(long rows, int k) {
    if (rows < 1 || rows > 2147483647L || k < 1 || k > 128) return 0;
    return kmeans_scratch_floats(rows, k);
}

static const char KMEANS_SIZES[] = "a size below 1, or a metric outside {0, 1}";

int msst_kmeans_assign(const float* x, int x_layout, long rows, long plane, int dim, const float* centroids, const float* bias, int k,
                       int metric, int32_t* assign, float* dist, int64_t* classes, float* slab, long slab_floats, void* stream) {
    if (int rc = feat_shape("msst_kmeans_assign", KMEANS_SIZES, "k", "rows", rows, dim, 0, rows, k, metric)) return rc;
    if (int rc = feat_layout("msst_kmeans_assign", "x_layout", "rows", rows, plane, x_layout)) return rc;
    if (!x || !centroids || !bias || !assign || !dist || ((uintptr_t)x & (x_layout == 0 ? 15 : 3)) || ((uintptr_t)centroids & 3) ||
        ((uintptr_t)bias & 3) || ((uintptr_t)assign & 3) || ((uintptr_t)dist & 3) || ((uintptr_t)classes & 7) || ((uintptr_t)slab & 3))
        return fail(MSST_ERR_BADARG, "msst_kmeans_assign (null or misaligned argument)");
    if (slab && slab_floats < kmeans_scratch_floats(rows, k))
        return fail(MSST_ERR_BADARG, "msst_kmeans_assign (slab smaller than msst_kmeans_scratch_floats)");
    return fail(launch_kmeans_assign(x, x_layout, rows, plane, centroids, bias, k, metric, assign, dist, classes, slab, (hipStream_t)stream),
                "msst_kmeans_assign");
}

int msst_kmeans_update(const float* slab, long slab_floats, long rows, int dim, int k, int metric, float* centroids, float* bias,
                       int32_t* counts, float* shift, float* history_row, void* stream) {
    if (int rc = feat_shape("msst_kmeans_update", KMEANS_SIZES, "k", "rows", rows, dim, 0, rows, k, metric)) return rc;
    if (!slab || !centroids || !bias || !counts || !shift || !history_row || ((uintptr_t)slab & 3) || ((uintptr_t)centroids & 3) ||
        ((uintptr_t)bias & 3) || ((uintptr_t)counts & 3) || ((uintptr_t)shift & 3) || ((uintptr_t)history_row & 3))
        return fail(MSST_ERR_BADARG, "msst_kmeans_update (null or misaligned argument)");
    if (slab_floats < kmeans_scratch_floats(rows, k)) return fail(MSST_ERR_BADARG, "msst_kmeans_update (slab smaller than msst_kmeans_scratch_floats)");
    return fail(launch_kmeans_update(slab, rows, k, metric, centroids, bias, counts, shift, history_row, (hipStream_t)stream), "msst_kmeans_update");
}

int msst_kmeans_pick(const float* x, long rows, int dim, const float* dist, const float* slab, long slab_floats, int j, int k, int metric,
                     uint32_t seed, float* centroids, float* bias, int32_t* seed_rows, void* stream) {
    if (j < 0 || (k >= 1 && j >= k) || (rows >= 1 && j >= rows)) return fail(MSST_ERR_BADARG, "msst_kmeans_pick (j outside [0, k), or no row left)");
    if (int rc = feat_shape("msst_kmeans_pick", KMEANS_SIZES, "k", "rows", rows, dim, 0, rows, k, metric)) return rc;
    if (!x || !centroids || !bias || !seed_rows || (j > 0 && (!dist || !slab)) || ((uintptr_t)x & 3) || ((uintptr_t)dist & 3) ||
        ((uintptr_t)slab & 3) || ((uintptr_t)centroids & 3) || ((uintptr_t)bias & 3) || ((uintptr_t)seed_rows & 3))
        return fail(MSST_ERR_BADARG, "msst_kmeans_pick (null or misaligned argument)");
    if (j > 0 && slab_floats < kmeans_scratch_floats(rows, j)) return fail(MSST_ERR_BADARG, "msst_kmeans_pick (slab smaller than msst_kmeans_scratch_floats(rows, j))");
    return fail(launch_kmeans_pick(x, rows, dist, slab, j, metric, seed, centroids, bias, seed_rows, (hipStream_t)stream), "msst_kmeans_pick");
}

long msst_feat_moments_scratch_floats(long rows) {
    if (rows < 1 || rows > 2147483647L) return 0;
    return feat_moments_scratch_floats(rows);
}

// the sizes of the three calls on the moments and projections of frozen features: r is 1 where the call has none
static int pca_shape(const char* what, long rows, int dim, int r, int ddof = 0) {
    if (rows < 1 || dim < 1 || ddof < 0) return fail(MSST_ERR_BADARG, what, " (rows or dim below 1, or a negative ddof)");
    if (dim != 96 || r < 1 || r > 96 || rows > 2147483647L) return fail(MSST_ERR_UNSUPPORTED, what, " (dim == 96, 1 <= r <= 96, rows <= 2^31 - 1)");
    return 0;
}

int msst_feat_moments(const float* x, int x_layout, long rows, long plane, int dim, const float* centre, float* slab, long slab_floats,
                      void* stream) {
    if (int rc = pca_shape("msst_feat_moments", rows, dim, 1)) return rc;
    if (int rc = feat_layout("msst_feat_moments", "x_layout", "rows", rows, plane, x_layout)) return rc;
    if (!x || !slab || ((uintptr_t)x & (x_layout == 0 ? 15 : 3)) || ((uintptr_t)centre & 3) || ((uintptr_t)slab & 3))
        return fail(MSST_ERR_BADARG, "msst_feat_moments (null or misaligned argument)");
    if (slab_floats < feat_moments_scratch_floats(rows))
        return fail(MSST_ERR_BADARG, "msst_feat_moments (slab smaller than msst_feat_moments_scratch_floats)");
    return fail(launch_feat_moments(x, x_layout, rows, plane, centre, slab, (hipStream_t)stream), "msst_feat_moments");
}

int msst_feat_moments_finish(const float* slab, long slab_floats, long rows, int dim, const float* centre, int ddof, int64_t* count,
                             float* mean, float* cov, float* raw, void* stream) {
    if (int rc = pca_shape("msst_feat_moments_finish", rows, dim, 1, ddof)) return rc;
    if (!slab || !count || !mean || ((uintptr_t)slab & 3) || ((uintptr_t)centre & 3) || ((uintptr_t)count & 7) || ((uintptr_t)mean & 3) ||
        ((uintptr_t)cov & 3) || ((uintptr_t)raw & 3))
        return fail(MSST_ERR_BADARG, "msst_feat_moments_finish (null or misaligned argument)");
    if (slab_floats < feat_moments_scratch_floats(rows))
        return fail(MSST_ERR_BADARG, "msst_feat_moments_finish (slab smaller than msst_feat_moments_scratch_floats)");
    return fail(launch_feat_moments_finish(slab, rows, centre, ddof, count, mean, cov, raw, (hipStream_t)stream), "msst_feat_moments_finish");
}

int msst_feat_project(const float* x, int x_layout, long rows, long plane, int dim, const float* mean, const float* components, int r,
                      float* out, int out_layout, float* sumsq, void* stream) {
    if (int rc = pca_shape("msst_feat_project", rows, dim, r)) return rc;
    if (int rc = feat_layout("msst_feat_project", "layout", "rows", rows, plane, x_layout, out_layout)) return rc;
    if (!x || !mean || !components || ((uintptr_t)x & (x_layout == 0 ? 15 : 3)) || ((uintptr_t)mean & 3) || ((uintptr_t)components & 3) ||
        ((uintptr_t)out & 3) || ((uintptr_t)sumsq & 3))
        return fail(MSST_ERR_BADARG, "msst_feat_project (null or misaligned argument)");
    if (!out && !sumsq) return fail(MSST_ERR_BADARG, "msst_feat_project (both outputs null)");
    return fail(launch_feat_project(x, x_layout, rows, plane, mean, components, r, out, out_layout, sumsq, (hipStream_t)stream),
                "msst_feat_project");
}

int msst_gauss_score(const float* x, int x_layout, long rows, long plane, int dim, const float* centres, const float* tables, int n_tables,
                     const int32_t* class_table, const float* offsets, const float* consts, int nc, float max_d2, int32_t* classes,
                     float* distance, float* scores, int out_layout, void* stream) {
    if (rows < 0 || dim < 1 || nc < 1 || n_tables < 1 || n_tables > nc)
        return fail(MSST_ERR_BADARG, "msst_gauss_score (negative rows, dim or nc below 1, or n_tables outside [1, nc])");
    if (dim != 96 || nc > 128 || rows > 2147483647L) return fail(MSST_ERR_UNSUPPORTED, "msst_gauss_score (dim == 96, nc <= 128, rows <= 2^31 - 1)");
    if (int rc = feat_layout("msst_gauss_score", "layout", "rows", rows, plane, x_layout, out_layout)) return rc;
    if (!(max_d2 >= 0.f)) return fail(MSST_ERR_BADARG, "msst_gauss_score (max_d2 negative or NaN)");
    if (rows == 0) return 0;
    if (!x || !centres || !tables || !class_table || !offsets || !consts || !classes || !distance || ((uintptr_t)x & (x_layout == 0 ? 15 : 3)) ||
        ((uintptr_t)centres & 3) || ((uintptr_t)tables & 15) || ((uintptr_t)class_table & 3) || ((uintptr_t)offsets & 3) ||
        ((uintptr_t)consts & 3) || ((uintptr_t)classes & 3) || ((uintptr_t)distance & 3) || ((uintptr_t)scores & 3))
        return fail(MSST_ERR_BADARG, "msst_gauss_score (null or misaligned argument)");
    for (int c = 0; c < nc; ++c) {   // class_table is the caller's host copy
        if (class_table[c] < 0 || class_table[c] >= n_tables) return fail(MSST_ERR_BADARG, "msst_gauss_score (a table id outside [0, n_tables))");
    }
    return fail(launch_gauss_score(x, x_layout, rows, plane, centres, tables, n_tables, class_table, offsets, consts, nc, max_d2, classes,
                                   distance, scores, out_layout, (hipStream_t)stream), "msst_gauss_score");
}

long msst_gmm_scratch_floats(long rows, int k) {
    if (rows < 1 || rows > 2147483647L || k < 1 || k > 32) return 0;
    return gmm_scratch_floats(rows, k);
}

// the sizes of the three calls on Gaussian mixtures: kmax is 32, or 128 for the posterior alone
static int gmm_shape(const char* what, long rows, int dim, int k, int kmax, int cov_kind = MSST_GMM_FULL, double reg_covar = 0.0,
                     double min_count = 0.0) {
    if (rows < 1 || dim < 1 || k < 1 || (cov_kind != MSST_GMM_FULL && cov_kind != MSST_GMM_DIAG) || !(reg_covar >= 0.0) || !(min_count >= 0.0))
        return fail(MSST_ERR_BADARG, what, " (a size below 1, a cov_kind outside {0, 1}, or a negative reg_covar or min_count)");
    if (dim != 96 || k > kmax || rows > 2147483647L)
        return fail(MSST_ERR_UNSUPPORTED, what, kmax == 32 ? " (dim == 96, k <= 32, rows <= 2^31 - 1)" : " (k <= 128, rows <= 2^31 - 1)");
    return 0;
}

int msst_gmm_posterior(const float* scores, int in_layout, long rows, long plane, int k, float* lse, float* probs, int out_layout,
                       void* stream) {
    if (int rc = gmm_shape("msst_gmm_posterior", rows, 96, k, 128)) return rc;
    if (int rc = feat_layout("msst_gmm_posterior", "layout", "rows", rows, plane, in_layout, out_layout)) return rc;
    if (!scores || !lse || ((uintptr_t)scores & 3) || ((uintptr_t)lse & 3) || ((uintptr_t)probs & 3))
        return fail(MSST_ERR_BADARG, "msst_gmm_posterior (null or misaligned argument)");
    return fail(launch_gmm_posterior(scores, in_layout, rows, plane, k, lse, probs, out_layout, (hipStream_t)stream), "msst_gmm_posterior");
}

int msst_gmm_moments(const float* x, int x_layout, long rows, long plane, int dim, const float* scores, int k, const float* centres,
                     float* slab, long slab_floats, void* stream) {
    if (int rc = gmm_shape("msst_gmm_moments", rows, dim, k, 32)) return rc;
    if (int rc = feat_layout("msst_gmm_moments", "x_layout", "rows", rows, plane, x_layout)) return rc;
    if (!x || !scores || !centres || !slab || ((uintptr_t)x & (x_layout == 0 ? 15 : 3)) || ((uintptr_t)scores & 3) || ((uintptr_t)centres & 3) ||
        ((uintptr_t)slab & 3))
        return fail(MSST_ERR_BADARG, "msst_gmm_moments (null or misaligned argument)");
    if (slab_floats < gmm_scratch_floats(rows, k)) return fail(MSST_ERR_BADARG, "msst_gmm_moments (slab smaller than msst_gmm_scratch_floats)");
    return fail(launch_gmm_moments(x, x_layout, rows, plane, scores, k, centres, slab, (hipStream_t)stream), "msst_gmm_moments");
}

int msst_gmm_update(const float* slab, long slab_floats, long rows, int dim, int k, int cov_kind, double reg_covar, double min_count,
                    float* centres, float* tables, float* covs, float* logdet, float* consts, float* weights, float* raw, float* record,
                    void* stream) {
    if (int rc = gmm_shape("msst_gmm_update", rows, dim, k, 32, cov_kind, reg_covar, min_count)) return rc;
    if (!slab || !centres || !tables || !covs || !logdet || !consts || !weights || !record || ((uintptr_t)slab & 3) || ((uintptr_t)centres & 3) ||
        ((uintptr_t)tables & 3) || ((uintptr_t)covs & 3) || ((uintptr_t)logdet & 3) || ((uintptr_t)consts & 3) || ((uintptr_t)weights & 3) ||
        ((uintptr_t)raw & 3) || ((uintptr_t)record & 3))
        return fail(MSST_ERR_BADARG, "msst_gmm_update (null or misaligned argument)");
    if (slab_floats < gmm_scratch_floats(rows, k)) return fail(MSST_ERR_BADARG, "msst_gmm_update (slab smaller than msst_gmm_scratch_floats)");
    return fail(launch_gmm_update(slab, rows, k, cov_kind, reg_covar, min_count, centres, tables, covs, logdet, consts, weights, raw, record,
                                  (hipStream_t)stream), "msst_gmm_update");
}

int msst_crf_affinity(const float* feat, const int32_t* cover, int Bs, int dim, int Hs, int Ws, int radius, const float* a_tab,
                      const float* s_tab, float g, float* k, uint8_t* live, void* stream) {
    if (Bs < 1 || dim < 1 || Hs < 1 || Ws < 1) return fail(MSST_ERR_BADARG, "msst_crf_affinity (Bs, dim, Hs or Ws below 1)");
    if (dim != 96 || radius < 1 || radius > 3 || crf_tiles(Bs, Hs, Ws, 0) > 2147483647L)
        return fail(MSST_ERR_UNSUPPORTED, "msst_crf_affinity (dim == 96, 1 <= radius <= 3, at most 2^31 - 1 tiles of 8 x 16 pixels)");
    if (!(g >= 0.f) || !(g <= 3.4028234e38f)) return fail(MSST_ERR_BADARG, "msst_crf_affinity (g negative or not finite)");
    if (!feat || !a_tab || !s_tab || !k || !live || ((uintptr_t)feat & 3) || ((uintptr_t)cover & 3) || ((uintptr_t)a_tab & 3) ||
        ((uintptr_t)s_tab & 3) || ((uintptr_t)k & 3))
        return fail(MSST_ERR_BADARG, "msst_crf_affinity (null or misaligned argument)");
    return fail(launch_crf_affinity(feat, cover, Bs, Hs, Ws, radius, a_tab, s_tab, g, k, live, (hipStream_t)stream), "msst_crf_affinity");
}

int msst_crf_step(const float* scores, int unary, float unary_scale, const float* q_in, const float* k, const uint8_t* live, int Bs, int nc,
                  int Hs, int Ws, int radius, float* q_out, int32_t* classes, const int32_t* prev_classes, int32_t* changed, void* stream) {
    if (Bs < 1 || nc < 1 || Hs < 1 || Ws < 1) return fail(MSST_ERR_BADARG, "msst_crf_step (Bs, nc, Hs or Ws below 1)");
    if (nc > 128 || radius < 1 || radius > 3 || crf_tiles(Bs, Hs, Ws, 1) > 2147483647L)
        return fail(MSST_ERR_UNSUPPORTED, "msst_crf_step (nc <= 128, 1 <= radius <= 3, at most 2^31 - 1 tiles of 8 x 32 pixels)");
    if (unary < 0 || unary > 1 || !(unary_scale > 0.f) || !(unary_scale <= 3.4028234e38f))
        return fail(MSST_ERR_BADARG, "msst_crf_step (unary outside {0, 1}, or unary_scale not positive and finite)");
    if (!scores || !k || !live || !q_out || q_in == q_out || ((uintptr_t)scores & 3) || ((uintptr_t)q_in & 3) || ((uintptr_t)k & 3) ||
        ((uintptr_t)q_out & 3) || ((uintptr_t)classes & 3) || ((uintptr_t)prev_classes & 3) || ((uintptr_t)changed & 3))
        return fail(MSST_ERR_BADARG, "msst_crf_step (null or misaligned argument, or q_in == q_out)");
    if (changed && !prev_classes) return fail(MSST_ERR_BADARG, "msst_crf_step (changed without prev_classes)");
    return fail(launch_crf_step(scores, unary, unary_scale, q_in, k, live, Bs, nc, Hs, Ws, radius, q_out, classes, prev_classes, changed,
                                (hipStream_t)stream), "msst_crf_step");
}

// the sizes every SLIC call shares: C is 96 where the call has no channel count of its own
static int slic_shape(const char* what, int Bs, int dim, int Hs, int Ws, int step, int C) {
    if (Bs < 1 || dim < 1 || Hs < 1 || Ws < 1 || step < 1 || C < 1) return fail(MSST_ERR_BADARG, what, " (Bs, dim, Hs, Ws, step or C below 1)");
    if (dim != 96 || (step != 4 && step != 8 && step != 16) || C > 128 || Hs > 32768 || Ws > 32768 || slic_blocks(Bs, Hs, Ws) > (1L << 29))
        return fail(MSST_ERR_UNSUPPORTED, what, " (dim == 96, step in {4, 8, 16}, C <= 128, Hs, Ws <= 32768, blocks <= 2^29)");
    return 0;
}

long msst_slic_scratch_floats(int Bs, int Hs, int Ws, int step, int C) {
    if (Bs < 1 || Hs < 1 || Ws < 1 || C < 1 || C > 128 || (step != 4 && step != 8 && step != 16) || Hs > 32768 || Ws > 32768 ||
        slic_blocks(Bs, Hs, Ws) > (1L << 29))
        return 0;
    return slic_scratch_floats(Bs, Hs, Ws, C);
}

int msst_slic_assign(const float* feat, const int32_t* cover, int Bs, int dim, int Hs, int Ws, int step, float hl, const float* centroids,
                     const float* offsets, const float* bias, const int32_t* counts, int64_t* labels, const int64_t* prev_labels, int32_t* moved,
                     float* best, float* slab, long slab_floats, void* stream) {
    if (int rc = slic_shape("msst_slic_assign", Bs, dim, Hs, Ws, step, 96)) return rc;
    if (!(hl >= 0.f) || !(hl <= 3.4028234e38f)) return fail(MSST_ERR_BADARG, "msst_slic_assign (hl negative or not finite)");
    if (!feat || !labels || ((uintptr_t)feat & 3) || ((uintptr_t)cover & 3) || ((uintptr_t)centroids & 3) || ((uintptr_t)offsets & 3) ||
        ((uintptr_t)bias & 3) || ((uintptr_t)counts & 3) || ((uintptr_t)labels & 7) || ((uintptr_t)prev_labels & 7) || ((uintptr_t)moved & 3) ||
        ((uintptr_t)best & 3) || ((uintptr_t)slab & 3))
        return fail(MSST_ERR_BADARG, "msst_slic_assign (null or misaligned argument)");
    if (centroids && (!offsets || !bias || !counts)) return fail(MSST_ERR_BADARG, "msst_slic_assign (centroids without offsets, bias and counts)");
    if (moved && !prev_labels) return fail(MSST_ERR_BADARG, "msst_slic_assign (moved without prev_labels)");
    if (slab && slab_floats < slic_scratch_floats(Bs, Hs, Ws, MSST_SLIC_FIT_CHANNELS))
        return fail(MSST_ERR_BADARG, "msst_slic_assign (slab smaller than msst_slic_scratch_floats(.., MSST_SLIC_FIT_CHANNELS))");
    return fail(launch_slic_assign(feat, cover, Bs, Hs, Ws, step, hl, centroids, offsets, bias, counts, labels, prev_labels, moved, best, slab,
                                   (hipStream_t)stream), "msst_slic_assign");
}

int msst_slic_update(const float* slab, long slab_floats, int Bs, int dim, int Hs, int Ws, int step, float* centroids, float* offsets,
                     float* bias, int32_t* counts, int32_t* empty, void* stream) {
    if (int rc = slic_shape("msst_slic_update", Bs, dim, Hs, Ws, step, 96)) return rc;
    if (!slab || !centroids || !offsets || !bias || !counts || ((uintptr_t)slab & 3) || ((uintptr_t)centroids & 3) || ((uintptr_t)offsets & 3) ||
        ((uintptr_t)bias & 3) || ((uintptr_t)counts & 3) || ((uintptr_t)empty & 3))
        return fail(MSST_ERR_BADARG, "msst_slic_update (null or misaligned argument)");
    if (slab_floats < slic_scratch_floats(Bs, Hs, Ws, MSST_SLIC_FIT_CHANNELS))
        return fail(MSST_ERR_BADARG, "msst_slic_update (slab smaller than msst_slic_scratch_floats(.., MSST_SLIC_FIT_CHANNELS))");
    return fail(launch_slic_update(slab, Bs, Hs, Ws, step, centroids, offsets, bias, counts, empty, (hipStream_t)stream), "msst_slic_update");
}

int msst_slic_pool(const float* map, const int64_t* labels, int Bs, int C, int Hs, int Ws, int step, float* slab, long slab_floats,
                   void* stream) {
    if (int rc = slic_shape("msst_slic_pool", Bs, 96, Hs, Ws, step, C)) return rc;
    if (!map || !labels || !slab || ((uintptr_t)map & 3) || ((uintptr_t)labels & 7) || ((uintptr_t)slab & 3))
        return fail(MSST_ERR_BADARG, "msst_slic_pool (null or misaligned argument)");
    if (slab_floats < slic_scratch_floats(Bs, Hs, Ws, C)) return fail(MSST_ERR_BADARG, "msst_slic_pool (slab smaller than msst_slic_scratch_floats)");
    return fail(launch_slic_pool(map, labels, Bs, C, Hs, Ws, step, slab, (hipStream_t)stream), "msst_slic_pool");
}

int msst_slic_pool_finish(const float* slab, long slab_floats, int Bs, int C, int Hs, int Ws, int step, float* table, int64_t* region_classes,
                          void* stream) {
    if (int rc = slic_shape("msst_slic_pool_finish", Bs, 96, Hs, Ws, step, C)) return rc;
    if (!slab || !table || ((uintptr_t)slab & 3) || ((uintptr_t)table & 3) || ((uintptr_t)region_classes & 7))
        return fail(MSST_ERR_BADARG, "msst_slic_pool_finish (null or misaligned argument)");
    if (slab_floats < slic_scratch_floats(Bs, Hs, Ws, C))
        return fail(MSST_ERR_BADARG, "msst_slic_pool_finish (slab smaller than msst_slic_scratch_floats)");
    return fail(launch_slic_pool_finish(slab, Bs, C, Hs, Ws, step, table, region_classes, (hipStream_t)stream), "msst_slic_pool_finish");
}

int msst_slic_broadcast(const int64_t* labels, const int64_t* region_classes, int Bs, int Hs, int Ws, int step, int64_t* classes, void* stream) {
    if (int rc = slic_shape("msst_slic_broadcast", Bs, 96, Hs, Ws, step, 96)) return rc;
    if (!labels || !region_classes || !classes || ((uintptr_t)labels & 7) || ((uintptr_t)region_classes & 7) || ((uintptr_t)classes & 7))
        return fail(MSST_ERR_BADARG, "msst_slic_broadcast (null or misaligned argument)");
    return fail(launch_slic_broadcast(labels, region_classes, Bs, Hs, Ws, step, classes, (hipStream_t)stream), "msst_slic_broadcast");
}

// the sizes both region calls share
static int regions_shape(const char* what, int Bs, int Hs, int Ws, int connectivity) {
    if (Bs < 1 || Hs < 1 || Ws < 1) return fail(MSST_ERR_BADARG, what, " (Bs, Hs or Ws below 1)");
    if (Hs > 32768 || Ws > 32768 || (long)Hs * Ws >= (1L << 31) || regions_tiles(Bs, Hs, Ws) > 2147483647L)
        return fail(MSST_ERR_UNSUPPORTED, what, " (Hs, Ws <= 32768, Hs * Ws < 2^31, at most 2^31 - 1 tiles of 16 x 16 pixels)");
    if (connectivity != 4 && connectivity != 8) return fail(MSST_ERR_BADARG, what, " (connectivity outside {4, 8})");
    return 0;
}

long msst_regions_scratch_bytes(int Bs, int Hs, int Ws) {
    if (Bs < 1 || Hs < 1 || Ws < 1 || Hs > 32768 || Ws > 32768 || (long)Hs * Ws >= (1L << 31) || regions_tiles(Bs, Hs, Ws) > 2147483647L) return 0;
    return regions_scratch_bytes(Bs, Hs, Ws);
}

int msst_regions_label(const int64_t* values, int Bs, int Hs, int Ws, int connectivity, int64_t* labels, int32_t* sizes, int32_t* count,
                       void* scratch, long scratch_bytes, void* stream) {
    if (int rc = regions_shape("msst_regions_label", Bs, Hs, Ws, connectivity)) return rc;
    if (!values || !labels || !sizes || !count || !scratch || ((uintptr_t)values & 7) || ((uintptr_t)labels & 7) || ((uintptr_t)sizes & 3) ||
        ((uintptr_t)count & 3) || ((uintptr_t)scratch & 15))
        return fail(MSST_ERR_BADARG, "msst_regions_label (null or misaligned argument)");
    if (scratch_bytes < regions_scratch_bytes(Bs, Hs, Ws))
        return fail(MSST_ERR_BADARG, "msst_regions_label (scratch smaller than msst_regions_scratch_bytes)");
    return fail(launch_regions_label(values, Bs, Hs, Ws, connectivity, labels, sizes, count, scratch, (hipStream_t)stream), "msst_regions_label");
}

int msst_regions_merge(const int64_t* values, const int64_t* labels, const int32_t* sizes, int Bs, int Hs, int Ws, int connectivity, int mode,
                       int min_size, int step, int64_t* values_out, int32_t* history, void* scratch, long scratch_bytes, void* stream) {
    if (Bs >= 1 && Hs >= 1 && Ws >= 1 && ((mode == 0 && min_size < 1) || (mode == 1 && step < 1)))
        return fail(MSST_ERR_BADARG, "msst_regions_merge (min_size or step below 1)");
    if (int rc = regions_shape("msst_regions_merge", Bs, Hs, Ws, connectivity)) return rc;
    if (mode != 0 && mode != 1) return fail(MSST_ERR_BADARG, "msst_regions_merge (mode outside {0, 1})");
    if (!values || !labels || !sizes || !values_out || !history || !scratch || ((uintptr_t)values & 7) || ((uintptr_t)labels & 7) ||
        ((uintptr_t)sizes & 3) || ((uintptr_t)values_out & 7) || ((uintptr_t)history & 3) || ((uintptr_t)scratch & 15))
        return fail(MSST_ERR_BADARG, "msst_regions_merge (null or misaligned argument)");
    if (values_out == values) return fail(MSST_ERR_BADARG, "msst_regions_merge (values_out == values: the round reads its input throughout)");
    if (scratch_bytes < regions_scratch_bytes(Bs, Hs, Ws))
        return fail(MSST_ERR_BADARG, "msst_regions_merge (scratch smaller than msst_regions_scratch_bytes)");
    return fail(launch_regions_merge(values, labels, sizes, Bs, Hs, Ws, connectivity, mode, min_size, step, values_out, history, scratch,
                                     (hipStream_t)stream), "msst_regions_merge");
}

int msst_scene_embed_assemble(const float* win_feat, long win0, int nwin, float* feat, int32_t* cover, int Bs, int D, int Hs, int Ws,
                              int window, int stride, int finalize, int l2norm, void* stream) {
    if (Bs < 1 || D < 1 || Hs < 1 || Ws < 1 || window < 1 || stride < 1 || nwin < 0 || win0 < 0)
        return fail(MSST_ERR_BADARG, "msst_scene_embed_assemble");
    if (stride > window || window > Hs || window > Ws || window * window > 64 || D > 128)
        return fail(MSST_ERR_UNSUPPORTED, "msst_scene_embed_assemble (1 <= stride <= window <= Hs, Ws; window * window <= 64, D <= 128)");
    if ((nwin > 0 && !win_feat) || !feat || (finalize && !cover)) return fail(MSST_ERR_BADARG, "msst_scene_embed_assemble (null argument)");
    int nr = 0, nq = 0;
    scene_grid(Bs, Hs, Ws, window, stride, &nr, &nq);
    const long wps = (long)nr * nq;
    if (win0 + nwin > (long)Bs * wps) return fail(MSST_ERR_BADARG, "msst_scene_embed_assemble (windows out of range)");
    // both launches' grids fit (so nothing is refused after the first one is enqueued)
    if (((long)Bs * Hs * Ws + 255) / 256 > 0x7fffffffL) return fail(MSST_ERR_UNSUPPORTED, "msst_scene_embed_assemble (scene batch too large)");
    SceneEmbedArgs a;
    fill_grid(a, win0, nwin, Bs, Hs, Ws, window, stride, nr, nq);
    a.win_feat = win_feat; a.feat = feat; a.cover = cover; a.D = D; a.l2norm = l2norm != 0;
    hipStream_t st = (hipStream_t)stream;
    int rc = launch_scene_fold(a, win_feat, feat, D, 16, scene_call_rows(a, wps), st);
    if (!rc && finalize) rc = launch_scene_embed_finalize(a, st);
    return fail(rc, "msst_scene_embed_assemble");
}

long msst_block_lse_floats(int mode, int B, int S, int N, int heads) {
    if (B < 1 || S < 1 || N < 1 || heads < 1 || N > 64 || S > 64) return 0;
    return (long)ntiles_of(make_tilemap(mode, B, S, N)) * heads * 64 + (long)B * S * N;   // [tiles][heads][64] lse | [tokens] rstd of LN1
}

long msst_block_tiles(int mode, int B, int S, int N) {
    if (B < 1 || S < 1 || N < 1 || N > 64 || S > 64) return 0;
    return (long)ntiles_of(make_tilemap(mode, B, S, N));
}

int msst_block_fwd(const MsstBlockWeights* w, const float* x, float* y, float* x1, int mode, int B, int S,
                   int N, int heads, int prec, int max_grid, float dropout_p, uint32_t seed, int layer,
                   void* xn_out, float* lse_out, int* saved, void* stream) {
    if (int rc = block_shape(mode, B, S, N, heads)) return fail(rc, "msst_block_fwd (B, S, N, heads < 1, mode not 0 / 1, or sequence length > 64)");
    if (!bw_ok(w) || !x || !y || x == y) return fail(MSST_ERR_BADARG, "msst_block_fwd (null argument, or MsstBlockWeights of another header revision)");
    const int dbg = (prec >> 8) & 0xffff;   // MSST_KERNEL_* selection flags ride in the upper bits of `prec`
    prec &= 0xff;
    BlockArgs a;
    a.w = to_bw(w);
    a.x = x; a.y = y; a.x1 = x1;
    a.tm = make_tilemap(mode, B, S, N);
    a.ntiles = ntiles_of(a.tm);
    a.max_grid = max_grid > 0 ? max_grid : a.ntiles;
    a.H = heads;
    a.scale = 0.125f;  // dim_head ** -0.5, dim_head = 64 (vit_spatial_spectral.py:54)
    a.dbg = dbg & ~8;
    a.stamps = nullptr;
#ifdef MSST_STAMPS
    a.stamps = g_stamps;
    if (g_stamps) a.dbg = dbg;
#elif defined(MSST_LAB)
    a.stamps = g_stamps;
#endif
    // MSST_X1_BF16: only the role-split forward (bf16, 8 heads, no kernel selection flags) writes bf16 x1 rows
    a.x1_bf16 = (dbg & 1024) ? 1 : 0;
    if (a.x1_bf16 && !(prec == MSST_PREC_BF16 && heads == 8 && !(dbg & (16 | 64))))
        return fail(MSST_ERR_UNSUPPORTED, "msst_block_fwd (MSST_X1_BF16 needs the role-split bf16 forward: 8 heads, no MSST_KERNEL_* flags)");
    // MSST_FWD_HALF: fp16 operands -- the role-split forward only, and the caller must have prepared the half copies of its four matrices
    a.half = (dbg & 4096) ? 1 : 0;
    if (a.half) {
        if (!(prec == MSST_PREC_BF16 && heads == 8 && !(dbg & (16 | 64))))
            return fail(MSST_ERR_UNSUPPORTED, "msst_block_fwd (MSST_FWD_HALF needs the role-split bf16 forward: 8 heads, no MSST_KERNEL_* flags)");
        if (!w->wqkv_h || !w->wout_h || !w->w1_h || !w->w2_h) return fail(MSST_ERR_BADARG, "msst_block_fwd (MSST_FWD_HALF without the half weight copies)");
        a.w.wqkv = w->wqkv_h; a.w.wout = w->wout_h; a.w.w1 = w->w1_h; a.w.w2 = w->w2_h;
    }
    a.drop = make_drop(dropout_p, seed, layer);
    a.xn_out = (xn_out && block_fwd_writes_xn(a, prec)) ? xn_out : nullptr;
    a.lse_out = (lse_out && block_fwd_writes_lse(a, prec)) ? lse_out : nullptr;
    if (saved) *saved = (a.xn_out ? MSST_SAVED_XN : 0) | (a.lse_out ? (MSST_SAVED_LSE | MSST_SAVED_RSTD) : 0);
    return fail(launch_block_fwd(a, prec, (hipStream_t)stream), "msst_block_fwd");
}

int msst_block_fwd_stack(const MsstBlockWeights* const* w, int nblk, const float* x0, float* const* y, float* const* x1,
                         void* const* xn_out, float* const* lse_out, int mode, int B, int S, int N, int heads, int prec, int max_grid,
                         float dropout_p, uint32_t seed, int layer0, int* saved, void* stream) {
    if (int rc = block_shape(mode, B, S, N, heads)) return fail(rc, "msst_block_fwd_stack (B, S, N, heads < 1, mode not 0 / 1, or sequence length > 64)");
    if (!w || !x0 || !y || nblk < 1) return fail(MSST_ERR_BADARG, "msst_block_fwd_stack");
    if (nblk > MSST_MAX_STACK) return fail(MSST_ERR_UNSUPPORTED, "msst_block_fwd_stack (more than 16 blocks)");
    const int dbg = (prec >> 8) & 0xffff;
    prec &= 0xff;
    // the role-split bf16 forward only: 8 heads, no kernel selection flags (MSST_X1_BF16 is the one flag it takes)
    if (prec != MSST_PREC_BF16 || heads != 8 || (dbg & ~(1024 | 4096))) return fail(MSST_ERR_UNSUPPORTED, "msst_block_fwd_stack (bf16, 8 heads, no MSST_KERNEL_* flags)");
    const bool half = (dbg & 4096) != 0;
    for (int j = 0; j < nblk; ++j) {
        if (!bw_ok(w[j])) return fail(MSST_ERR_BADARG, "msst_block_fwd_stack (null block, or MsstBlockWeights of another header revision)");
        if (half && (!w[j]->wqkv_h || !w[j]->wout_h || !w[j]->w1_h || !w[j]->w2_h)) return fail(MSST_ERR_BADARG, "msst_block_fwd_stack (MSST_FWD_HALF without the half weight copies)");
    }
    StackArgs sa;
    BlockArgs& a = sa.base;
    memset(&a.w, 0, sizeof(a.w));
    a.x = x0; a.y = nullptr; a.x1 = nullptr; a.xn_out = nullptr; a.lse_out = nullptr;
    a.tm = make_tilemap(mode, B, S, N);
    a.ntiles = ntiles_of(a.tm);
    a.max_grid = max_grid > 0 ? max_grid : a.ntiles;
    a.H = heads;
    a.scale = 0.125f;
    a.dbg = 0;
    a.stamps = nullptr;
    a.x1_bf16 = (dbg & 1024) ? 1 : 0;
    a.half = half ? 1 : 0;
    a.drop = make_drop(dropout_p, seed, layer0);
    if (lse_out && !block_fwd_writes_lse(a, prec)) lse_out = nullptr;   // same rule as msst_block_fwd: a statistics buffer past the 31-bit descriptor range is declined, not clipped
    sa.nblk = nblk;
    // the kernel addresses block j's operands as block 0's + j x a byte stride: every array of the call must be affine in the block
    // index (maskedsst_amd lays its weight copies, parameters and activations out that way); anything else is refused
    auto blk_of = [&](int j, const float* xin) {
        StackBlk sb;
        sb.wqkv = half ? w[j]->wqkv_h : w[j]->wqkv; sb.wout = half ? w[j]->wout_h : w[j]->wout;
        sb.w1 = half ? w[j]->w1_h : w[j]->w1; sb.w2 = half ? w[j]->w2_h : w[j]->w2;
        sb.ln1_g = w[j]->ln1_g; sb.ln1_b = w[j]->ln1_b; sb.bo = w[j]->bo; sb.ln2_g = w[j]->ln2_g; sb.ln2_b = w[j]->ln2_b; sb.b1 = w[j]->b1; sb.b2 = w[j]->b2;
        sb.x = xin; sb.y = y[j]; sb.x1 = x1 ? x1[j] : nullptr; sb.xn_out = xn_out ? xn_out[j] : nullptr; sb.lse_out = lse_out ? lse_out[j] : nullptr;
        sb.layer = layer0 + j; sb.pad_ = 0;
        return sb;
    };
    for (int j = 0; j < nblk; ++j)
        if (!bw_ok(w[j]) || !y[j] || y[j] == (j ? y[j - 1] : x0))
            return fail(MSST_ERR_BADARG, "msst_block_fwd_stack (null argument, or MsstBlockWeights of another header revision)");
    sa.b0 = blk_of(0, x0);
    memset(&sa.st, 0, sizeof(sa.st));
    bool affine = true;
    if (nblk > 1) {
        const StackBlk b1 = blk_of(1, y[0]);
        auto dist = [&](const void* p1, const void* p0, int& out) {
            const long d = (const char*)p1 - (const char*)p0;
            if (d > 0x7fffffffL || d < -0x7fffffffL) affine = false;
            out = (int)d;
        };
        dist(b1.wqkv, sa.b0.wqkv, sa.st.wqkv); dist(b1.wout, sa.b0.wout, sa.st.wout); dist(b1.w1, sa.b0.w1, sa.st.w1); dist(b1.w2, sa.b0.w2, sa.st.w2);
        dist(b1.ln1_g, sa.b0.ln1_g, sa.st.ln1_g); dist(b1.ln1_b, sa.b0.ln1_b, sa.st.ln1_b); dist(b1.bo, sa.b0.bo, sa.st.bo);
        dist(b1.ln2_g, sa.b0.ln2_g, sa.st.ln2_g); dist(b1.ln2_b, sa.b0.ln2_b, sa.st.ln2_b); dist(b1.b1, sa.b0.b1, sa.st.b1); dist(b1.b2, sa.b0.b2, sa.st.b2);
        dist(b1.y, sa.b0.y, sa.st.y); dist(b1.x1, sa.b0.x1, sa.st.x1); dist(b1.xn_out, sa.b0.xn_out, sa.st.xn_out); dist(b1.lse_out, sa.b0.lse_out, sa.st.lse_out);
        // block j > 0 reads what block j - 1 wrote: x_j = y_(j-1) = y_0 + (j - 1) stride_y -- affine from block 1 on; block 0 reads x0.  The
        // kernel takes x_j = x_base + j stride_y with x_base = y_0 - stride_y for j >= 1 and x0 for j = 0: keep both
        sa.st.x = sa.st.y;
        const float* xin = y[0];
        for (int j = 1; j < nblk && affine; ++j) {
            const StackBlk bj = blk_of(j, xin);
            auto same = [&](const void* pj, const void* p0, int stride) { return !p0 ? !pj : (const char*)pj == (const char*)p0 + (long)j * stride; };
            affine = same(bj.wqkv, sa.b0.wqkv, sa.st.wqkv) && same(bj.wout, sa.b0.wout, sa.st.wout) && same(bj.w1, sa.b0.w1, sa.st.w1) &&
                     same(bj.w2, sa.b0.w2, sa.st.w2) && same(bj.ln1_g, sa.b0.ln1_g, sa.st.ln1_g) && same(bj.ln1_b, sa.b0.ln1_b, sa.st.ln1_b) &&
                     same(bj.bo, sa.b0.bo, sa.st.bo) && same(bj.ln2_g, sa.b0.ln2_g, sa.st.ln2_g) && same(bj.ln2_b, sa.b0.ln2_b, sa.st.ln2_b) &&
                     same(bj.b1, sa.b0.b1, sa.st.b1) && same(bj.b2, sa.b0.b2, sa.st.b2) && same(bj.y, sa.b0.y, sa.st.y) &&
                     same(bj.x1, sa.b0.x1, sa.st.x1) && same(bj.xn_out, sa.b0.xn_out, sa.st.xn_out) && same(bj.lse_out, sa.b0.lse_out, sa.st.lse_out);
            xin = y[j];
        }
    }
    if (!affine) return fail(MSST_ERR_UNSUPPORTED, "msst_block_fwd_stack (per-block operands not a constant stride apart)");
    sa.x_rest = nblk > 1 ? reinterpret_cast<const float*>(reinterpret_cast<const char*>(y[0]) - (long)sa.st.y) : x0;   // x of block j >= 1 = x_rest + j stride_y
    if (saved) *saved = (xn_out ? MSST_SAVED_XN : 0) | (lse_out ? (MSST_SAVED_LSE | MSST_SAVED_RSTD) : 0);
    if (a.ntiles < 1) return 0;
    int ncu = 256, dev = 0;
    hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu < 1) ncu = 256;
    int grid = a.max_grid < a.ntiles ? a.max_grid : a.ntiles;
    if (grid > ncu) grid = ncu;
    return fail(launch_block_fwd_rs_stack(sa, grid, (hipStream_t)stream), "msst_block_fwd_stack");
}

int msst_head_fwd(const float* y, const float* img, const int32_t* idx, const float* w_pix,
                  const float* b_pix, int per_block, float* dpred, float* pred, float* partial,
                  float* loss, int B, int S, int N, int P, int K, void* stream) {
    HeadArgs a{};   // a batch of cubes: no window tables
    a.y = y; a.src.base = img; a.idx = idx; a.w_pix = w_pix; a.b_pix = b_pix; a.dpred = dpred; a.pred = pred;
    a.partial = partial; a.B = B; a.S = S; a.N = N; a.T = S * N; a.P = P; a.K = K; a.per_block = per_block;
    return fail(launch_head_fwd(a, WIN_BATCH, loss, (hipStream_t)stream), "msst_head_fwd");
}

// msst_head_at_fwd and msst_head_at_fwd_orient (oriented: the orientation table is required too)
static int head_at_fwd(const char* what, bool oriented, const float* y, const float* scene, const int32_t* origins, const uint8_t* orient,
                       const int32_t* idx, const float* w_pix, const float* b_pix, int per_block, float* dpred, float* pred, float* partial,
                       float* loss, int Bs, int Hs, int Ws, int window, int nwin, int S, int P, int K, void* stream) {
    if (Bs < 1 || Hs < 1 || Ws < 1 || window < 1 || S < 1 || P < 1 || K < 1 || nwin < 1) return fail(MSST_ERR_BADARG, what);
    if (window > Hs || window > Ws || window > 8 || P > 16 || nwin > 65535)   // 65535: one workgroup row per window (grid y)
        return fail(MSST_ERR_UNSUPPORTED, what, " (window <= Hs, Ws, window * window <= 64, P <= 16, nwin <= 65535)");
    if (!y || !scene || !origins || (oriented && !orient) || !idx || !w_pix || !b_pix || !dpred || !partial || !loss || K > S * window * window)
        return fail(MSST_ERR_BADARG, what);
    HeadArgs a{};
    a.y = y; a.src.base = scene; a.idx = idx; a.w_pix = w_pix; a.b_pix = b_pix; a.dpred = dpred; a.pred = pred;
    a.partial = partial; a.B = nwin; a.S = S; a.N = window * window; a.T = S * a.N; a.P = P; a.K = K; a.per_block = per_block;
    const WinSrc w{Bs, Hs, Ws, window, window, 0, nwin, true, origins, 1, 1, oriented, orient};
    fill_src(a.src, w);
    return fail(launch_head_fwd(a, w.kind(), loss, (hipStream_t)stream), what);
}

int msst_head_at_fwd(const float* y, const float* scene, const int32_t* origins, const int32_t* idx, const float* w_pix,
                     const float* b_pix, int per_block, float* dpred, float* pred, float* partial, float* loss, int Bs, int Hs, int Ws,
                     int window, int nwin, int S, int P, int K, void* stream) {
    return head_at_fwd("msst_head_at_fwd", false, y, scene, origins, nullptr, idx, w_pix, b_pix, per_block, dpred, pred, partial, loss, Bs,
                       Hs, Ws, window, nwin, S, P, K, stream);
}

int msst_head_at_fwd_orient(const float* y, const float* scene, const int32_t* origins, const uint8_t* orient, const int32_t* idx,
                            const float* w_pix, const float* b_pix, int per_block, float* dpred, float* pred, float* partial, float* loss,
                            int Bs, int Hs, int Ws, int window, int nwin, int S, int P, int K, void* stream) {
    return head_at_fwd("msst_head_at_fwd_orient", true, y, scene, origins, orient, idx, w_pix, b_pix, per_block, dpred, pred, partial, loss,
                       Bs, Hs, Ws, window, nwin, S, P, K, stream);
}

int msst_head_bwd(const float* y, const float* dpred, const int32_t* csr_ptr, const int32_t* csr_pos,
                  const float* w_pix, int per_block, float gscale, const float* gout, float* dy, float* slab,
                  int nchunk, float* dw_pix, float* db_pix, int B, int S, int N, int P, int K, void* stream) {
    if (nchunk < 1) return fail(MSST_ERR_BADARG, "msst_head_bwd");
    hipStream_t st = (hipStream_t)stream;
    HeadBwdArgs a;
    a.y = y; a.dpred = dpred; a.csr_ptr = csr_ptr; a.csr_pos = csr_pos; a.w_pix = w_pix; a.dy = dy; a.slab = slab;
    a.gscale = gscale; a.gout = gout; a.B = B; a.S = S; a.N = N; a.T = S * N; a.P = P; a.K = K; a.per_block = per_block;
    int rc = launch_head_bwd(a, nchunk, st);
    if (rc) return fail(rc, "msst_head_bwd");
    const long ss = (long)P * 96 + P;
    RSegBuilder rb;
    bool ok = true;
    if (per_block) {
        for (int c = 0; c < S && ok; ++c) {
            ok = rb.add(slab + (long)c * nchunk * ss, ss, nchunk, dw_pix + (long)c * P * 96, P * 96);
            ok = ok && rb.add(slab + (long)c * nchunk * ss + P * 96, ss, nchunk, db_pix + (long)c * P, P);
            if (rb.r.nseg > MSST_MAX_RSEG - 2 && c + 1 < S) {   // table full (S > 36): flush and start a new one
                rc = launch_reduce_segs(rb.r, st);
                if (rc) return fail(rc, "msst_head_bwd(reduce)");
                rb = RSegBuilder();
            }
        }
    } else {
        ok = rb.add(slab, ss, S * nchunk, dw_pix, P * 96);
        ok = ok && rb.add(slab + P * 96, ss, S * nchunk, db_pix, P);
    }
    if (!ok) return fail(MSST_ERR_UNSUPPORTED, "msst_head_bwd(reduce table)");
    rc = launch_reduce_segs(rb.r, st);
    return fail(rc, "msst_head_bwd(reduce)");
}

// where the parts of one block backward keep their partial-gradient slabs inside the caller's `slab` workspace
struct SlabLayout {
    int grid, grid_mlp, nc;
    float *mlp, *attn, *ln1, *mlp_prev;
};
static SlabLayout slab_layout(float* slab, long ntok, int grid_rows, int nchunk, int ntiles_attn, int heads, int prec) {
    SlabLayout l;
    const int ntiles_rows = (int)((ntok + 63) / 64);
    l.grid = grid_rows < ntiles_rows ? grid_rows : ntiles_rows;   // LN1 backward: HBM bound at one workgroup per CU
    // the bf16 MLP backward is latency bound and fits two workgroups per CU: twice the persistent grid (and slabs)
    const int gmlp2 = (prec == MSST_PREC_BF16 && PBF16::WAVES_BWD_MLP == 2) ? 2 * grid_rows : grid_rows;
    l.grid_mlp = gmlp2 < ntiles_rows ? gmlp2 : ntiles_rows;
    l.nc = nchunk < ntiles_attn ? nchunk : ntiles_attn;
    l.mlp = slab;
    l.attn = l.mlp + (long)l.grid_mlp * MSST_MLP_SLAB_N;
    l.ln1 = l.attn + (long)l.nc * heads * MSST_ATTN_SLAB_N;
    l.mlp_prev = l.ln1 + (long)l.grid * MSST_LN1_SLAB;
    return l;
}
// the reduction table of one block backward (or, ny_* > 1, of a run of chained ones: see msst_block_bwd_reduce).
// g_mlp: gradients the standalone MLP half wrote slabs for (null: it did not run); g_prev: the same for the fused launch's MLP half
static int reduce_block_slabs(const SlabLayout& lay, int heads, const MsstBlockGrads* g, const MsstBlockGrads* g_mlp, int ny_mlp,
                              const MsstBlockGrads* g_prev, int ny_prev, int ny, long src_ystride, long dst_ystride, hipStream_t st) {
    RSegBuilder rb;
    auto fresh = [&]() { rb = RSegBuilder(); rb.r.src_ystride = src_ystride; rb.r.dst_ystride = dst_ystride; };
    fresh();
    const long ms = MSST_MLP_SLAB_N;
    bool ok = true;
    auto add_mlp = [&](const float* sm_, int nslab, const MsstBlockGrads* gg, int nyy) {
        ok = ok && rb.add(sm_, ms, nslab, gg->w1, 6144, 0, 0, nyy);
        ok = ok && rb.add(sm_ + 6144, ms, nslab, gg->w2, 6144, 0, 0, nyy);
        ok = ok && rb.add(sm_ + 12288, ms, nslab, gg->b1, 64, 0, 0, nyy);
        ok = ok && rb.add(sm_ + 12288 + 64, ms, nslab, gg->b2, 96, 0, 0, nyy);
        ok = ok && rb.add(sm_ + 12288 + 160, ms, nslab, gg->ln2_g, 96, 0, 0, nyy);
        ok = ok && rb.add(sm_ + 12288 + 256, ms, nslab, gg->ln2_b, 96, 0, 0, nyy);
    };
    if (g_mlp) add_mlp(lay.mlp, lay.grid_mlp, g_mlp, ny_mlp);
    if (g_prev) add_mlp(lay.mlp_prev, lay.grid, g_prev, ny_prev);
    if (g) {
        ok = ok && rb.add(lay.ln1, 288, lay.grid, g->ln1_g, 96, 0, 0, ny);
        ok = ok && rb.add(lay.ln1 + 96, 288, lay.grid, g->ln1_b, 96, 0, 0, ny);
        ok = ok && rb.add(lay.ln1 + 192, 288, lay.grid, g->bo, 96, 0, 0, ny);
        const long as = (long)heads * MSST_ATTN_SLAB_N;
        const int inner = heads * 64;
        for (int h = 0; h < heads && ok; ++h) {
            const float* sh = lay.attn + (long)h * MSST_ATTN_SLAB_N;
            for (int which = 0; which < 3 && ok; ++which)
                ok = rb.add(sh + which * 6144, as, lay.nc, g->wqkv + ((long)(which * heads + h) * 64) * 96, 6144, 0, 0, ny);
            ok = ok && rb.add(sh + 3 * 6144, as, lay.nc, g->wout + h * 64, 6144, 64, inner, ny);
            if (rb.r.nseg > MSST_MAX_RSEG - 4 && h + 1 < heads) {   // flush when the table is nearly full
                int rc = launch_reduce_segs(rb.r, st);
                if (rc) return rc;
                fresh();
            }
        }
    }
    if (!ok) return MSST_ERR_UNSUPPORTED;
    return launch_reduce_segs(rb.r, st);
}

// chain == 0: the three halves of ONE block (MLP half -> attention half -> LN1 backward), msst_block_bwd.
// chain != 0: msst_block_bwd_chain (see include/msst.h): [MLP half of block i when `first`] -> attention half of block i ->
//             LN1 backward of block i fused with the MLP half of block i - 1 (w_prev), or alone (block 0).
static int block_bwd_impl(const MsstBlockWeights* w, const MsstBlockGrads* g, const MsstBlockWeights* w_prev,
                          const MsstBlockGrads* g_prev, const float* x, const float* x1, const float* x1_prev,
                          const float* dy, float* dx, float* dx1, void* dxn_part, float* slab, int grid_rows,
                          int nchunk, int mode, int B, int S, int N, int heads, int prec, float dropout_p,
                          uint32_t seed, int layer, const void* xn_saved, const float* lse_saved, void* dab_ws, int chain, int first,
                          int32_t* tile_queue, hipStream_t st) {
    if (int rc = block_shape(mode, B, S, N, heads)) return fail(rc, "msst_block_bwd (B, S, N, heads < 1, mode not 0 / 1, or sequence length > 64)");
    if (!bw_ok(w) || (w_prev && !bw_ok(w_prev)) || !g || grid_rows < 1 || nchunk < 1)
        return fail(MSST_ERR_BADARG, "msst_block_bwd (null argument, or MsstBlockWeights of another header revision)");
    const int dbg = (prec >> 8) & 0xffff;   // MSST_KERNEL_* selection flags ride in the upper bits of `prec`
    prec &= 0xff;
    const long ntok = (long)B * S * N;
    const BlockWeights bw = to_bw(w);
    const Drop drop = make_drop(dropout_p, seed, layer);
    AttnBwdArgs aa;
    aa.tm = make_tilemap(mode, B, S, N);
    aa.ntiles = ntiles_of(aa.tm);
    const SlabLayout lay = slab_layout(slab, ntok, grid_rows, nchunk, aa.ntiles, heads, prec);
    const int grid = lay.grid, grid_mlp = lay.grid_mlp, nc = lay.nc;
    float* slab_mlp = lay.mlp;
    float* slab_attn = lay.attn;
    float* slab_ln1 = lay.ln1;
    float* slab_mlp_prev = lay.mlp_prev;   // chain: the fused launch's MLP slabs (block i - 1), one per workgroup
    // saved LN1 rows + pre-dropped bf16 da rows: both or neither, and only for the tuned bf16 attention kernel
    const bool fast_rows = xn_saved && dab_ws && prec == MSST_PREC_BF16 && !(dbg & 16);
    if (chain && (!fast_rows || (w_prev && (!g_prev || !x1_prev)) || (first && !dy) || (!w_prev && !dx)))
        return fail(MSST_ERR_BADARG, "msst_block_bwd_chain (bf16 with saved LN1 rows and the dab workspace only)");
    const bool run_mlp = !chain || first;
    // MSST_X1_BF16: the saved mid-residual rows (x1, x1_prev) are bf16 -- the bf16 MLP-half kernels read either kind
    const int x1b = (dbg & 1024) ? 1 : 0;
    if (x1b && prec != MSST_PREC_BF16)
        return fail(MSST_ERR_UNSUPPORTED, "msst_block_bwd (MSST_X1_BF16 needs the bf16 kernels)");
    // dynamic tile queues (data parallel): counters [0, heads / 2) for the two-head attention backward, [32] for the fused launch
    if (tile_queue) {
        hipError_t e = hipMemsetAsync(tile_queue, 0, MSST_TILE_QUEUE_WORDS * sizeof(int32_t), st);
        if (e != hipSuccess) return fail((int)e, "msst_block_bwd_chain(tile queue)");
    }
    // 1. MLP half: dy -> dx1
    if (run_mlp) {
        MlpBwdArgs a;
        a.w = bw; a.x1 = x1; a.dy = dy; a.dx1 = dx1; a.slab = slab_mlp; a.ntok = ntok; a.drop = drop;
        a.dab = fast_rows ? dab_ws : nullptr;
        a.x1_bf16 = x1b;
        int rc = launch_block_bwd_mlp(a, grid_mlp, prec, st);
        if (rc) return fail(rc, "msst_block_bwd(mlp)");
    }
    // 2. attention half, per (chunk, head)
    int nparts = heads;
    {
        aa.w = bw; aa.x = x; aa.da = dx1; aa.dxn_part = dxn_part; aa.slab = slab_attn;
        aa.xn = fast_rows ? xn_saved : nullptr; aa.dab = fast_rows ? dab_ws : nullptr;
        aa.H = heads; aa.ntok = ntok; aa.scale = 0.125f; aa.drop = drop;
        aa.queue = (tile_queue && heads / 2 <= 32) ? tile_queue : nullptr;
        aa.lse = fast_rows ? lse_saved : nullptr;   // (only the two-head kernel reads it; launch_block_bwd_attn drops it for the others)
        aa.lse_renorm = (dbg & 8192) ? 1 : 0;       // MSST_LSE_RENORM: statistics of a half-operand forward
        aa.dbg = dbg & ~8;
        aa.stamps = nullptr;
#ifdef MSST_STAMPS
        aa.stamps = g_stamps;
        if (g_stamps) aa.dbg = dbg;
#elif defined(MSST_LAB)
        aa.stamps = g_stamps;
#endif
        int rc = launch_block_bwd_attn(aa, nc, prec, st, &nparts);
        if (rc) return fail(rc, "msst_block_bwd(attn)");
    }
    // 3. LN1 backward + residual -- alone, or fused with the MLP half of the block before (dx stays on chip)
    const bool fused = chain && w_prev;
    if (fused) {
        if (nparts > 4) return fail(MSST_ERR_UNSUPPORTED, "msst_block_bwd_chain (more than four d(LN1 out) partials)");
        LnMlpArgs a;
        a.w = to_bw(w_prev); a.ln1_g = w->ln1_g; a.x = x; a.dx1 = dx1; a.dxn_part = dxn_part; a.x1 = x1_prev; a.dab = dab_ws;
        a.x1_bf16 = x1b;
        // MSST_LN1_FROM_XN: xhat of LN1 from the saved bf16 LN1 rows + the saved rstd (the tail of the statistics buffer)
        a.xn = nullptr; a.rstd = nullptr; a.ln1_b = w->ln1_b;
        if (dbg & 2048) {
            if (!xn_saved || !lse_saved) return fail(MSST_ERR_BADARG, "msst_block_bwd_chain (MSST_LN1_FROM_XN needs xn_saved and lse_saved)");
            a.xn = xn_saved; a.rstd = lse_saved + (long)aa.ntiles * heads * 64;
        }
        a.slab_mlp = slab_mlp_prev; a.slab_ln1 = slab_ln1; a.ntok = ntok; a.nparts = nparts;
        a.drop_i = drop; a.drop_p = make_drop(dropout_p, seed, layer - 1);
        a.stamps = nullptr;
#ifdef MSST_STAMPS
        a.stamps = g_stamps;
#endif
        a.queue = tile_queue ? tile_queue + 32 : nullptr;
        int rc = launch_block_bwd_ln1mlp(a, grid, st);
        if (rc) return fail(rc, "msst_block_bwd_chain(ln1 + mlp)");
    } else {
        Ln1BwdArgs a;
        a.x = x; a.dx1 = dx1; a.dxn_part = dxn_part; a.ln1_g = w->ln1_g; a.dx = dx; a.slab = slab_ln1; a.ntok = ntok; a.H = nparts; a.drop = drop;
        int rc = launch_block_bwd_ln1(a, grid, prec, st);
        if (rc) return fail(rc, "msst_block_bwd(ln1)");
    }
    // 4. one deterministic reduction of all partial-gradient slabs written above -- unless the caller collects the slab sets of a
    //    run of chained calls and reduces them in one launch (MSST_BWD_DEFER_REDUCE, msst_block_bwd_reduce)
    if (!(chain && (dbg & 512))) {
        int rc = reduce_block_slabs(lay, heads, g, run_mlp ? g : nullptr, 1, fused ? g_prev : nullptr, 1, 1, 0, 0, st);
        if (rc) return fail(rc, "msst_block_bwd(reduce)");
    }
    return 0;
}

int msst_block_bwd(const MsstBlockWeights* w, const MsstBlockGrads* g, const float* x, const float* x1,
                   const float* dy, float* dx, float* dx1, void* dxn_part, float* slab, int grid_rows,
                   int nchunk, int mode, int B, int S, int N, int heads, int prec, float dropout_p,
                   uint32_t seed, int layer, const void* xn_saved, const float* lse_saved, void* dab_ws, void* stream) {
    return block_bwd_impl(w, g, nullptr, nullptr, x, x1, nullptr, dy, dx, dx1, dxn_part, slab, grid_rows, nchunk, mode, B, S, N,
                          heads, prec, dropout_p, seed, layer, xn_saved, lse_saved, dab_ws, 0, 0, nullptr, (hipStream_t)stream);
}

int msst_block_bwd_chain(const MsstBlockWeights* w, const MsstBlockGrads* g, const MsstBlockWeights* w_prev,
                         const MsstBlockGrads* g_prev, const float* x, const float* x1, const float* x1_prev,
                         const float* dy, float* dx, float* dx1, void* dxn_part, float* slab, int grid_rows,
                         int nchunk, int mode, int B, int S, int N, int heads, int prec, float dropout_p,
                         uint32_t seed, int layer, const void* xn_saved, const float* lse_saved, void* dab_ws, int first,
                         int32_t* tile_queue, void* stream) {
    return block_bwd_impl(w, g, w_prev, g_prev, x, x1, x1_prev, dy, dx, dx1, dxn_part, slab, grid_rows, nchunk, mode, B, S, N,
                          heads, prec, dropout_p, seed, layer, xn_saved, lse_saved, dab_ws, 1, first, tile_queue, (hipStream_t)stream);
}

int msst_block_bwd_reduce(const MsstBlockGrads* g, const MsstBlockGrads* g_prev, float* slab, long slab_stride, long grad_stride,
                          int count, int count_prev, int first, int grid_rows, int nchunk, int mode, int B, int S, int N, int heads,
                          int prec, void* stream) {
    if (int rc = block_shape(mode, B, S, N, heads)) return fail(rc, "msst_block_bwd_reduce (B, S, N, heads < 1, mode not 0 / 1, or sequence length > 64)");
    if (!g || count < 1 || count_prev < 0 || count_prev > count || (count_prev && !g_prev) || !slab || grid_rows < 1 || nchunk < 1 ||
        (count > 1 && ((slab_stride & 3) || (grad_stride & 3))))
        return fail(MSST_ERR_BADARG, "msst_block_bwd_reduce");
    prec &= 0xff;
    const long ntok = (long)B * S * N;
    const TileMap tm = make_tilemap(mode, B, S, N);
    const SlabLayout lay = slab_layout(slab, ntok, grid_rows, nchunk, ntiles_of(tm), heads, prec);
    return fail(reduce_block_slabs(lay, heads, g, first ? g : nullptr, 1, count_prev ? g_prev : nullptr, count_prev, count,
                                   slab_stride, grad_stride, (hipStream_t)stream), "msst_block_bwd_reduce");
}

// the tokenizer backward's second half: the slabs its kernel wrote, summed into the gradients (msst_tokenize_bwd and
// msst_tokenize_scene_bwd: one table, one summation order)
static int tokenize_bwd_reduce(float* slab, int nchunk, const TokGradPtrs& g, int S, int N, int P, hipStream_t st) {
    int rc = 0;
    const long ss = (long)N * 96 + 96 * P + 96 * 4 + 32;
    const long bs = (long)nchunk * ss;
    float* stage = slab + (long)S * nchunk * ss;  // [S][N][96] position-gradient staging
    float* dpos_dst = g.pos_split ? stage : g.dpos_a;
    const long v0 = (long)N * 96 + 96 * P;
    RSegBuilder rb;
    bool ok = true;
    for (int c = 0; c < S && ok; ++c) {   // per spectral block: position rows, embed weight, embed bias
        const float* sc = slab + c * bs;
        if (g.dpos_a) ok = rb.add(sc, ss, nchunk, dpos_dst + (long)c * N * 96, N * 96);   // null: position table applied by the caller
        ok = ok && rb.add(sc + N * 96, ss, nchunk, g.dw_emb + (long)c * 96 * P, 96 * P);
        ok = ok && rb.add(sc + v0, ss, nchunk, g.db_emb + (long)c * 96, 96);
        if (rb.r.nseg > MSST_MAX_RSEG - 8) {
            rc = launch_reduce_segs(rb.r, st);
            if (rc) return fail(rc, "msst_tokenize_bwd(reduce)");
            rb = RSegBuilder();
        }
    }
    // shared across blocks
    ok = ok && rb.add(slab + v0 + 96, ss, S * nchunk, g.dpost_g, 96);
    ok = ok && rb.add(slab + v0 + 192, ss, S * nchunk, g.dpost_b, 96);
    if (g.dmask_token) ok = ok && rb.add(slab + v0 + 288, ss, S * nchunk, g.dmask_token, 96);
    ok = ok && rb.add(slab + v0 + 384, ss, S * nchunk, g.dpre_g, P);
    ok = ok && rb.add(slab + v0 + 384 + 16, ss, S * nchunk, g.dpre_b, P);
    if (!ok) return fail(MSST_ERR_UNSUPPORTED, "msst_tokenize_bwd(reduce table)");
    rc = launch_reduce_segs(rb.r, st);
    if (!rc && g.pos_split && g.dpos_a) rc = launch_pos_split(stage, S, N, g.pos_split, g.dpos_a, g.dpos_b, st);
    return fail(rc, "msst_tokenize_bwd(reduce)");
}

// the four parameter backwards: the argument check of a window source (w null: a batch of cubes, unchecked as ever), nchunk, one launch
// over all samples, the slab reduction
static int tokenize_src_bwd(const char* what, const TokPtrs& p, const uint8_t* mask, bool masked, const float* dx0, float* slab, int nchunk,
                            const TokGradPtrs& g, WinSrc* w, int B, int S, int N, int P, Drop drop, void* stream) {
    if (w) {
        const bool pointers = p.all_set() && (!masked || mask) && dx0 && slab && g.all_set();
        if (int rc = check_src(*w, pointers, 1, S, P, g.pos_split)) return fail(rc, what);
    }
    if (nchunk < 1) return fail(MSST_ERR_BADARG, what);
    hipStream_t st = (hipStream_t)stream;
    TokBwdArgs a{};
    fill_tok_common(a, p, B, S, N, P, drop);
    a.mask = mask; a.dx0 = dx0; a.slab = slab;
    if (w) fill_src(a.src, *w);
    if (int rc = launch_tokenize_bwd(a, w ? w->kind() : WIN_BATCH, nchunk, st)) return fail(rc, what);
    return tokenize_bwd_reduce(slab, nchunk, g, S, N, P, st);
}

int msst_tokenize_bwd(const float* img, const float* pre_g, const float* pre_b, const float* w_emb,
                      const float* b_emb, const float* post_g, const float* post_b, const uint8_t* mask,
                      const float* dx0, float* slab, int nchunk, float* dpre_g, float* dpre_b,
                      float* dw_emb, float* db_emb, float* dpost_g, float* dpost_b, float* dpos_a,
                      float* dpos_b, int pos_split, float* dmask_token, int B, int S, int N, int P,
                      float emb_dropout_p, uint32_t seed, void* stream) {
    return tokenize_src_bwd("msst_tokenize_bwd", {img, pre_g, pre_b, w_emb, b_emb, post_g, post_b}, mask, false, dx0, slab, nchunk,
                            {dpre_g, dpre_b, dw_emb, db_emb, dpost_g, dpost_b, dpos_a, dpos_b, pos_split, dmask_token}, nullptr, B, S, N, P,
                            make_drop(emb_dropout_p, seed, 255), stream);
}

int msst_tokenize_scene_bwd(const float* scene, const float* pre_g, const float* pre_b, const float* w_emb,
                            const float* b_emb, const float* post_g, const float* post_b, const float* dx0, float* slab,
                            int nchunk, float* dpre_g, float* dpre_b, float* dw_emb, float* db_emb, float* dpost_g,
                            float* dpost_b, float* dpos_a, float* dpos_b, int pos_split, int Bs, int Hs, int Ws, int window,
                            int stride, long win0, int nwin, int S, int P, float emb_dropout_p, uint32_t seed, void* stream) {
    WinSrc w = WinSrc{Bs, Hs, Ws, window, stride, win0, nwin};
    return tokenize_src_bwd("msst_tokenize_scene_bwd", {scene, pre_g, pre_b, w_emb, b_emb, post_g, post_b}, nullptr, false, dx0, slab,
                            nchunk, {dpre_g, dpre_b, dw_emb, db_emb, dpost_g, dpost_b, dpos_a, dpos_b, pos_split, nullptr}, &w, nwin, S,
                            window * window, P, make_drop(emb_dropout_p, seed, 255), stream);
}

int msst_tokenize_at_bwd(const float* scene, const int32_t* origins, const float* pre_g, const float* pre_b, const float* w_emb,
                         const float* b_emb, const float* post_g, const float* post_b, const float* dx0, float* slab, int nchunk,
                         float* dpre_g, float* dpre_b, float* dw_emb, float* db_emb, float* dpost_g, float* dpost_b, float* dpos_a,
                         float* dpos_b, int pos_split, int Bs, int Hs, int Ws, int window, int nwin, int S, int P,
                         float emb_dropout_p, uint32_t seed, void* stream) {
    WinSrc w = WinSrc{Bs, Hs, Ws, window, window, 0, nwin, true, origins};
    return tokenize_src_bwd("msst_tokenize_at_bwd", {scene, pre_g, pre_b, w_emb, b_emb, post_g, post_b}, nullptr, false, dx0, slab, nchunk,
                            {dpre_g, dpre_b, dw_emb, db_emb, dpost_g, dpost_b, dpos_a, dpos_b, pos_split, nullptr}, &w, nwin, S,
                            window * window, P, make_drop(emb_dropout_p, seed, 255), stream);
}

int msst_tokenize_at_bwd_masked(const float* scene, const int32_t* origins, const float* pre_g, const float* pre_b, const float* w_emb,
                                const float* b_emb, const float* post_g, const float* post_b, const uint8_t* mask, const float* dx0,
                                float* slab, int nchunk, float* dpre_g, float* dpre_b, float* dw_emb, float* db_emb, float* dpost_g,
                                float* dpost_b, float* dpos_a, float* dpos_b, int pos_split, float* dmask_token, int Bs, int Hs, int Ws,
                                int window, int nwin, int S, int P, void* stream) {
    WinSrc w = WinSrc{Bs, Hs, Ws, window, window, 0, nwin, true, origins};
    return tokenize_src_bwd("msst_tokenize_at_bwd_masked", {scene, pre_g, pre_b, w_emb, b_emb, post_g, post_b}, mask, true, dx0, slab,
                            nchunk, {dpre_g, dpre_b, dw_emb, db_emb, dpost_g, dpost_b, dpos_a, dpos_b, pos_split, dmask_token}, &w, nwin, S,
                            window * window, P, make_drop(0.f, 0, 255), stream);
}

int msst_tokenize_at_bwd_orient(const float* scene, const int32_t* origins, const uint8_t* orient, const float* pre_g, const float* pre_b,
                                const float* w_emb, const float* b_emb, const float* post_g, const float* post_b, const float* dx0,
                                float* slab, int nchunk, float* dpre_g, float* dpre_b, float* dw_emb, float* db_emb, float* dpost_g,
                                float* dpost_b, float* dpos_a, float* dpos_b, int pos_split, int Bs, int Hs, int Ws, int window, int nwin,
                                int S, int P, float emb_dropout_p, uint32_t seed, void* stream) {
    WinSrc w = WinSrc{Bs, Hs, Ws, window, window, 0, nwin, true, origins, 1, 1, true, orient};
    return tokenize_src_bwd("msst_tokenize_at_bwd_orient", {scene, pre_g, pre_b, w_emb, b_emb, post_g, post_b}, nullptr, false, dx0, slab,
                            nchunk, {dpre_g, dpre_b, dw_emb, db_emb, dpost_g, dpost_b, dpos_a, dpos_b, pos_split, nullptr}, &w, nwin, S,
                            window * window, P, make_drop(emb_dropout_p, seed, 255), stream);
}

int msst_tokenize_at_bwd_masked_orient(const float* scene, const int32_t* origins, const uint8_t* orient, const float* pre_g,
                                       const float* pre_b, const float* w_emb, const float* b_emb, const float* post_g,
                                       const float* post_b, const uint8_t* mask, const float* dx0, float* slab, int nchunk, float* dpre_g,
                                       float* dpre_b, float* dw_emb, float* db_emb, float* dpost_g, float* dpost_b, float* dpos_a,
                                       float* dpos_b, int pos_split, float* dmask_token, int Bs, int Hs, int Ws, int window, int nwin,
                                       int S, int P, void* stream) {
    WinSrc w = WinSrc{Bs, Hs, Ws, window, window, 0, nwin, true, origins, 1, 1, true, orient};
    return tokenize_src_bwd("msst_tokenize_at_bwd_masked_orient", {scene, pre_g, pre_b, w_emb, b_emb, post_g, post_b}, mask, true, dx0,
                            slab, nchunk, {dpre_g, dpre_b, dw_emb, db_emb, dpost_g, dpost_b, dpos_a, dpos_b, pos_split, dmask_token}, &w,
                            nwin, S, window * window, P, make_drop(0.f, 0, 255), stream);
}

// ---- input gradient (msst_input_grad.hip)
int msst_tokenize_bwd_input(const float* img, const float* pre_g, const float* pre_b, const float* w_emb, const float* b_emb,
                            const float* post_g, const float* post_b, const uint8_t* mask, const float* dx0, const float* dtarget,
                            float* dimg, int B, int S, int N, int P, float emb_dropout_p, uint32_t seed, void* stream) {
    const TokPtrs p{img, pre_g, pre_b, w_emb, b_emb, post_g, post_b};
    if (B < 1 || S < 1 || N < 1 || P < 1) return fail(MSST_ERR_BADARG, "msst_tokenize_bwd_input");
    if (N > 64 || S > 64 || P > 16) return fail(MSST_ERR_UNSUPPORTED, "msst_tokenize_bwd_input");
    if (!p.all_set() || !dx0 || !dimg) return fail(MSST_ERR_BADARG, "msst_tokenize_bwd_input");
    TokInArgs a{};   // a batch of cubes: no window grid
    fill_tok_in(a, p, mask, dx0, dtarget, dimg, B, S, N, P, make_drop(emb_dropout_p, seed, 255));
    return fail(launch_tokenize_bwd_input(a, WIN_BATCH, (hipStream_t)stream), "msst_tokenize_bwd_input");
}

int msst_head_bwd_target(const float* dpred, const int32_t* csr_ptr, const int32_t* csr_pos, const float* gout, float* dtarget,
                         int B, int S, int N, int P, int K, void* stream) {
    if (B < 1 || S < 1 || N < 1 || P < 1 || K < 1) return fail(MSST_ERR_BADARG, "msst_head_bwd_target");
    if (N > 64 || S > 64 || P > 16) return fail(MSST_ERR_UNSUPPORTED, "msst_head_bwd_target");
    if (!dpred || !csr_ptr || !csr_pos || !dtarget) return fail(MSST_ERR_BADARG, "msst_head_bwd_target");
    const float gscale = (float)(1.0 / ((double)B * K * P) / K);   // the loss normalisation of msst_head_fwd: mean over B K P, then / K
    return fail(launch_head_bwd_target(dpred, csr_ptr, csr_pos, gout, gscale, dtarget, B, S, N, P, K, (hipStream_t)stream),
                "msst_head_bwd_target");
}

// the input gradient over a window source: into the scenes themselves (a grid of windows that do not overlap), or stacked per window
// (listed windows: msst_scene_fold_at sums them)
static int tokenize_src_bwd_input(const char* what, const TokPtrs& p, const float* dx0, float* dimg, WinSrc w, int S, int P, Drop drop,
                                  void* stream) {
    if (int rc = check_src(w, p.all_set() && dx0 && dimg, 0, S, P, 0)) return fail(rc, what);
    hipStream_t st = (hipStream_t)stream;
    if (!w.listed) {
        // overlapping windows would have to add into a pixel: only the non-overlapping grid of the tile path is built
        if (w.stride != w.window || S > 64) return fail(MSST_ERR_UNSUPPORTED, what, " (stride != window)");
        if (w.win0 == 0) {   // the call that starts a batch zeroes the pixels beyond the window grid
            const int nr = (int)(w.wps / w.nq);
            if (int rc = launch_scene_border_zero(dimg, (long)w.Bs * S * P * w.Hs, w.Hs, w.Ws, nr * w.window, w.nq * w.window, st))
                return fail(rc, what, "(border)");
        }
    }
    TokInArgs a{};
    fill_tok_in(a, p, nullptr, dx0, nullptr, dimg, w.nwin, S, w.window * w.window, P, drop);
    fill_src(a.src, w);
    return fail(launch_tokenize_bwd_input(a, w.kind(), st), what);
}

int msst_tokenize_scene_bwd_input(const float* scene, const float* pre_g, const float* pre_b, const float* w_emb, const float* b_emb,
                                  const float* post_g, const float* post_b, const float* dx0, float* dscene, int Bs, int Hs, int Ws,
                                  int window, int stride, long win0, int nwin, int S, int P, float emb_dropout_p, uint32_t seed,
                                  void* stream) {
    return tokenize_src_bwd_input("msst_tokenize_scene_bwd_input", {scene, pre_g, pre_b, w_emb, b_emb, post_g, post_b}, dx0, dscene,
                                  WinSrc{Bs, Hs, Ws, window, stride, win0, nwin}, S, P, make_drop(emb_dropout_p, seed, 255), stream);
}

int msst_tokenize_at_bwd_input(const float* scene, const int32_t* origins, const float* pre_g, const float* pre_b, const float* w_emb,
                               const float* b_emb, const float* post_g, const float* post_b, const float* dx0, float* dwin, int Bs,
                               int Hs, int Ws, int window, int nwin, int S, int P, float emb_dropout_p, uint32_t seed, void* stream) {
    return tokenize_src_bwd_input("msst_tokenize_at_bwd_input", {scene, pre_g, pre_b, w_emb, b_emb, post_g, post_b}, dx0, dwin,
                                  WinSrc{Bs, Hs, Ws, window, window, 0, nwin, true, origins}, S, P, make_drop(emb_dropout_p, seed, 255), stream);
}

int msst_scene_fold_at(const float* dwin, const int32_t* cell_ptr, const int32_t* cell_win, float* dscene, int Bs, int C, int Hs, int Ws,
                       int window, int nwin, int group, int accumulate, void* stream) {
    if (Bs < 1 || C < 1 || Hs < 1 || Ws < 1 || window < 1 || group < 1 || nwin < 0) return fail(MSST_ERR_BADARG, "msst_scene_fold_at");
    if (group > 16 || window > 8 || window > Hs || window > Ws) return fail(MSST_ERR_UNSUPPORTED, "msst_scene_fold_at");
    if (!cell_ptr || !dscene || (nwin > 0 && (!dwin || !cell_win))) return fail(MSST_ERR_BADARG, "msst_scene_fold_at");
    if (nwin == 0 && accumulate) return 0;   // nothing to add; without accumulate the launch writes the zeros
    SceneFoldAtArgs a;
    a.dwin = dwin; a.cell_ptr = cell_ptr; a.cell_win = cell_win; a.dscene = dscene;
    a.Bs = Bs; a.C = C; a.Hs = Hs; a.Ws = Ws; a.win = window; a.nwin = nwin; a.group = group; a.accumulate = accumulate != 0;
    return fail(launch_scene_fold_at(a, (hipStream_t)stream), "msst_scene_fold_at");
}

// shape of the default head: 0, MSST_ERR_BADARG (a size below 1) or MSST_ERR_UNSUPPORTED (beyond the kernels' limits; any n_classes)
static int cls_head_shape(int B, int S, int N, int n_classes) {
    if (B < 1 || S < 1 || N < 1 || n_classes < 1) return MSST_ERR_BADARG;
    if (S > 64 || N > 64) return MSST_ERR_UNSUPPORTED;
    return 0;
}

int msst_cls_head_fwd(const float* y, const float* ln_g, const float* ln_b, const float* w, const float* b,
                      float* logits, int B, int S, int N, int n_classes, void* stream) {
    const int rc = cls_head_shape(B, S, N, n_classes);
    if (rc) return fail(rc, "msst_cls_head_fwd");
    if (!y || !ln_g || !ln_b || !w || !b || !logits) return fail(MSST_ERR_BADARG, "msst_cls_head_fwd");
    ClsArgs a;
    a.y = y; a.ln_g = ln_g; a.ln_b = ln_b; a.w = w; a.b = b; a.logits = logits;
    a.B = B; a.S = S; a.N = N; a.T = S * N; a.NC = n_classes;
    return fail(launch_cls_head_fwd(a, (hipStream_t)stream), "msst_cls_head_fwd");
}

int msst_cls_head_bwd(const float* y, const float* dlogits, const float* ln_g, const float* ln_b, const float* w,
                      float* dy, float* slab, float* dln_g, float* dln_b, float* dw, float* db, int B, int S,
                      int N, int n_classes, void* stream) {
    int rc = cls_head_shape(B, S, N, n_classes);
    if (rc) return fail(rc, "msst_cls_head_bwd");
    if (!y || !dlogits || !ln_g || !ln_b || !w || !slab || !dln_g || !dln_b || !dw || !db)   // dy may be null: no dy wanted
        return fail(MSST_ERR_BADARG, "msst_cls_head_bwd");
    hipStream_t st = (hipStream_t)stream;
    ClsBwdArgs a;
    a.y = y; a.dlogits = dlogits; a.ln_g = ln_g; a.ln_b = ln_b; a.w = w; a.dy = dy; a.slab = slab;
    a.B = B; a.S = S; a.N = N; a.T = S * N; a.NC = n_classes;
    rc = launch_cls_head_bwd(a, st);
    if (rc) return fail(rc, "msst_cls_head_bwd");
    const long ss = (long)n_classes * 96 + n_classes + 192;
    RSegBuilder rb;
    bool ok = rb.add(slab, ss, B, dw, n_classes * 96);
    ok = ok && rb.add(slab + n_classes * 96, ss, B, db, n_classes);
    ok = ok && rb.add(slab + n_classes * 96 + n_classes, ss, B, dln_g, 96);
    ok = ok && rb.add(slab + n_classes * 96 + n_classes + 96, ss, B, dln_b, 96);
    if (!ok) return fail(MSST_ERR_UNSUPPORTED, "msst_cls_head_bwd");
    return fail(launch_reduce_segs(rb.r, st), "msst_cls_head_bwd(reduce)");
}

int msst_spec_head_fwd(const float* y, const float* ln_g, const float* ln_b, const float* w, const float* b,
                       float* logits, int B, int S, int N, int n_classes, void* stream) {
    SpecHeadArgs a = {};
    a.y = y; a.ln_g = ln_g; a.ln_b = ln_b; a.w = w; a.b = b; a.logits = logits;
    a.B = B; a.S = S; a.N = N; a.T = S * N; a.NC = n_classes; a.R = B * N;
    return fail(launch_spec_head_fwd(a, (hipStream_t)stream), "msst_spec_head_fwd");
}

long msst_spec_head_bwd_slab(int B, int S, int N, int n_classes) {
    return B < 1 || S < 1 || N < 1 || n_classes < 1 ? 0 : spec_head_bwd_slab_floats(B, S, N, n_classes);
}

int msst_spec_head_bwd(const float* y, const float* dlogits, const float* ln_g, const float* ln_b, const float* w,
                       float* dy, float* slab, float* dln_g, float* dln_b, float* dw, float* db, int B, int S,
                       int N, int n_classes, void* stream) {
    if (B < 1 || S < 1 || S > 64 || N < 1 || N > 64 || n_classes < 1 || n_classes > 32) return fail(MSST_ERR_UNSUPPORTED, "msst_spec_head_bwd");
    if (!y || !dlogits || !ln_g || !ln_b || !w || !slab || !dln_g || !dln_b || !dw || !db)   // dy may be null: no dy wanted
        return fail(MSST_ERR_BADARG, "msst_spec_head_bwd");
    hipStream_t st = (hipStream_t)stream;
    SpecHeadArgs a = {};
    a.y = y; a.dlogits = dlogits; a.ln_g = ln_g; a.ln_b = ln_b; a.w = w; a.dy = dy;
    a.B = B; a.S = S; a.N = N; a.T = S * N; a.NC = n_classes; a.R = B * N;
    spec_head_chunks(a.R, a.G, a.RC);
    const long F = 96L * S, stats = (2L * a.R + 3) / 4 * 4;
    a.stats = slab;
    a.slab = slab + stats;
    a.slab_stride = n_classes * F + 32;
    float* A = a.slab + (long)a.G * a.slab_stride;
    int rc = launch_spec_head_bwd_rows(a, st);
    if (!rc) rc = launch_spec_head_wgrad(a, st);
    if (rc) return fail(rc, "msst_spec_head_bwd");
    RSegBuilder rb;
    bool ok = rb.add(a.slab, a.slab_stride, a.G, A, (int)(n_classes * F));
    ok = ok && rb.add(a.slab + n_classes * F, a.slab_stride, a.G, db, n_classes);
    if (!ok) return fail(MSST_ERR_UNSUPPORTED, "msst_spec_head_bwd");
    rc = launch_reduce_segs(rb.r, st);
    if (!rc) rc = launch_spec_head_wgrad_finish(a, A, db, dw, dln_g, dln_b, st);
    return fail(rc, "msst_spec_head_bwd(reduce)");
}

// shape of the pixelwise head: 0, MSST_ERR_BADARG (a size below 1) or MSST_ERR_UNSUPPORTED (beyond the kernels' limits)
static int pix_head_shape(int B, int S, int N, int n_classes) {
    if (B < 1 || S < 1 || N < 1 || n_classes < 1) return MSST_ERR_BADARG;
    if (S > 64 || N > 64 || n_classes > 32) return MSST_ERR_UNSUPPORTED;
    return 0;
}

long msst_pix_head_fwd_ws(int B, int N) { return B < 1 || N < 1 || N > 64 ? 0 : 96L * B * N; }

int msst_pix_head_fwd(const float* y, const float* ln_g, const float* ln_b, const float* w, const float* b, float* logits,
                      float* ws, int B, int S, int N, int n_classes, void* stream) {
    int rc = pix_head_shape(B, S, N, n_classes);
    if (rc) return fail(rc, "msst_pix_head_fwd");
    if (!y || !ln_g || !ln_b || !w || !b || !logits || !ws) return fail(MSST_ERR_BADARG, "msst_pix_head_fwd");
    PixHeadArgs a = {};
    a.y = y; a.ln_g = ln_g; a.ln_b = ln_b; a.w = w; a.b = b; a.logits = logits; a.xn = ws;
    a.B = B; a.S = S; a.N = N; a.T = S * N; a.NC = n_classes; a.G = pix_head_groups(B);
    return fail(launch_pix_head_fwd(a, (hipStream_t)stream), "msst_pix_head_fwd");
}

long msst_pix_head_bwd_slab(int B, int S, int N, int n_classes) {
    return pix_head_shape(B, S, N, n_classes) ? 0 : pix_head_bwd_slab_floats(B, N, n_classes);
}

int msst_pix_head_bwd(const float* y, const float* dlogits, const float* ln_g, const float* ln_b, const float* w, float* dy,
                      float* slab, float* dln_g, float* dln_b, float* dw, float* db, int B, int S, int N, int n_classes,
                      void* stream) {
    int rc = pix_head_shape(B, S, N, n_classes);
    if (rc) return fail(rc, "msst_pix_head_bwd");
    if (!y || !dlogits || !ln_g || !ln_b || !w || !slab || !dln_g || !dln_b || !dw || !db)   // dy may be null: no dy wanted
        return fail(MSST_ERR_BADARG, "msst_pix_head_bwd");
    hipStream_t st = (hipStream_t)stream;
    PixHeadArgs a = {};
    a.y = y; a.dlogits = dlogits; a.ln_g = ln_g; a.ln_b = ln_b; a.w = w; a.dy = dy; a.slab = slab;
    a.B = B; a.S = S; a.N = N; a.T = S * N; a.NC = n_classes; a.G = pix_head_groups(B);
    const long K = 96L * N, G = a.G;
    const float* p_db = slab + G * n_classes * K;
    const float* p_dg = p_db + G * 32;
    const float* p_dbeta = p_dg + G * K;
    RSegBuilder rb;
    bool ok = rb.add(slab, n_classes * K, a.G, dw, (int)(n_classes * K));
    ok = ok && rb.add(p_db, 32, a.G, db, n_classes);
    ok = ok && rb.add(p_dg, 96, a.G * N, dln_g, 96);
    ok = ok && rb.add(p_dbeta, 96, a.G * N, dln_b, 96);
    if (!ok) return fail(MSST_ERR_UNSUPPORTED, "msst_pix_head_bwd");
    rc = launch_pix_head_bwd(a, st);
    if (rc) return fail(rc, "msst_pix_head_bwd");
    return fail(launch_reduce_segs(rb.r, st), "msst_pix_head_bwd(reduce)");
}

int msst_scene_centre_assemble(const float* win_logits, long win0, int nwin, float* logits, int64_t* classes, int Bs,
                               int n_classes, int Hs, int Ws, int window, int stride, int finalize, void* stream) {
    int nr = 0, nq = 0;
    if (!logits || !classes || (nwin > 0 && !win_logits) || n_classes < 1 || nwin < 0 || win0 < 0 ||
        !scene_grid(Bs, Hs, Ws, window, stride, &nr, &nq))
        return fail(MSST_ERR_BADARG, "msst_scene_centre_assemble");
    const long wps = (long)nr * nq;
    if (win0 + nwin > (long)Bs * wps) return fail(MSST_ERR_BADARG, "msst_scene_centre_assemble (windows out of range)");
    SceneArgs a;
    fill_grid(a, win0, nwin, Bs, Hs, Ws, window, stride, nr, nq);
    a.win_logits = win_logits; a.logits = logits; a.classes = classes; a.NC = n_classes;
    hipStream_t st = (hipStream_t)stream;
    int rc = launch_scene_centre_scatter(a, st);
    if (!rc && finalize) rc = launch_scene_centre_fill(a, st);
    return fail(rc, "msst_scene_centre_assemble");
}

int msst_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, long rows,
                       int D, float eps, void* stream) {
    return fail(launch_layernorm_fwd(x, gamma, beta, y, mean, rstd, rows, D, eps, (hipStream_t)stream), "msst_layernorm_fwd");
}

long msst_layernorm_bwd_slab(long rows, int D) { return rows < 1 || D < 1 ? 0 : (long)layernorm_bwd_grid(rows, D) * 2 * D; }

int msst_layernorm_bwd(const float* x, const float* gamma, const float* dy, float* dx, float* dgamma, float* dbeta, float* slab,
                       long rows, int D, float eps, void* stream) {
    if (!dgamma || !dbeta) return fail(MSST_ERR_BADARG, "msst_layernorm_bwd");
    hipStream_t st = (hipStream_t)stream;
    if (rows == 0) {   // "fully written" holds for an empty input too: the sums over no rows
        if (D < 1) return fail(MSST_ERR_BADARG, "msst_layernorm_bwd");
        if (hipMemsetAsync(dgamma, 0, sizeof(float) * D, st) != hipSuccess || hipMemsetAsync(dbeta, 0, sizeof(float) * D, st) != hipSuccess)
            return fail(MSST_ERR_BADARG, "msst_layernorm_bwd(memset)");
        return 0;
    }
    const int grid = layernorm_bwd_grid(rows, D);
    int rc = launch_layernorm_bwd(x, gamma, dy, dx, slab, grid, rows, D, eps, st);
    if (rc) return fail(rc, "msst_layernorm_bwd");
    RSegBuilder rb;
    bool ok = rb.add(slab, 2L * D, grid, dgamma, D);
    ok = ok && rb.add(slab + D, 2L * D, grid, dbeta, D);
    if (!ok) return fail(MSST_ERR_UNSUPPORTED, "msst_layernorm_bwd");
    return fail(launch_reduce_segs(rb.r, st), "msst_layernorm_bwd(reduce)");
}

// shape of a cross-entropy call: 0, MSST_ERR_BADARG (a size below 1) or MSST_ERR_UNSUPPORTED (2^31 rows or logits and beyond)
static int ce_shape(int R0, int n_classes, int M) {
    if (R0 < 1 || n_classes < 1 || M < 1) return MSST_ERR_BADARG;
    if ((long)R0 * M > 0x7fffffffL || (long)R0 * M > 0x7fffffffL / n_classes) return MSST_ERR_UNSUPPORTED;
    return 0;
}

long msst_ce_scratch_bytes(int R0, int n_classes, int M) {
    if (ce_shape(R0, n_classes, M)) return 0;
    return (long)ce_workgroups((long)R0 * M) * (5 + 2L * n_classes) * 4;
}

// the forward of both entry points: the arguments, the scratch (partial | [wpartial] | slab | [cslab]) and the two launches.
// ext: the layout of msst_ce_ext_fwd, which keeps the wpartial region whether or not the call is weighted
static int ce_forward(const float* logits, const int64_t* labels, const int64_t* skip, long ignore_index, const float* class_weight,
                      float label_smoothing, float* d, float* loss, int64_t* record, double* sums, int64_t* confusion, void* scratch,
                      bool ext, int R0, int n_classes, int M, void* stream, const char* what) {
    CeArgs a = {};
    a.logits = logits; a.labels = labels; a.skip = skip; a.d = d; a.loss = loss; a.record = record;
    a.rows = (long)R0 * M; a.ignore_index = ignore_index; a.NC = n_classes; a.M = M;
    a.w = class_weight; a.eps = label_smoothing; a.confusion = confusion; a.sums = sums;
    const long G = ce_workgroups(a.rows);
    a.partial = (float*)scratch;
    a.wpartial = ext ? a.partial + G : nullptr;
    a.slab = (int*)scratch + (ext ? 2 : 1) * G;
    a.cslab = confusion ? a.slab + G * (4 + 2L * n_classes) : nullptr;
    hipStream_t st = (hipStream_t)stream;
    const int rc = launch_ce_fwd(a, st);
    if (rc) return fail(rc, what);
    return fail(launch_ce_finish(a, st), what, "(finish)");
}

int msst_ce_stats_fwd(const float* logits, const int64_t* labels, const int64_t* skip, long ignore_index, float* d, float* loss,
                      int64_t* record, void* scratch, int R0, int n_classes, int M, void* stream) {
    const int rc = ce_shape(R0, n_classes, M);
    if (rc) return fail(rc, "msst_ce_stats_fwd");
    if (!logits || !labels || !loss || !record || !scratch) return fail(MSST_ERR_BADARG, "msst_ce_stats_fwd");   // skip and d are optional
    return ce_forward(logits, labels, skip, ignore_index, nullptr, 0.f, d, loss, record, nullptr, nullptr, scratch, false, R0, n_classes, M,
                      stream, "msst_ce_stats_fwd");
}

int msst_ce_bwd(const float* d, const int64_t* record, const float* gout, float* dlogits, int R0, int n_classes, int M, void* stream) {
    const int rc = ce_shape(R0, n_classes, M);
    if (rc) return fail(rc, "msst_ce_bwd");
    if (!d || !record || !dlogits) return fail(MSST_ERR_BADARG, "msst_ce_bwd");   // gout is optional (1)
    return fail(launch_ce_bwd(d, record, gout, dlogits, (long)R0 * n_classes * M, (hipStream_t)stream), "msst_ce_bwd");
}

static_assert(CE_CONF_MAX_CLASSES == MSST_CE_CONFUSION_MAX_CLASSES, "the kernels' confusion limit is the header's");

// shape of a call of the extended family, in the header's order: ce_shape, then the confusion matrix's class and scratch limits
static int ce_ext_shape(int R0, int n_classes, int M, bool confusion) {
    const int rc = ce_shape(R0, n_classes, M);
    if (rc) return rc;
    if (confusion && (n_classes > MSST_CE_CONFUSION_MAX_CLASSES ||
                      (long)ce_workgroups((long)R0 * M) * n_classes * n_classes > 0x7fffffffL))
        return MSST_ERR_UNSUPPORTED;
    return 0;
}

long msst_ce_ext_scratch_bytes(int R0, int n_classes, int M, int confusion) {
    if (ce_ext_shape(R0, n_classes, M, confusion != 0)) return 0;
    const long G = ce_workgroups((long)R0 * M);
    return G * (6 + 2L * n_classes + (confusion ? (long)n_classes * n_classes : 0)) * 4;
}

int msst_ce_ext_fwd(const float* logits, const int64_t* labels, const int64_t* skip, long ignore_index, const float* class_weight,
                    float label_smoothing, float* d, float* loss, int64_t* record, double* sums, int64_t* confusion, void* scratch,
                    int R0, int n_classes, int M, void* stream) {
    int rc = ce_shape(R0, n_classes, M);
    if (rc) return fail(rc, "msst_ce_ext_fwd");
    if (!(label_smoothing >= 0.f && label_smoothing < 1.f)) return fail(MSST_ERR_BADARG, "msst_ce_ext_fwd (label_smoothing outside [0, 1))");
    rc = ce_ext_shape(R0, n_classes, M, confusion != nullptr);
    if (rc) return fail(rc, "msst_ce_ext_fwd (confusion matrix: more than MSST_CE_CONFUSION_MAX_CLASSES classes, or 2^31 scratch words)");
    if (!logits || !labels || !loss || !record || !sums || !scratch)   // skip, class_weight, d and confusion are optional
        return fail(MSST_ERR_BADARG, "msst_ce_ext_fwd");
    return ce_forward(logits, labels, skip, ignore_index, class_weight, label_smoothing, d, loss, record, sums, confusion, scratch, true,
                      R0, n_classes, M, stream, "msst_ce_ext_fwd");
}

int msst_ce_ext_bwd(const float* d, const double* sums, const float* gout, float* dlogits, int R0, int n_classes, int M, void* stream) {
    const int rc = ce_shape(R0, n_classes, M);
    if (rc) return fail(rc, "msst_ce_ext_bwd");
    if (!d || !sums || !dlogits) return fail(MSST_ERR_BADARG, "msst_ce_ext_bwd");   // gout is optional (1)
    return fail(launch_ce_ext_bwd(d, sums, gout, dlogits, (long)R0 * n_classes * M, (hipStream_t)stream), "msst_ce_ext_bwd");
}

int msst_recon_fwd(const float* y, const float* img, const uint8_t* mask, const float* w_pix, const float* b_pix, int per_block,
                   int blend, float* recon, double* band_err, int32_t* band_cnt, int B, int S, int N, int P, void* stream) {
    if (B < 1 || S < 1 || N < 1 || P < 1) return fail(MSST_ERR_BADARG, "msst_recon_fwd");
    if (N > 64 || S > 64 || P > 16) return fail(MSST_ERR_UNSUPPORTED, "msst_recon_fwd (N <= 64, S <= 64, P <= 16)");
    if (!y || !img || !mask || !w_pix || !b_pix || !recon || (band_err == nullptr) != (band_cnt == nullptr))
        return fail(MSST_ERR_BADARG, "msst_recon_fwd (null argument, or one of band_err / band_cnt without the other)");
    if ((uintptr_t)y & 15) return fail(MSST_ERR_BADARG, "msst_recon_fwd (y not 16-byte aligned)");
    ReconArgs a;
    a.y = y; a.img = img; a.mask = mask; a.w_pix = w_pix; a.b_pix = b_pix; a.recon = recon; a.band_err = band_err; a.band_cnt = band_cnt;
    a.B = B; a.S = S; a.N = N; a.P = P; a.per_block = per_block ? 1 : 0; a.blend = blend ? 1 : 0;
    return fail(launch_recon_fwd(a, (hipStream_t)stream), "msst_recon_fwd");
}

int msst_adamw(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2,
               float eps, float weight_decay, int step, float clamp, float gscale, void* stream) {
    return fail(launch_adamw(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step, clamp, gscale,
                             (hipStream_t)stream), "msst_adamw");
}

int msst_adam_groups(float* p, const float* g, float* m, float* v, const MsstAdamGroup* groups, int ngroups, int group_bytes,
                     double beta1, double beta2, float eps, float gscale, void* stream) {
    if (group_bytes != (int)sizeof(MsstAdamGroup)) return fail(MSST_ERR_BADARG, "msst_adam_groups (MsstAdamGroup of another header revision)");
    if (ngroups < 0 || ngroups > MSST_ADAM_MAX_GROUPS) return fail(MSST_ERR_BADARG, "msst_adam_groups (more than MSST_ADAM_MAX_GROUPS ranges)");
    if (ngroups == 0) return 0;
    if (!groups) return fail(MSST_ERR_BADARG, "msst_adam_groups (null table)");
    if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0)) return fail(MSST_ERR_BADARG, "msst_adam_groups (beta outside [0, 1))");
    // the whole table is validated before anything is enqueued
    long prev_end = 0;
    for (int i = 0; i < ngroups; ++i) {
        const MsstAdamGroup& q = groups[i];
        if (q.start < 0 || q.end < q.start) return fail(MSST_ERR_BADARG, "msst_adam_groups (range with end < start)");
        if (q.start < prev_end) return fail(MSST_ERR_BADARG, "msst_adam_groups (ranges overlap or are not sorted by start)");
        if (q.step < 1) return fail(MSST_ERR_BADARG, "msst_adam_groups (step < 1)");
        if (q.flags & ~MSST_ADAM_DECOUPLED) return fail(MSST_ERR_BADARG, "msst_adam_groups (unknown flag)");
        prev_end = q.end;
    }
    const bool aligned = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
    AdamTable t;
    t.nseg = 0; t.nblocks = 0;
    t.b2 = (float)beta2; t.omb1 = (float)(1.0 - beta1); t.omb2 = (float)(1.0 - beta2); t.eps = eps; t.gscale = gscale;
    constexpr long QPB = ADAM_QPB;
    for (int i = 0; i < ngroups; ++i) {
        const MsstAdamGroup& q = groups[i];
        if (q.end == q.start) continue;
        AdamSeg& s = t.s[t.nseg++];
        s.start = q.start; s.end = q.end;
        s.a0 = (q.start + 3) & ~3L;
        s.a1 = q.end & ~3L;
        if (!aligned || s.a1 <= s.a0) s.a0 = s.a1 = q.end;   // no aligned interior: the range moves float by float
        const bool dec = (q.flags & MSST_ADAM_DECOUPLED) != 0;
        s.step_size = (float)((double)q.lr / (1.0 - pow(beta1, (double)q.step)));
        s.bc2_sqrt = (float)sqrt(1.0 - pow(beta2, (double)q.step));
        s.wd = dec ? 0.f : q.weight_decay;
        s.decay = dec ? (float)(1.0 - (double)q.lr * (double)q.weight_decay) : 1.f;
        s.blk0 = t.nblocks; s.pad = 0;
        const long nb = ((s.a1 - s.a0) / 4 + QPB - 1) / QPB;
        const long total = (long)t.nblocks + (nb < 1 ? 1 : nb);
        if (total > 0x7fffffffL) return fail(MSST_ERR_UNSUPPORTED, "msst_adam_groups (grid)");
        t.nblocks = (int)total;
    }
    if (!t.nseg) return 0;
    if (!p || !g || !m || !v) return fail(MSST_ERR_BADARG, "msst_adam_groups (null buffer)");
    return fail(launch_adam_groups(p, g, m, v, t, (hipStream_t)stream), "msst_adam_groups");
}

// ---- gradient accumulation and the global-norm clip (msst_accum.hip) ----
// the checks both entry points share, in the order include/msst.h states; `have_ptrs`: every required pointer of the caller is non-null
static int grad_ranges_check(const char* what, bool have_ptrs, const MsstGradRange* ranges, int nranges, int range_bytes) {
    if (!have_ptrs || !ranges) return fail(MSST_ERR_BADARG, what, " (null argument)");
    if (nranges < 1) return fail(MSST_ERR_BADARG, what, " (nranges < 1)");
    if (range_bytes != (int)sizeof(MsstGradRange)) return fail(MSST_ERR_BADARG, what, " (MsstGradRange of another header revision)");
    if (nranges > MSST_GRAD_MAX_RANGES) return fail(MSST_ERR_UNSUPPORTED, what, " (more than MSST_GRAD_MAX_RANGES ranges)");
    long prev_end = 0;
    for (int i = 0; i < nranges; ++i) {
        if (ranges[i].start < 0 || ranges[i].end <= ranges[i].start) return fail(MSST_ERR_BADARG, what, " (range with end <= start)");
        if (ranges[i].start < prev_end) return fail(MSST_ERR_BADARG, what, " (ranges overlap or are not ascending)");
        prev_end = ranges[i].end;
    }
    return 0;
}

// The workgroups of either launch over the table: range i gets one per 256 * GRAD_U float4 pieces of its aligned interior (at least
// one), scaled down together when that exceeds GRAD_GRID; nblocks <= GRAD_GRID + nranges.  The split depends on the element ranges
// alone, so the finalize launch knows how many partials the accumulate launch left; buffers that are not 16-byte aligned themselves
// only empty the interiors (the first workgroup of a range then walks all of it float by float, the others find nothing).
static void grad_table(GradTable& t, const MsstGradRange* ranges, int nranges, bool aligned) {
    long need[MSST_GRAD_MAX_RANGES], total = 0;
    const long per = 256L * GRAD_U, grid_cap = GRAD_GRID;
    for (int i = 0; i < nranges; ++i) {
        GradSeg& s = t.s[i];
        s.start = ranges[i].start; s.end = ranges[i].end;
        s.a0 = (s.start + 3) & ~3L;
        s.a1 = s.end & ~3L;
        if (s.a1 <= s.a0) s.a0 = s.a1 = s.end;
        need[i] = ((s.a1 - s.a0) / 4 + per - 1) / per;
        if (need[i] < 1) need[i] = 1;
        total += need[i];
        if (!aligned) s.a0 = s.a1 = s.end;
    }
    t.nseg = nranges; t.nblocks = 0;
    for (int i = 0; i < nranges; ++i) {
        long nb = total <= grid_cap ? need[i] : need[i] * grid_cap / total;
        if (nb < 1) nb = 1;
        t.s[i].blk0 = t.nblocks; t.s[i].nblk = (int)nb;
        t.nblocks += (int)nb;
    }
}

long msst_grad_accum_scratch_bytes(int nranges) {
    if (nranges < 1 || nranges > MSST_GRAD_MAX_RANGES) return 0;
    return ((long)(GRAD_GRID + nranges) * (long)(sizeof(double) + sizeof(unsigned)) + 15) & ~15L;
}

int msst_grad_accumulate(float* acc, const float* g, const MsstGradRange* ranges, int nranges, int range_bytes, int first, float* out,
                         float scale, void* scratch, void* stream) {
    const int rc = grad_ranges_check("msst_grad_accumulate", acc && g, ranges, nranges, range_bytes);
    if (rc) return rc;
    if ((uintptr_t)scratch & 7) return fail(MSST_ERR_BADARG, "msst_grad_accumulate (scratch not 8-byte aligned)");
    if (out == acc || g == acc) return fail(MSST_ERR_BADARG, "msst_grad_accumulate (g and out must not be acc)");
    const bool aligned = (((uintptr_t)acc | (uintptr_t)g | (uintptr_t)out) & 15) == 0;
    GradTable t;
    grad_table(t, ranges, nranges, aligned);
    double* part_sum = (double*)scratch;
    unsigned* part_bad = scratch ? (unsigned*)(part_sum + t.nblocks) : nullptr;
    return fail(launch_grad_accumulate(acc, g, out, scale, first != 0, part_sum, part_bad, t, (hipStream_t)stream), "msst_grad_accumulate");
}

int msst_grad_finalize(const float* acc, float* g, const MsstGradRange* ranges, int nranges, int range_bytes, float scale, float max_norm,
                       const void* scratch, float* record, void* stream) {
    const int rc = grad_ranges_check("msst_grad_finalize", acc && g && scratch && record, ranges, nranges, range_bytes);
    if (rc) return rc;
    if ((uintptr_t)scratch & 7) return fail(MSST_ERR_BADARG, "msst_grad_finalize (scratch not 8-byte aligned)");
    if ((const void*)acc == (const void*)g) return fail(MSST_ERR_BADARG, "msst_grad_finalize (g must not be acc)");
    GradTable t;
    grad_table(t, ranges, nranges, (((uintptr_t)acc | (uintptr_t)g) & 15) == 0);
    const double* part_sum = (const double*)scratch;   // one slot per workgroup of the accumulate launch: the same split
    const unsigned* part_bad = (const unsigned*)(part_sum + t.nblocks);
    return fail(launch_grad_finalize(acc, g, scale, max_norm, part_sum, part_bad, t.nblocks, record, t, (hipStream_t)stream), "msst_grad_finalize");
}

}  // extern "C"
