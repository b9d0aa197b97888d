"""Shared by tests/test_tok_head_host.py and tests/test_gpu_tok_head_kernels.py: float64 restatements of the tokenizer
(msst_tokenize_fwd / msst_tokenize_bwd) and of the SimMIM head (msst_head_fwd / msst_head_bwd), and the case tables both files walk.
CPU only; every input comes from a seeded CPU float64 generator, every reference is computed once per case and left unchanged."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

D = 96
BAR = 2e-5          # rel-L2 per tensor against float64: the bar of test_gpu_input_grad.py::test_tokenize_bwd_input_vs_float64
MARGIN = 3.5        # the project's margin convention: a case may enter the tables only if fp32 autograd on the CPU stays within BAR / MARGIN
BAND = 1e-4         # |pred - target| below this: the sign of the L1 loss is not compared
BAND_SHARE = 1e-3   # at most this share of a case's dpred elements may lie in the band
DROP = (0.3, 4711)  # (emb_dropout_p, seed) of the dropout rows
GOUT = 0.37


# ---------------------------------------------------------------------------------------------- tokenizer
def tok_params(S, P, gen):
    """pre-norm gamma / beta [P], W [S, 96, P], b [S, 96], post-norm gamma / beta [96]: float64 on the CPU, away from the init values"""
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)   # noqa: E731
    return dict(pre_g=1 + 0.3 * r(P), pre_b=0.2 * r(P), w=r(S, 96, P) / max(P, 1) ** 0.5, b=0.1 * r(S, 96), post_g=1 + 0.3 * r(96),
                post_b=0.2 * r(96))


def tok_ref(img, q, S, N, P):
    """LN(P) -> per-block Linear -> LN(96) on img [B, S P, N] -> tokens [B, S N, 96] (token order c n), float64"""
    B = img.shape[0]
    patches = img.reshape(B, S, P, N).permute(0, 1, 3, 2)
    xn = F.layer_norm(patches, (P,), q["pre_g"], q["pre_b"], 1e-5)
    e = torch.einsum("bsnp,sdp->bsnd", xn, q["w"]) + q["b"][None, :, None, :]
    return F.layer_norm(e, (96,), q["post_g"], q["post_b"], 1e-5).reshape(B, S * N, 96)


def pos_rows(pos, S, N):
    """the additive table [S N, 96]: `pos` itself (learned), or from the split form (pos_a [N, split], pos_b [S, 96 - split]): token
    (c, n), feature d < split takes pos_a[n, d], the others pos_b[c, d - split] (include/msst.h, msst_tokenize_fwd)"""
    if isinstance(pos, (tuple, list)):
        pa, pb = pos
        return torch.cat([pa[None, :, :].expand(S, N, -1), pb[:, None, :].expand(S, N, -1)], dim=-1).reshape(S * N, D)
    return pos


def tokenizer_ref(img, q, mask, pos, keep):
    """msst_tokenize_fwd: (where(mask, mask_token, tok_ref(img)) + position rows) * keep.  img [B, S P, N]; q: tok_params plus
    "mask_token" [96]; mask [B, S N] bool; pos: pos_rows; keep: the dropout keep mask times its scale [B, S N, 96], or 1"""
    S, _, P = q["w"].shape
    N = img.shape[2]
    tok = torch.where(mask[..., None], q["mask_token"], tok_ref(img, q, S, N, P))
    return (tok + pos_rows(pos, S, N)) * keep


# ---------------------------------------------------------------------------------------------- head
def head_ref(y, img, idx, w_pix, b_pix, per_block):
    """msst_head_fwd: pred[b, k] = W_c y[b, idx[b, k]] + b_c, c = idx // N (0 in both tables when per_block == 0); target: the raw pixels
    img[b, c P + p, n]; loss = mean|pred - target| / K.  y [B, S N, 96], img [B, S P, N], idx [B, K] int64, w_pix [S or 1, P, 96],
    b_pix [S or 1, P] -> (pred [B, K, P], target [B, K, P], loss)"""
    B, SP, N = img.shape
    P = w_pix.shape[1]
    S, K = SP // P, idx.shape[1]
    br = torch.arange(B)[:, None]
    wc = idx // N if per_block else torch.zeros_like(idx)
    pred = torch.einsum("bkd,bkpd->bkp", y[br, idx], w_pix[wc]) + b_pix[wc]
    target = img.reshape(B, S, P, N).permute(0, 1, 3, 2).reshape(B, S * N, P)[br, idx]
    return pred, target, (pred - target).abs().mean() / K


def head_bwd_ref(y, dpred, idx, w_pix, per_block, gscale, gout):
    """msst_head_bwd: g[b, t] = gscale gout sum_{k : idx[b, k] = t} dpred[b, k] (index_add: a row may name a token more than once);
    dy = g W_c, dW_c = sum_{b, n} g^T y, db_c = sum g -> (dy [B, S N, 96], dw like w_pix, db like b_pix)"""
    B, T, _ = y.shape
    P = w_pix.shape[1]
    g = torch.zeros(B, T, P, dtype=y.dtype)
    for b in range(B):
        g[b].index_add_(0, idx[b], dpred[b])
    g = g * (gscale * gout)
    if per_block:
        S = w_pix.shape[0]
        gs, ys = g.reshape(B, S, T // S, P), y.reshape(B, S, T // S, D)
        return torch.einsum("bsnp,spd->bsnd", gs, w_pix).reshape(B, T, D), torch.einsum("bsnp,bsnd->spd", gs, ys), gs.sum(dim=(0, 2))
    return g @ w_pix[0], torch.einsum("btp,btd->pd", g, y)[None], g.sum(dim=(0, 1))[None]


# ---------------------------------------------------------------------------------------------- case tables
MASKS3 = ("none", "random", "all")
NODROP = ((0.0, 0),)
BOTH = ((0.0, 0), DROP)


def _tok(name, kernel, B, S, N, P, split, nchunks, masks=("random",), drops=NODROP, null_pos=False):
    return dict(name=name, kernel=kernel, B=B, S=S, N=N, P=P, split=split, nchunks=nchunks, masks=masks, drops=drops, null_pos=null_pos)


# the smallest shapes that reach each tokenizer backward kernel (P = 10 and N = 64: tokenize_bwd_mfma; P = 10: tokenize_bwd_kernel<10>;
# else <0>) and each walk length: nchunk 1, 2, 4, 11 over B = 11 are walks of 11, 6 / 5, 3 / 3 / 3 / 2 and 1 samples.  S = 21 / 22
# straddles the reduce-table flush (3 segments per spectral block, flush above 64 of 72), S = 64 takes three tables.  P <= 2 stays out:
# the gradient of a LayerNorm over one or two pixels is ill conditioned and fp32 autograd itself misses BAR there.
# null_pos: also run with dpos_a, dpos_b and dmask_token null (the classification path)
TOK_CASES = [
    _tok("mfma_B11_S2", "mfma", 11, 2, 64, 10, 0, (1, 2, 4, 11), MASKS3, BOTH, null_pos=True),
    _tok("mfma_B7_S3_split48", "mfma", 7, 3, 64, 10, 48, (1, 3)),
    _tok("p10_B11_S3_N25", "<10>", 11, 3, 25, 10, 0, (1, 2, 11), MASKS3, BOTH),
    _tok("p10_B6_S5_N1", "<10>", 6, 5, 1, 10, 0, (1, 4)),
    _tok("gen_B13_S2_N49_P16_split32", "<0>", 13, 2, 49, 16, 32, (1, 3), MASKS3, BOTH, null_pos=True),
    _tok("gen_B7_S21_N4_P3", "<0>", 7, 21, 4, 3, 0, (2,)),
    _tok("gen_B7_S22_N4_P3", "<0>", 7, 22, 4, 3, 0, (2,)),
    _tok("gen_B5_S64_N9_P5", "<0>", 5, 64, 9, 5, 0, (2,)),
]
# forward only: msst_tokenize_fwd takes nchunk = min(B, 1024 // S) for the mfma kernel, so several samples per forward chunk need
# S = 64: 16 chunks of 3 / 3 / 3 / 2 ... samples
TOK_FWD_BIG = dict(name="mfma_fwd_B35_S64", kernel="mfma", B=35, S=64, N=64, P=10, split=0, masks=("random",), drops=NODROP)
TOK_BY_NAME = {c["name"]: c for c in TOK_CASES + [TOK_FWD_BIG]}
TOK_GRADS = ("dpre_g", "dpre_b", "dw_emb", "db_emb", "dpost_g", "dpost_b", "dpos_a", "dpos_b", "dmask_token")
TOK_GRADS_NO_POS = TOK_GRADS[:6]


def _head(name, kernel, B, S, N, P, K, per_block, nchunks):
    return dict(name=name, kernel=kernel, B=B, S=S, N=N, P=P, K=K, per_block=per_block, nchunks=nchunks)


# head backward: P = 10 and N = 64 run head_bwd_mfma, everything else head_bwd_kernel.  With per_block the reduce table takes 2 segments
# per spectral block and flushes above 70 of 72: S = 36 fills it exactly, S = 37 flushes.  nchunk <= B, as the engine guarantees
HEAD_CASES = [
    _head("mfma_B11_S2_K65_pb", "mfma", 11, 2, 64, 10, 65, 1, (1, 2, 4, 11)),
    _head("mfma_B7_S3_K130_shared", "mfma", 7, 3, 64, 10, 130, 0, (1, 3)),
    _head("gen_B11_S3_N25_K63_pb", "generic", 11, 3, 25, 10, 63, 1, (1, 2)),
    _head("gen_B13_S2_N49_P16_K64_shared", "generic", 13, 2, 49, 16, 64, 0, (3,)),
    _head("gen_B5_S36_N4_P3_K70_pb", "generic", 5, 36, 4, 3, 70, 1, (2,)),
    _head("gen_B5_S37_N4_P3_K70_pb", "generic", 5, 37, 4, 3, 70, 1, (2,)),
    _head("gen_B6_S5_N1_P5_K1_pb", "generic", 6, 5, 1, 5, 1, 1, (4,)),
]
HEAD_BY_NAME = {c["name"]: c for c in HEAD_CASES}


def _seed(name):
    return int(np.frombuffer(name.encode(), dtype=np.uint8).astype(np.int64).dot(np.arange(1, len(name) + 1)) % 100003)


@functools.lru_cache(maxsize=None)
def tok_inputs(name):
    """float64 inputs of a tokenizer case: q (tok_params + mask_token), pos (pos_rows form), img, dx0, masks {name: bool [B, S N]}.
    Scales of tok_params; img = 1.5 randn + 0.3; position table(s) and mask token non-zero, so that under dropout a dropped element of
    msst_tokenize_fwd's output is an exact 0 and a kept one is not"""
    c = TOK_BY_NAME[name]
    B, S, N, P, split = c["B"], c["S"], c["N"], c["P"], c["split"]
    gen = torch.Generator().manual_seed(_seed(name))
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)   # noqa: E731
    q = tok_params(S, P, gen)
    q["mask_token"] = r(D)
    pos = (r(N, split), r(S, D - split)) if split else r(S * N, D)
    img = r(B, S * P, N) * 1.5 + 0.3
    dx0 = r(B, S * N, D) if "nchunks" in c else None
    masks = {"none": torch.zeros(B, S * N, dtype=torch.bool), "random": torch.rand(B, S * N, generator=gen) < 0.5,
             "all": torch.ones(B, S * N, dtype=torch.bool)}
    return dict(q=q, pos=pos, img=img, dx0=dx0, masks=masks)


def tok_autograd(q, pos, img, mask, dx0, keep=1.0, dtype=torch.float64):
    """autograd of sum(tokenizer_ref * dx0) in `dtype` -> {TOK_GRADS name: tensor} (dpos_b: None for a learned table) and "dx0_colsum",
    the per-feature sum of the dropout-applied dx0 rows [96], the quantity the kernels subtract dmask_token from"""
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_(True)   # noqa: E731
    split = isinstance(pos, (tuple, list))
    q = {k: leaf(v) for k, v in q.items()}
    pos = tuple(leaf(t) for t in pos) if split else leaf(pos)
    keep = keep.to(dtype) if torch.is_tensor(keep) else keep
    dx0 = dx0.detach().to(dtype)
    out = tokenizer_ref(img.detach().to(dtype), q, mask, pos, keep)
    (out * dx0).sum().backward()
    g = dict(dpre_g=q["pre_g"].grad, dpre_b=q["pre_b"].grad, dw_emb=q["w"].grad, db_emb=q["b"].grad, dpost_g=q["post_g"].grad,
             dpost_b=q["post_b"].grad, dmask_token=q["mask_token"].grad)
    g["dpos_a"], g["dpos_b"] = (pos[0].grad, pos[1].grad) if split else (pos.grad, None)
    g["dx0_colsum"] = (dx0 * keep).sum(dim=(0, 1))
    return g


def tok_grads_ref(name, mname, keep=1.0, dtype=torch.float64):
    """tok_autograd on the inputs of a case of TOK_CASES under its mask `mname`"""
    x = tok_inputs(name)
    return tok_autograd(x["q"], x["pos"], x["img"], x["masks"][mname], x["dx0"], keep, dtype)


def synthetic_keep(name, p=DROP[0], seed=1):
    """a seeded keep mask times its scale with the statistics of the kernels' (the host has no kernel to read the real one from)"""
    c = TOK_BY_NAME[name]
    gen = torch.Generator().manual_seed(seed)
    thr = int(p * 65536.0 + 0.5)
    return (torch.rand(c["B"], c["S"] * c["N"], D, generator=gen) >= thr / 65536.0).double() / (1.0 - thr / 65536.0)


def drop_scale(p):
    """msst_api.hip make_drop: the exact inverse of the realised keep probability"""
    thr = int(p * 65536.0 + 0.5)
    return 1.0 / (1.0 - thr / 65536.0)


def index_rows(B, K, T, gen):
    """[B, K] int64, drawn with replacement (rows hold unnamed tokens, tokens named twice and three or more times).  Row 0 names one
    token K times, the longest possible duplicate list; row 1 holds token 0 and token T - 1 (K = 1: row 1 holds token 0, row 2 token T - 1)"""
    idx = torch.randint(0, T, (B, K), generator=gen)
    idx[0, :] = int(torch.randint(0, T, (1,), generator=gen))
    idx[1, 0] = 0
    if K >= 2:
        idx[1, K - 1] = T - 1
    else:
        idx[2, 0] = T - 1
    return idx


@functools.lru_cache(maxsize=None)
def head_inputs(name):
    """float64 inputs of a head case: y, img, w_pix = randn / sqrt(96), b_pix, dpred (random normal: the backward is linear in it, which
    is stricter than signs), idx (index_rows), its inverse CSR (maskedsst_amd.masking.inverse_csr), gscale"""
    from maskedsst_amd.masking import inverse_csr
    c = HEAD_BY_NAME[name]
    B, S, N, P, K = c["B"], c["S"], c["N"], c["P"], c["K"]
    T, nw = S * N, (S if c["per_block"] else 1)
    gen = torch.Generator().manual_seed(_seed(name))
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)   # noqa: E731
    y, img, w_pix, b_pix, dpred = r(B, T, D), r(B, S * P, N) * 1.5 + 0.3, r(nw, P, D) / D ** 0.5, 0.1 * r(nw, P), r(B, K, P)
    idx = index_rows(B, K, T, gen)
    ptr, pos = inverse_csr(idx.numpy(), T)
    return dict(y=y, img=img, w_pix=w_pix, b_pix=b_pix, dpred=dpred, idx=idx, csr_ptr=torch.from_numpy(ptr), csr_pos=torch.from_numpy(pos),
                gscale=1.0 / (B * K * P) / K)


@functools.lru_cache(maxsize=None)
def head_fwd_ref(name):
    c, x = HEAD_BY_NAME[name], head_inputs(name)
    return head_ref(x["y"], x["img"], x["idx"], x["w_pix"], x["b_pix"], c["per_block"])


@functools.lru_cache(maxsize=None)
def head_grads_ref(name, gout):
    c, x = HEAD_BY_NAME[name], head_inputs(name)
    return head_bwd_ref(x["y"], x["dpred"], x["idx"], x["w_pix"], c["per_block"], x["gscale"], gout)
