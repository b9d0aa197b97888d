"""GPU: attention maps -- msst_attn_maps alone against float64 at the shapes where its tiling can go wrong, its determinism and
batch independence, ViTSpatialSpectral.attention_maps / SimMIMSpatialSpectral.attention_maps against the float64 softmax of the
oracle's block inputs (fp32) and of the model's own block inputs (bf16), tools/attn_maps_time.py and finetune.py --val-attention.

Bars.  |P - P64| <= 1e-4: the project's standing bar for its fp32 kernels; an fp32 restatement of the maps
sits at <= 6.1e-7 from float64 in numpy, a 3 % error of the softmax scale moves these (peaky) maps by >= 8e-3.  Row sums: 128 * 2^-24
(a 64-term fp32 sum, its reciprocal and the product).  MEAN_SEQ against the float64 mean of the kernel's own PER_SEQ output:
(G + 1) * 2^-24 (G fp32 additions of terms <= 1 and one division).
Measured on an MI355X (profiles/attn_maps_parity_measured.jsonl): kernel <= 1.1e-6, row sums <= 2.3e-7, mean against per-sequence
<= 8.1e-8; fp32 model against the oracle <= 1.7e-5 (peaky weights; 1.8e-7 otherwise); bf16 model against its own block inputs <= 2.8e-6."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, oracle_cfg_from
from util import build_product, record

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
PER_SEQ, MEAN_SEQ = 0, 1
SPATIAL, SPECTRAL = 0, 1


def _p(t):
    import ctypes
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    import ctypes
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def sequences(x, mode, S, N):
    """x [B, S N, 96] -> [B, G, L, 96] in the kernels' sequence order"""
    v = x.reshape(x.shape[0], S, N, 96)
    return v if mode == SPATIAL else v.transpose(1, 2)


def maps_f64(x, ln_g, ln_b, wqkv, heads, mode, S, N):
    """float64 reference [B, G, heads, L, L] on CPU tensors"""
    seq = sequences(x.double(), mode, S, N)
    B, G, L, _ = seq.shape
    xn = F.layer_norm(seq, (96,), ln_g.double(), ln_b.double(), 1e-5)
    w = wqkv.double()
    q = (xn @ w[:heads * 64].t()).reshape(B, G, L, heads, 64).permute(0, 1, 3, 2, 4)
    k = (xn @ w[heads * 64:2 * heads * 64].t()).reshape(B, G, L, heads, 64).permute(0, 1, 3, 2, 4)
    return torch.softmax(q @ k.transpose(-1, -2) * 64 ** -0.5, dim=-1)


def run_kernel(x, ln_g, ln_b, wqkv, heads, mode, S, N, reduce, gap=0):
    """msst_attn_maps on device tensors -> the whole NaN-prefilled buffer [B, sample floats + gap]"""
    from maskedsst_amd import _lib
    lib = _lib.load()
    B = x.shape[0]
    L, G = (N, S) if mode == SPATIAL else (S, N)
    per = (G if reduce == PER_SEQ else 1) * heads * L * L
    out = torch.full((B, per + gap), float("nan"), device="cuda")
    rc = lib.msst_attn_maps(_p(x), _p(ln_g), _p(ln_b), _p(wqkv), _p(out), per + gap, mode, B, S, N, heads, reduce, _stream())
    assert rc == 0, lib.msst_last_error()
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def kernel_case(mode, S, N, B, heads):
    """seeded inputs (CPU) and the float64 reference of one kernel case, computed once"""
    g = torch.Generator().manual_seed(1000 * mode + 100 * S + N + 7 * B + heads)
    T = S * N
    x = torch.randn(B, T, 96, generator=g) * (0.5 + 1.5 * torch.rand(B, T, 1, generator=g)) + torch.randn(B, T, 1, generator=g)
    ln_g = 0.5 + torch.rand(96, generator=g)
    ln_b = 0.4 * torch.rand(96, generator=g) - 0.2
    wqkv = 0.15 * torch.randn(3 * heads * 64, 96, generator=g)
    return x, ln_g, ln_b, wqkv, maps_f64(x, ln_g, ln_b, wqkv, heads, mode, S, N)


# (mode, S, N, B, heads): the issue's cases -- spectral as (S, N, B, heads), spatial as (N, S, B, heads)
KERNEL_CASES = [(SPECTRAL, 1, 64, 2, 2), (SPECTRAL, 3, 36, 1, 2), (SPECTRAL, 5, 64, 2, 8), (SPECTRAL, 7, 16, 3, 3),
                (SPECTRAL, 20, 64, 1, 8), (SPECTRAL, 64, 4, 2, 2),
                (SPATIAL, 2, 64, 2, 8), (SPATIAL, 7, 16, 3, 2), (SPATIAL, 3, 36, 1, 2), (SPATIAL, 5, 49, 2, 8), (SPATIAL, 3, 25, 1, 3)]


# ------------------------------------------------------------------------------------------------- 1. the kernel alone against float64
@pytest.mark.parametrize("mode,S,N,B,heads", KERNEL_CASES, ids=lambda v: str(v))
def test_kernel_against_float64(mode, S, N, B, heads):
    x, ln_g, ln_b, wqkv, ref = kernel_case(mode, S, N, B, heads)
    L, G = (N, S) if mode == SPATIAL else (S, N)
    rowmax = float(ref.max(dim=-1).values.mean())
    if L >= 5:
        assert rowmax >= 0.3, rowmax          # peaky rows: a wrong softmax scale would be seen
    dev = [t.cuda().contiguous() for t in (x, ln_g, ln_b, wqkv)]
    gap = 12 if (mode, S, N) == (SPECTRAL, 3, 36) else 0       # one case: sample_stride beyond the sample, the gap keeps its NaN
    per = run_kernel(*dev, heads, mode, S, N, PER_SEQ, gap=gap).cpu()
    mean = run_kernel(*dev, heads, mode, S, N, MEAN_SEQ, gap=gap).cpu()
    if gap:
        assert torch.isnan(per[:, -gap:]).all() and torch.isnan(mean[:, -gap:]).all()
        per, mean = per[:, :-gap], mean[:, :-gap]
    per = per.reshape(B, G, heads, L, L)
    mean = mean.reshape(B, heads, L, L)
    assert torch.isfinite(per).all() and torch.isfinite(mean).all()
    err = float((per.double() - ref).abs().max())
    err_mean = float((mean.double() - ref.mean(dim=1)).abs().max())
    row = float((per.double().sum(dim=-1) - 1.0).abs().max())
    fold = float((mean.double() - per.double().mean(dim=1)).abs().max())
    print(f"attn_maps kernel mode {mode} S {S} N {N} B {B} heads {heads}: err {err:.3e} mean err {err_mean:.3e} row sum {row:.3e} "
          f"fold {fold:.3e} row max {rowmax:.3f}")
    assert err <= 1e-4 and err_mean <= 1e-4, (err, err_mean)
    assert row <= 128 * EPS, row
    assert fold <= (G + 1) * EPS, (fold, (G + 1) * EPS)
    if L == 1:
        assert torch.equal(per, torch.ones_like(per)) and torch.equal(mean, torch.ones_like(mean))   # every probability is exactly 1.0
    record("attn_maps_kernel", mode=mode, S=S, N=N, B=B, heads=heads, worst_abs=err, mean_worst_abs=err_mean)


# ------------------------------------------------------------------------------------------ 2. determinism and batch independence
@pytest.mark.parametrize("S,N,heads", [(3, 36, 2), (20, 64, 8)])
@pytest.mark.parametrize("mode", [SPATIAL, SPECTRAL])
def test_kernel_is_deterministic_and_batch_independent(mode, S, N, heads):
    g = torch.Generator().manual_seed(31 + S + mode)
    x = torch.randn(3, S * N, 96, generator=g).cuda()
    ln_g, ln_b = (0.5 + torch.rand(96, generator=g)).cuda(), (0.2 * torch.randn(96, generator=g)).cuda()
    wqkv = (0.15 * torch.randn(3 * heads * 64, 96, generator=g)).cuda()
    for reduce in (PER_SEQ, MEAN_SEQ):
        a = run_kernel(x, ln_g, ln_b, wqkv, heads, mode, S, N, reduce)
        b = run_kernel(x, ln_g, ln_b, wqkv, heads, mode, S, N, reduce)
        assert torch.isfinite(a).all() and torch.equal(a, b)                                 # two calls: the same bits
        for k in range(3):
            alone = run_kernel(x[k:k + 1].clone(), ln_g, ln_b, wqkv, heads, mode, S, N, reduce)
            assert torch.equal(alone[0], a[k]), (reduce, k)                                  # whatever batch, whatever index
        swapped = run_kernel(x.flip(0).contiguous(), ln_g, ln_b, wqkv, heads, mode, S, N, reduce)
        assert torch.equal(swapped.flip(0), a)


# ------------------------------------------------------------------------------------------------------ 3 / 4. through the model
MODEL_CASES = [dict(bands=50, depth=2, B=4, spectral_pos_embed=True),                      # simmim_50b_L2_B4_specpos
               dict(bands=30, depth=1, B=2, image_size=6, mask_patch_size=2, heads=2),     # simmim_30b_L1_B2_img6_mps2_h2
               dict(bands=70, depth=1, B=3, image_size=4, mask_patch_size=2),              # simmim_70b_L1_B3_img4_mps2
               dict(bands=50, depth=2, B=4, qkv_scale=4)]                                  # peaky: to_qkv.weight x 4 on a depth-2 model
_ids = lambda c: "-".join(f"{k}{v}" for k, v in c.items())   # noqa: E731


def block_maps_f64(params, pre, heads, xin):
    """float64 softmax of one block of the oracle's parameter dict on its input xin [sequences, L, 96] -> [sequences, heads, L, L]"""
    xn = F.layer_norm(xin.double(), (96,), params[pre + "0.norm.weight"].double(), params[pre + "0.norm.bias"].double(), 1e-5)
    w = params[pre + "0.fn.to_qkv.weight"].double()
    n, L = xin.shape[0], xin.shape[1]
    q = (xn @ w[:heads * 64].t()).reshape(n, L, heads, 64).transpose(1, 2)
    k = (xn @ w[heads * 64:2 * heads * 64].t()).reshape(n, L, heads, 64).transpose(1, 2)
    return torch.softmax(q @ k.transpose(-1, -2) * 64 ** -0.5, dim=-1)


def oracle_maps(params, tokens, ocfg):
    """the loop of oracle.transformer_forward restated with oracle.block, keeping every block's input -> (spatial [B, depth, S, heads,
    N, N], spectral [B, depth, N, heads, S, S]) float64"""
    from oracle.model import block
    B = tokens.shape[0]
    S, N, D, H = ocfg.S, ocfg.N, ocfg.dim, ocfg.heads
    p = params
    sp, sc = [], []
    x = tokens.reshape(B * S, N, D)
    for l in range(ocfg.depth):
        pre = f"encoder.spatial_spectral_transformer.1.layers.{l}."
        sp.append(block_maps_f64(p, pre, H, x).reshape(B, S, H, N, N))
        x = block(x, p, pre, H)
    x = x.reshape(B, S, N, D).transpose(1, 2).reshape(B * N, S, D)
    for l in range(ocfg.depth):
        pre = f"encoder.spatial_spectral_transformer.3.layers.{l}."
        sc.append(block_maps_f64(p, pre, H, x).reshape(B, N, H, S, S))
        x = block(x, p, pre, H)
    return torch.stack(sp, dim=1), torch.stack(sc, dim=1)


def oracle_tokens(params, x, ocfg, bool_mask=None):
    from oracle.model import encoder_embed, pos_table
    _, tok = encoder_embed(params, x, ocfg)
    pos = pos_table(params, ocfg)
    tokens = tok + pos
    if bool_mask is not None:
        tokens = torch.where(torch.as_tensor(bool_mask)[..., None], params["mask_token"][None, None, :] + pos, tokens)
    return tokens


@functools.lru_cache(maxsize=None)
def oracle_case(key, masked):
    """(params, x, masks, ocfg, spatial, spectral) of one model case from the CPU oracle in fp32 with a float64 softmax, computed once"""
    cfg = json.loads(key)
    model, params, x = build_product(cfg, precision="fp32", device="cpu")
    ocfg = oracle_cfg_from(cfg)
    masks = model.draw_masks(cfg["B"]) if masked else None
    with torch.no_grad():
        sp, sc = oracle_maps(params, oracle_tokens(params, x, ocfg, masks[0] if masked else None), ocfg)
    return params, x, masks, ocfg, sp, sc


def own_maps_f64(model, img, mask_u8=None):
    """float64 softmax of the model's OWN block inputs (Engine.blocks_fwd(save=False)) -> (spatial, spectral) as oracle_maps"""
    eng = model.engine()
    enc = model.encoder
    S, N, H = eng.S, eng.N, enc.heads
    with torch.no_grad():
        eng.prep_weights()
        acts, _ = eng.blocks_fwd(eng.tokenize(img, mask_u8), save=False)
        torch.cuda.synchronize()
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    B = img.shape[0]
    out = {"spatial": [], "spectral": []}
    for i, (sname, l) in enumerate(eng._layers()):
        xin = acts[i].cpu().reshape(B, S, N, 96)
        idx, (G, L) = (1, (S, N)) if sname == "spatial" else (3, (N, S))
        xin = (xin if sname == "spatial" else xin.transpose(1, 2)).reshape(B * G, L, 96)
        pre = f"encoder.spatial_spectral_transformer.{idx}.layers.{l}."
        out[sname].append(block_maps_f64(sd, pre, H, xin).reshape(B, G, H, L, L))
    return torch.stack(out["spatial"], dim=1), torch.stack(out["spectral"], dim=1)


@pytest.mark.parametrize("cfg", MODEL_CASES, ids=_ids)
def test_model_fp32_against_the_oracle(cfg):
    params, x, _, ocfg, ref_sp, ref_sc = oracle_case(json.dumps(cfg, sort_keys=True), False)
    model, _, x2 = build_product(cfg, precision="fp32", device="cuda")
    assert torch.equal(x, x2)
    enc = model.encoder
    img = x.cuda()
    full = enc.attention_maps(img, reduce=None)
    mean = enc.attention_maps(img)
    torch.cuda.synchronize()
    S, N, H, Ld, B = ocfg.S, ocfg.N, ocfg.heads, ocfg.depth, cfg["B"]
    assert tuple(full.spatial.shape) == (B, Ld, S, H, N, N) and tuple(full.spectral.shape) == (B, Ld, N, H, S, S)
    assert tuple(mean.spatial.shape) == (B, Ld, H, N, N) and tuple(mean.spectral.shape) == (B, Ld, H, S, S)
    assert full.spatial.dtype == full.spectral.dtype == mean.spatial.dtype == torch.float32 and not full.spatial.requires_grad
    e_sp = float((full.spatial.cpu().double() - ref_sp).abs().max())
    e_sc = float((full.spectral.cpu().double() - ref_sc).abs().max())
    print(f"attention_maps fp32 {cfg}: spatial {e_sp:.3e} spectral {e_sc:.3e}")
    assert e_sp <= 1e-4 and e_sc <= 1e-4, (e_sp, e_sc)
    # reduce="mean" is the mean of reduce=None over the sample's sequences
    for m, f, G in ((mean.spatial, full.spatial, S), (mean.spectral, full.spectral, N)):
        d = float((m.cpu().double() - f.cpu().double().mean(dim=2)).abs().max())
        assert d <= (G + 1) * EPS, (d, G)
    # blocks / stack select slices of the same bits; the other field is None
    last = Ld - 1
    one = enc.attention_maps(img, blocks=[last], reduce=None)
    assert torch.equal(one.spatial, full.spatial[:, last:last + 1]) and torch.equal(one.spectral, full.spectral[:, last:last + 1])
    only = enc.attention_maps(img, stack="spectral")
    assert only.spatial is None and torch.equal(only.spectral, mean.spectral)
    only = enc.attention_maps(img, stack="spatial", reduce=None, blocks=[0])
    assert only.spectral is None and torch.equal(only.spatial, full.spatial[:, :1])
    record("attention_maps_model", cfg=cfg, prec="fp32", spatial_worst_abs=e_sp, spectral_worst_abs=e_sc)


@pytest.mark.parametrize("cfg", MODEL_CASES, ids=_ids)
def test_model_bf16_against_its_own_block_inputs(cfg):
    _, x, _, ocfg, ora_sp, ora_sc = oracle_case(json.dumps(cfg, sort_keys=True), False)
    model, _, _ = build_product(cfg, precision="bf16", device="cuda")
    img = x.cuda()
    full = model.encoder.attention_maps(img, reduce=None)
    torch.cuda.synchronize()
    ref_sp, ref_sc = own_maps_f64(model, img)
    got_sp, got_sc = full.spatial.cpu().double(), full.spectral.cpu().double()
    e_sp, e_sc = float((got_sp - ref_sp).abs().max()), float((got_sc - ref_sc).abs().max())
    o_sp, o_sc = float((got_sp - ora_sp).abs().max()), float((got_sc - ora_sc).abs().max())
    print(f"attention_maps bf16 {cfg}: spatial {e_sp:.3e} spectral {e_sc:.3e}; to the fp32 oracle's maps {o_sp:.3e} {o_sc:.3e}")
    assert e_sp <= 1e-4 and e_sc <= 1e-4, (e_sp, e_sc)      # the maps kernel is fp32 given x
    record("attention_maps_model", cfg=cfg, prec="bf16", spatial_worst_abs=e_sp, spectral_worst_abs=e_sc,
           spatial_to_oracle=o_sp, spectral_to_oracle=o_sc)


# ---------------------------------------------------------------------------------------------------------- 5. the SimMIM wrapper
def test_simmim_wrapper_masks_mode_and_grads():
    cfg = MODEL_CASES[0]
    params, x, masks, ocfg, ref_sp, ref_sc = oracle_case(json.dumps(cfg, sort_keys=True), True)
    model, _, _ = build_product(cfg, precision="fp32", device="cuda")
    img = x.cuda()
    for p in model.parameters():
        p.grad = torch.full_like(p, 0.25)
    grads = [p.grad for p in model.parameters()]
    model.train()
    got = model.attention_maps(img, masks=masks, reduce=None)
    assert model.training and model.encoder.training
    # the same float64 check as the encoder path: the oracle with the mask token substituted ...
    e_sp = float((got.spatial.cpu().double() - ref_sp).abs().max())
    e_sc = float((got.spectral.cpu().double() - ref_sc).abs().max())
    assert e_sp <= 1e-4 and e_sc <= 1e-4, (e_sp, e_sc)
    # ... and the encoder run on the tokens Engine.tokenize gives for that mask
    mask_u8 = torch.as_tensor(masks[0]).to(device="cuda", dtype=torch.uint8).contiguous()
    own_sp, own_sc = own_maps_f64(model, img, mask_u8)
    assert float((got.spatial.cpu().double() - own_sp).abs().max()) <= 1e-4
    assert float((got.spectral.cpu().double() - own_sc).abs().max()) <= 1e-4
    bare_bool = model.attention_maps(img, masks=torch.as_tensor(masks[0]), reduce=None)      # the bare bool mask: the same bits
    assert torch.equal(bare_bool.spatial, got.spatial) and torch.equal(bare_bool.spectral, got.spectral)
    # masks=None: the bare encoder's maps, bit for bit; the mask matters
    none = model.attention_maps(img, reduce=None)
    enc = model.encoder.attention_maps(img, reduce=None)
    assert torch.equal(none.spatial, enc.spatial) and torch.equal(none.spectral, enc.spectral)
    assert not torch.equal(none.spatial, got.spatial)
    # the module's mode leaves every bit and is left as found
    model.eval()
    ev = model.attention_maps(img, masks=masks, reduce=None)
    assert not model.training and not model.encoder.training
    assert torch.equal(ev.spatial, got.spatial) and torch.equal(ev.spectral, got.spectral)
    assert not got.spatial.requires_grad and got.spatial.grad_fn is None
    for p, g in zip(model.parameters(), grads):
        assert p.grad is g and torch.equal(g, torch.full_like(g, 0.25))
    record("attention_maps_simmim", cfg=cfg, prec="fp32", spatial_worst_abs=e_sp, spectral_worst_abs=e_sc)


# ------------------------------------------------------------------------------------------------------------------------ 6. scripts
def child(cmd, timeout):
    """a script in a fresh child process under its own time limit.  A child that timed out or died of a signal (a GPU fault, an abort)
    ends the session: nothing more is started on the device after it."""
    e = dict(os.environ)
    e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
    try:
        r = subprocess.run(cmd, cwd=ROOT, env=e, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as t:
        pytest.exit(f"{' '.join(cmd)} timed out after {timeout} s: no further GPU work\n{(t.stderr or '')[-2000:]}", returncode=1)
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        pytest.exit(f"{' '.join(cmd)} ended with {r.returncode}: no further GPU work\n{r.stderr[-3000:]}", returncode=1)
    assert r.returncode == 0, f"--- stdout\n{r.stdout[-3000:]}\n--- stderr\n{r.stderr[-3000:]}"
    return r.stdout


def test_attn_maps_time_script(tmp_path):
    """tools/attn_maps_time.py --quick: exit 0, ONE JSON line with the three legs' times, the same line appended to --append"""
    log = str(tmp_path / "t.jsonl")
    out = child([sys.executable, os.path.join("tools", "attn_maps_time.py"), "--quick", "--append", log], 300)
    lines = [l for l in out.splitlines() if l.strip()]
    assert len(lines) == 1, out
    row = json.loads(lines[0])
    assert [json.loads(l) for l in open(log)] == [row]
    assert row["tool"] == "attn_maps_time" and row["bands"] == 50 and row["depth"] == 1
    assert [r["batch"] for r in row["results"]] == [4]
    for r in row["results"]:
        assert len(r["attention_maps_ms"]) == len(r["eager_ms"]) == len(r["forward_ms"]) == 2
        assert all(v > 0 for v in r["attention_maps_ms"] + r["eager_ms"] + r["forward_ms"])
        assert all(r["kernel_ms"][s][k] > 0 for s in ("spatial", "spectral") for k in ("mean", "per_seq"))
        assert r["max_abs_diff"] < 1e-4, r      # an fp32 eager restatement on the same block inputs


def test_finetune_val_attention_script():
    """finetune.py --val-attention: one more line per validation pass, after the 'val step' line"""
    out = child([sys.executable, "finetune.py", "--steps", "2", "--val-scenes", "2", "--val-every", "1", "--val-attention"], 600)
    lines = out.splitlines()
    att = [l.split() for l in lines if l.startswith("val-attention step ")]
    assert [a[2] for a in att] == ["1", "2"], out
    assert len([l for l in lines if l.startswith("val step ")]) == 2
    for a in att:
        assert a[3:6] == ["top", "spectral", "blocks"] and a[9:] == ["windows", "128"], a
        blocks = [int(t.split(":")[0]) for t in a[6:9]]
        scores = [float(t.split(":")[1]) for t in a[6:9]]
        assert len(set(blocks)) == 3 and all(0 <= b < 20 for b in blocks)
        assert scores == sorted(scores, reverse=True) and all(0.0 < s < 1.0 for s in scores)
