"""Shared helpers for the parity tests: build the product model and the oracle parameters from
the same seed (parameters are drawn on the CPU in the reference order, then moved to the GPU)."""
import json
import os

import numpy as np
import torch

from conftest import ROOT, seed_all, oracle_cfg_from, apply_qkv_scale


def build_product(cfg, precision="fp32", device="cpu"):
    """cfg key spectral_patch: the spectral patch depth P (default 10, the shipped band_patch_size)"""
    from maskedsst_amd import ViTSpatialSpectral, SimMIMSpatialSpectral
    seed_all(5)
    P = cfg.get("spectral_patch", 10)
    enc = ViTSpatialSpectral(
        image_size=cfg.get("image_size", 8), spatial_patch_size=1, spectral_patch_size=P, num_classes=cfg.get("n_classes", 8),
        dim=96, depth=cfg["depth"], heads=cfg.get("heads", 8), mlp_dim=64, dropout=0.0, emb_dropout=0.0,
        channels=cfg["bands"], spectral_pos_embed=cfg.get("spectral_pos_embed", False),
        spectral_pos=torch.arange(cfg["bands"] // P), blockwise_patch_embed=True, spectral_only=False,
        precision=precision)
    model = SimMIMSpatialSpectral(
        encoder=enc, intermediate_losses=False, masking_ratio=cfg.get("masking_ratio", 0.7),
        mask_patch_size=cfg.get("mask_patch_size", 4),
        to_pixels_per_spectral_block=cfg.get("to_pixels_per_spectral_block", True),
        tube_masking=cfg.get("tube_masking", True))
    apply_qkv_scale(model.named_parameters(), cfg)
    x = torch.randn(cfg["B"], cfg["bands"], cfg.get("image_size", 8), cfg.get("image_size", 8))
    if cfg.get("zero_pad_bands"):
        x[:, cfg["bands"] - cfg["zero_pad_bands"]:] = 0.0
    params = {k: v.detach().clone() for k, v in model.state_dict().items()}
    if device != "cpu":
        model = model.to(device)
    return model, params, x


def oracle_cfg(cfg):
    """conftest.oracle_cfg_from plus the spectral patch depth (cfg key spectral_patch, default 10)"""
    import dataclasses
    return dataclasses.replace(oracle_cfg_from(cfg), spectral_patch=cfg.get("spectral_patch", 10))


# ---- the three classifier heads on encoder tokens y [B, S N, 96] (token order c h w), in plain PyTorch: float64 references ----
def cls_head_ref(y, ln_g, ln_b, w, b, S, N):
    """default head (reference vit_spatial_spectral.py:481-493, :536-564): mean over c -> LayerNorm(96) -> Linear -> [B, nc, N]"""
    B = y.shape[0]
    x = torch.nn.functional.layer_norm(y.reshape(B, S, N, 96).mean(dim=1), (96,), ln_g, ln_b, 1e-5)
    return torch.moveaxis(x @ w.t() + b, -1, 1)


def spectral_head_ref(y, ln_g, ln_b, w, b, S, Nsq):
    """the spectral MLP head: 'b (c h w) d -> b h w (c d)' -> LayerNorm -> Linear -> [B, nc, H, W]"""
    B = y.shape[0]
    x = y.reshape(B, S, Nsq, Nsq, 96).permute(0, 2, 3, 1, 4).reshape(B, Nsq, Nsq, S * 96)
    x = torch.nn.functional.layer_norm(x, (S * 96,), ln_g, ln_b, 1e-5)
    return torch.moveaxis(x @ w.t() + b, -1, 1)


def pix_head_ref(y, ln_g, ln_b, w, b, S, N):
    """the pixelwise head: mean over c -> LayerNorm(96) per position -> flatten (n, d) -> Linear -> [B, nc]"""
    B = y.shape[0]
    x = y.reshape(B, S, N, 96).mean(dim=1)
    x = torch.nn.functional.layer_norm(x, (96,), ln_g, ln_b, 1e-5)
    return x.reshape(B, N * 96) @ w.t() + b


# ---- the role-split forward's saved softmax statistics (include/msst.h: msst_block_fwd, lse_out) and their float64 restatement ----
def ln1_rows_as_used(x, ln_g, ln_b, x1, half):
    """LN1 rows [tokens, 96] as the role-split forward multiplied them, and their element type: IEEE half of LN1(x) computed in fp32
    (MSST_FWD_HALF), else the bf16 rows the forward saved with x1 (x1._msst_xn)"""
    if half:
        xn = torch.nn.functional.layer_norm(x.float().reshape(-1, 96), (96,), ln_g, ln_b, 1e-5)
        return xn.to(torch.float16).float(), torch.float16
    return x1._msst_xn.float().reshape(-1, 96), torch.bfloat16


def lse_restatement(xn, wqkv, heads, low, scores=False):
    """xn [sequences, L, 96]: LN1 rows as used (ln1_rows_as_used, in sequence layout); wqkv [3 heads 64, 96] fp32 -> [sequences, heads, L]
    lse = log2 of every query's softmax denominator in the kernels' exponent domain (s = q k * dim_head^-0.5 * log2 e), q and k
    rounded to `low` as the forward rounds them, the rest in float64.  scores=True: -> (lse, the largest |s|)"""
    wq = wqkv.to(low).float()
    qkv = (xn @ wq.t()).to(low).double()
    n, L = xn.shape[0], xn.shape[1]
    q, k = qkv[..., :heads * 64].reshape(n, L, heads, 64), qkv[..., heads * 64:2 * heads * 64].reshape(n, L, heads, 64)
    s = torch.einsum("bnhd,bmhd->bhnm", q, k) * (0.125 * 1.4426950408889634)
    lse = torch.logsumexp(s * 0.6931471805599453, dim=-1) * 1.4426950408889634
    return (lse, float(s.abs().max())) if scores else lse


def saved_lse_rows(lse, heads, L, nseq):
    """the statistics buffer [tiles][heads][64] lse | [tokens] rstd of LN1 -> (lse [sequences, heads, L] without the padding rows of
    each tile (64 // L whole sequences per tile), rstd [tokens])"""
    TS = 64 // L
    ntiles = -(-nseq // TS)
    got = lse[:ntiles * heads * 64].reshape(ntiles, heads, 64)[:, :, :TS * L].reshape(ntiles, heads, TS, L).permute(0, 2, 1, 3)
    return got.reshape(ntiles * TS, heads, L)[:nseq], lse[ntiles * heads * 64:]


def host_fold(win, Bs, Hs, Ws, w, stride, dtype=torch.float64):
    """fold of win [Bs nr nq, D, w w] (window order) into scene planes, the running sums in `dtype`: (sum, sum of |terms|, cover
    [Bs, Hs, Ws] int32).  float64: the reference of the error bounds.  float32: every pixel's sum takes its covering windows in the
    order of the scene kernels (window row, then column), one rounded addition each -- their bits."""
    from maskedsst_amd.scene import scene_windows
    D = win.shape[1]
    org = scene_windows(Hs, Ws, w, stride)
    acc = torch.zeros(Bs, D, Hs, Ws, dtype=dtype)
    mag = torch.zeros(Bs, D, Hs, Ws, dtype=dtype)
    cover = torch.zeros(Bs, Hs, Ws, dtype=torch.int32)
    i = 0
    for s in range(Bs):
        for (y, x) in org:
            v = win[i].to(dtype).view(D, w, w)
            acc[s, :, y:y + w, x:x + w] += v
            mag[s, :, y:y + w, x:x + w] += v.abs()
            cover[s, y:y + w, x:x + w] += 1
            i += 1
    assert i == win.shape[0]
    return acc, mag, cover


def relerr(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def rel_l2(a, b):
    a = a.detach().double().cpu().reshape(-1)
    b = b.detach().double().cpu().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-30))


# ---- two assertion tiers for the bf16 kernels ----
# hard tier: the bars written in the tests (3-4x the error measured on the device: they survive compiler / clock / box changes);
# strict tier, MSST_STRICT_PARITY=1 (tools/final_prof.sh and __graft_entry__.smoke() set it): every error a test records must
# also stay within STRICT_FACTOR x the value the SAME test recorded in the pinned baseline (_baseline(): round 5's committed file, later
# rounds only for measurements that round did not have; or $MSST_PARITY_BASELINE), so that a 2x regression of a gradient error is seen by the builder before the driver's run.
STRICT_FACTOR = 1.5
_ERR_KEY = ("err", "dx", "worst_grad", "stage_l2", "one_minus_cos", "worst_slice", "worst_abs", "rel_dev")
_baseline_rows = None


def _is_err_key(k):
    return k != "worst_grad_name" and any(t in k for t in _ERR_KEY)


STRICT_PIN = "r05"   # the round whose measurements are the strict tier's baseline


def _baseline():
    """The strict tier's baseline rows: profiles/r05_parity_measured.jsonl (pinned -- ADVICE r5: against "the newest file" a 1.5x drift
    per round would compound, and a rerun inside a round would compare with itself), plus, for measurements that did not exist in that
    round (new tests, new configurations), the row of the FIRST later round that recorded them.  $MSST_PARITY_BASELINE: that file alone."""
    global _baseline_rows
    if _baseline_rows is None:
        import glob
        one = os.environ.get("MSST_PARITY_BASELINE")
        paths = [one] if one else [p for p in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_parity_measured.jsonl")))
                                   if os.path.basename(p)[:3] >= STRICT_PIN]
        rows, seen = [], set()
        for p in paths:
            if not os.path.exists(p):
                continue
            here = [json.loads(l) for l in open(p) if l.strip()]
            keys = [json.dumps(_identity(r), sort_keys=True) for r in here]
            rows += [r for r, k in zip(here, keys) if k not in seen]     # a round's own repeats of one identity stay together (the last one counts)
            seen |= set(keys)
        _baseline_rows = rows
    return _baseline_rows


def _identity(row):
    """the fields that say WHICH measurement a row is (configuration, kernel, fixture ...): everything that is not a float"""
    return {k: v for k, v in row.items() if not isinstance(v, float) and not (isinstance(v, dict) and k != "cfg") and k not in ("worst_grad_name", "worst")}


# comparisons of two summation orders of the SAME arithmetic: their size is decided by whether a last-bit difference flips a bf16
# rounding somewhere (1e-7 for one input, 1e-4 for the next): not a measurement a ratio can be held against
STRICT_EXEMPT = {"chained_backward_matches_unchained", "attn_bwd_kernels_agree"}
# ... and the variant-vs-variant halves of tests that ALSO record errors against the oracle (those stay in the tier)
STRICT_EXEMPT_KEYS = {"saved_softmax_statistics": {"dx", "worst_grad", "lse_abs_err"}, "ln1_backward_from_saved_rows": {"dx", "worst_grad"}}


def strict_violations(test, kv, factor=STRICT_FACTOR, floor=1e-6, unmatched=None):
    """[(key, measured, baseline)] of the recorded errors that exceed factor x the baseline row of the same test and identity.
    No such row: nothing to compare with -> [] (and `unmatched`, a list, gets the test's name: record() warns)."""
    if test in STRICT_EXEMPT:
        return []
    ident = json.loads(json.dumps(_identity(dict(test=test, **kv))))
    rows = [r for r in _baseline() if json.loads(json.dumps(_identity(r))) == ident]
    if not rows:
        if unmatched is not None:
            unmatched.append(test)
        return []
    base = rows[-1]
    bad = []

    def cmp(key, got, ref):
        if isinstance(got, dict) and isinstance(ref, dict):
            for k in got:
                if k in ref:
                    cmp(f"{key}.{k}", got[k], ref[k])
        elif isinstance(got, (list, tuple)) and isinstance(ref, (list, tuple)) and len(got) == len(ref):
            for i, (g, r) in enumerate(zip(got, ref)):
                cmp(f"{key}[{i}]", g, r)
        elif isinstance(got, float) and isinstance(ref, float):
            if abs(got) > factor * abs(ref) + floor:
                bad.append((key, got, ref))

    for k, v in kv.items():
        if k not in base or k in STRICT_EXEMPT_KEYS.get(test, ()):
            continue
        if k == "cos" and isinstance(v, float):
            cmp("1-cos", 1.0 - v, 1.0 - base[k])
        elif _is_err_key(k):
            cmp(k, v, base[k])
    return bad


def record(test, **kv):
    """Every parity test hands its measured errors here AFTER its hard-tier assertions.
    MSST_STRICT_PARITY=1: the strict tier (above) is asserted.
    MSST_RECORD=1 (tools/final_prof.sh sets it): the row is appended to gpurun_out/parity_$MSST_ROUND.jsonl (scratch; the
    round's copy lives in profiles/).  Ordinary test runs write nothing."""
    if os.environ.get("MSST_RECORD") == "1":
        try:
            d = os.path.join(ROOT, "gpurun_out")
            os.makedirs(d, exist_ok=True)
            with open(os.path.join(d, "parity_%s.jsonl" % os.environ.get("MSST_ROUND", "dev")), "a") as f:
                f.write(json.dumps(dict(test=test, **kv)) + "\n")
        except OSError:
            pass
    if os.environ.get("MSST_STRICT_PARITY") == "1":
        unmatched = []
        bad = strict_violations(test, kv, unmatched=unmatched)
        if unmatched:   # a renamed / new test or a changed cfg has no committed row: it passes the strict tier UNCHECKED -- say so
            import warnings
            warnings.warn(f"strict parity tier: no committed baseline row matches {test} {_identity(kv)} -- not checked")
        assert not bad, f"strict parity tier ({STRICT_FACTOR}x the committed baseline) tripped in {test}: " + \
            ", ".join(f"{k} = {g:.3e} (baseline {r:.3e})" for k, g, r in bad)
