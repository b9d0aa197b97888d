"""Tokenizer and SimMIM head restatements, host side (no GPU needed): tests/tok_head_util.py, the float64 reference of
tests/test_gpu_tok_head_kernels.py, is itself checked here -- composed into the non-block parts of the SimMIM step against the oracle,
head_bwd_ref against autograd of head_ref, and per case the two conditions that keep the GPU tests' bars honest (fp32 autograd of the
restatement within BAR / MARGIN of float64; at most BAND_SHARE of the dpred elements inside the excluded band) and the promised content
of the index rows."""
import numpy as np
import pytest
import torch

from util import relerr, rel_l2
from tok_head_util import (BAR, MARGIN, BAND, BAND_SHARE, GOUT, TOK_CASES, HEAD_CASES, TOK_GRADS, tok_inputs, tok_grads_ref, tok_autograd,
                           tokenizer_ref, synthetic_keep, head_inputs, head_fwd_ref, head_grads_ref, head_ref, head_bwd_ref, index_rows)

# two small configurations of the oracle: learned position table with per-block to_pixels, split (sincos) tables with a shared to_pixels
ORACLE_CASES = [
    dict(name="learned_per_block", bands=20, P=10, image_size=4, B=3, spectral_pos_embed=False, per_block=True),
    dict(name="split_shared", bands=15, P=5, image_size=3, B=2, spectral_pos_embed=True, per_block=False),
]


def _oracle_step(case):
    from oracle import OracleConfig, simmim_forward
    from oracle.model import init_params
    cfg = OracleConfig(bands=case["bands"], image_size=case["image_size"], spectral_patch=case["P"], depth=1, heads=2,
                       spectral_pos_embed=case["spectral_pos_embed"], masking_ratio=0.5, to_pixels_per_spectral_block=case["per_block"])
    torch.manual_seed(11)
    params = init_params(cfg)
    gen = torch.Generator().manual_seed(12)
    for k, v in params.items():   # away from the init values (LayerNorm vectors of ones / zeros), the sincos tables included
        if "norm" in k or "embed" in k and "blockwise" not in k:
            v.add_(0.2 * torch.randn(v.shape, generator=gen))
    params = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    B = case["B"]
    img = torch.randn(B, cfg.bands, cfg.Nsq, cfg.Nsq, generator=gen) * 1.5 + 0.3
    bool_mask = torch.rand(B, cfg.T, generator=gen) < 0.5
    idx = index_rows(B, cfg.K, cfg.T, gen)
    st = simmim_forward(params, img, cfg, masks=(bool_mask, idx))
    st["tok_masked"].retain_grad()
    st["enc_out"].retain_grad()
    st["loss"].backward()
    return cfg, params, img, bool_mask, idx, st


@pytest.mark.parametrize("case", ORACLE_CASES, ids=[c["name"] for c in ORACLE_CASES])
def test_restatements_compose_into_the_oracle_step(case):
    """forward stages tok_masked, pred, loss and the oracle's autograd gradients of the tokenizer, position, mask-token and to_pixels
    parameters, the encoder blocks bypassed by feeding the oracle's own enc_out and its gradient: 1e-5, the bar of
    test_oracle_img_grad_matches_the_reference (fp32 oracle against a float64 restatement)"""
    cfg, params, img, bool_mask, idx, st = _oracle_step(case)
    B, S, N, P, K = img.shape[0], cfg.S, cfg.N, cfg.P, cfg.K
    d = lambda k: params[k].detach().double()   # noqa: E731
    pe = "encoder.to_patch_embedding."
    q = dict(pre_g=d(pe + "pre_norm.weight"), pre_b=d(pe + "pre_norm.bias"), post_g=d(pe + "post_norm.weight"), post_b=d(pe + "post_norm.bias"),
             w=torch.stack([d(pe + f"blockwise_embed.{i}.weight") for i in range(S)]),
             b=torch.stack([d(pe + f"blockwise_embed.{i}.bias") for i in range(S)]), mask_token=d("mask_token"))
    if case["spectral_pos_embed"]:
        pos = (d("encoder.pos_embed")[0], d("encoder.channel_embed")[0])
        assert pos[0].shape == (N, 64) and pos[1].shape == (S, 32)
    else:
        pos = d("encoder.pos_embedding")[0, :S * N]
    if case["per_block"]:
        w_pix = torch.stack([d(f"to_pixels.layers.{i}.weight") for i in range(S)])
        b_pix = torch.stack([d(f"to_pixels.layers.{i}.bias") for i in range(S)])
    else:
        w_pix, b_pix = d("to_pixels.weight")[None], d("to_pixels.bias")[None]
    img3 = img.double().reshape(B, S * P, N)
    # forward
    assert relerr(tokenizer_ref(img3, q, bool_mask, pos, 1.0), st["tok_masked"]) <= 1e-5
    y = st["enc_out"].detach().double()
    pred, target, loss = head_ref(y, img3, idx, w_pix, b_pix, case["per_block"])
    assert relerr(pred, st["pred"]) <= 1e-5 and relerr(target, st["target"]) == 0.0
    assert abs(float(loss) - float(st["loss"].detach())) <= 1e-5 * abs(float(st["loss"].detach()))
    # head backward on the oracle's sign pattern
    sign = torch.sign(st["pred"] - st["target"]).detach().double()
    dy, dw, db = head_bwd_ref(y, sign, idx, w_pix, case["per_block"], 1.0 / (B * K * P) / K, 1.0)
    errs = {"dy": relerr(dy, st["enc_out"].grad)}
    if case["per_block"]:
        want_w = torch.stack([params[f"to_pixels.layers.{i}.weight"].grad for i in range(S)])
        want_b = torch.stack([params[f"to_pixels.layers.{i}.bias"].grad for i in range(S)])
    else:
        want_w, want_b = params["to_pixels.weight"].grad[None], params["to_pixels.bias"].grad[None]
    errs["dw_pix"], errs["db_pix"] = relerr(dw, want_w), relerr(db, want_b)
    # tokenizer backward on the oracle's d(loss) / d(tok_masked)
    g = tok_autograd(q, pos, img3, bool_mask, st["tok_masked"].grad.double())
    want = dict(dpre_g=params[pe + "pre_norm.weight"].grad, dpre_b=params[pe + "pre_norm.bias"].grad,
                dpost_g=params[pe + "post_norm.weight"].grad, dpost_b=params[pe + "post_norm.bias"].grad,
                dw_emb=torch.stack([params[pe + f"blockwise_embed.{i}.weight"].grad for i in range(S)]),
                db_emb=torch.stack([params[pe + f"blockwise_embed.{i}.bias"].grad for i in range(S)]), dmask_token=params["mask_token"].grad)
    if case["spectral_pos_embed"]:
        want["dpos_a"], want["dpos_b"] = params["encoder.pos_embed"].grad[0], params["encoder.channel_embed"].grad[0]
    else:
        full = params["encoder.pos_embedding"].grad[0]
        want["dpos_a"] = full[:S * N]
        assert float(full[S * N:].abs().max()) == 0.0   # the class-token row takes no part
    for k, v in want.items():
        assert float(v.abs().max()) > 0, k
        errs[k] = relerr(g[k], v)
    print(case["name"], {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= 1e-5, errs


@pytest.mark.parametrize("case", HEAD_CASES, ids=[c["name"] for c in HEAD_CASES])
def test_head_bwd_ref_is_the_autograd_of_head_ref(case):
    """float64 both sides, <= 1e-12; the index rows hold duplicates (index_rows), which autograd sums through the gather"""
    x = head_inputs(case["name"])
    y, w, b = (x[k].clone().requires_grad_(True) for k in ("y", "w_pix", "b_pix"))
    pred, target, loss = head_ref(y, x["img"], x["idx"], w, b, case["per_block"])
    loss.backward()
    dy, dw, db = head_bwd_ref(x["y"], torch.sign(pred - target).detach(), x["idx"], x["w_pix"], case["per_block"], x["gscale"], 1.0)
    assert relerr(dy, y.grad) <= 1e-12 and relerr(dw, w.grad) <= 1e-12 and relerr(db, b.grad) <= 1e-12
    # ... and is linear in (dpred, gout): the form the GPU test feeds it
    dy2, dw2, db2 = head_grads_ref(case["name"], GOUT)
    dy1, dw1, db1 = head_grads_ref(case["name"], 1.0)
    assert relerr(dy2, GOUT * dy1) <= 1e-12 and relerr(dw2, GOUT * dw1) <= 1e-12 and relerr(db2, GOUT * db1) <= 1e-12


@pytest.mark.parametrize("case", TOK_CASES, ids=[c["name"] for c in TOK_CASES])
def test_condition_tokenizer_gradients_fp32_autograd(case):
    """the condition of the GPU test's bar: plain fp32 autograd of the restatement stays within BAR / MARGIN of float64 for every
    compared tensor of the case (every mask, without and with a keep mask).  Tensors whose float64 value is identically zero are
    compared for exact zeros on the GPU, not by this bar"""
    worst = {}
    for mname in case["masks"]:
        for keep in [1.0] + ([synthetic_keep(case["name"])] if len(case["drops"]) > 1 else []):
            ref = tok_grads_ref(case["name"], mname, keep)
            got = tok_grads_ref(case["name"], mname, keep, dtype=torch.float32)
            for k in TOK_GRADS:
                if ref[k] is None or float(ref[k].abs().max()) == 0.0:
                    assert got[k] is None or float(got[k].abs().max()) == 0.0, (mname, k)
                    continue
                worst[k] = max(worst.get(k, 0.0), rel_l2(got[k], ref[k]))
    print(case["name"], {k: f"{v:.2e}" for k, v in worst.items()})
    assert set(worst) == {k for k in TOK_GRADS if k != "dpos_b" or case["split"]}
    assert max(worst.values()) <= BAR / MARGIN, worst


@pytest.mark.parametrize("case", HEAD_CASES, ids=[c["name"] for c in HEAD_CASES])
def test_condition_head_fp32_and_the_sign_band(case):
    """the two conditions of the head cases: fp32 autograd of sum(pred dpred) gscale gout within BAR / MARGIN of head_bwd_ref in float64
    (and fp32 pred, loss of float64), and at most BAND_SHARE of the dpred elements with |pred - target| < BAND"""
    x = head_inputs(case["name"])
    f = lambda k: x[k].float()   # noqa: E731
    y, w, b = (f(k).requires_grad_(True) for k in ("y", "w_pix", "b_pix"))
    pred32, _, loss32 = head_ref(y, f("img"), x["idx"], w, b, case["per_block"])
    (pred32 * f("dpred")).sum().mul(x["gscale"] * GOUT).backward()
    dy, dw, db = head_grads_ref(case["name"], GOUT)
    errs = dict(dy=rel_l2(y.grad, dy), dw_pix=rel_l2(w.grad, dw), db_pix=rel_l2(b.grad, db))
    pred, target, loss = head_fwd_ref(case["name"])
    errs["pred"] = rel_l2(pred32, pred)
    errs["loss"] = abs(float(loss32) - float(loss)) / abs(float(loss))
    share = float(((pred - target).abs() < BAND).double().mean())
    print(case["name"], {k: f"{v:.2e}" for k, v in errs.items()}, "band share", share, "max |pred32 - pred64|", float((pred32.double() - pred).abs().max()))
    assert max(errs.values()) <= BAR / MARGIN, errs
    assert share <= BAND_SHARE, share


@pytest.mark.parametrize("case", HEAD_CASES, ids=[c["name"] for c in HEAD_CASES])
def test_index_rows_hold_what_the_case_list_promises(case):
    """an unnamed token, a token named twice, a token named three or more times in a row other than the single-token row (K = 1: a row
    cannot name a token more often than once), the row that names one token K times, tokens 0 and S N - 1 in one row (K = 1: in two),
    and a CSR that lists exactly the positions of every token"""
    x = head_inputs(case["name"])
    B, K, T = case["B"], case["K"], case["S"] * case["N"]
    idx = x["idx"].numpy()
    assert idx.shape == (B, K) and idx.min() >= 0 and idx.max() < T
    counts = np.stack([np.bincount(r, minlength=T) for r in idx])
    assert (counts == 0).any(axis=1).all(), "every row leaves tokens unnamed"
    assert counts[0].max() == K and (counts[0] > 0).sum() == 1, "row 0 names a single token K times"
    assert counts[1:].max() >= min(3, K)
    if K >= 2:
        assert (counts[1:] == 2).any()
        assert counts[1, 0] > 0 and counts[1, T - 1] > 0
    else:
        assert counts[1, 0] > 0 and counts[2, T - 1] > 0
    ptr, pos = x["csr_ptr"].numpy(), x["csr_pos"].numpy()
    assert ptr.shape == (B, T + 1) and pos.shape == (B, K) and ptr.dtype == pos.dtype == np.int32
    for b in range(B):
        assert ptr[b, 0] == 0 and ptr[b, T] == K
        for t in np.unique(np.concatenate([idx[b], [0, T - 1]])):
            assert sorted(pos[b, ptr[b, t]:ptr[b, t + 1]]) == list(np.nonzero(idx[b] == t)[0])


def test_case_tables_reach_every_kernel_and_walk_length():
    """the kernel column is what the launchers select (msst_bwd.hip: launch_tokenize_bwd, launch_head_bwd), nchunk <= B throughout, and
    the walks occur that the tables are there for: per kernel a ragged end (B % nchunk != 0) and several walk lengths, one of them
    above 4 samples (the head backward keeps four CSR stages in flight); for the two pipelined kernels also walks of 1, 2 and 3"""
    for c in TOK_CASES:
        want = "mfma" if (c["P"], c["N"]) == (10, 64) else "<10>" if c["P"] == 10 else "<0>"
        assert c["kernel"] == want and c["P"] > 2 and all(1 <= n <= c["B"] for n in c["nchunks"]), c["name"]
        assert tok_inputs(c["name"])["masks"]["random"].any() and not tok_inputs(c["name"])["masks"]["random"].all()
    for c in HEAD_CASES:
        assert c["kernel"] == ("mfma" if (c["P"], c["N"]) == (10, 64) else "generic") and all(1 <= n <= c["B"] for n in c["nchunks"]), c["name"]
    for table in (TOK_CASES, HEAD_CASES):
        for kernel in {c["kernel"] for c in table}:
            walks = {-(-(c["B"] - chunk) // n) for c in table if c["kernel"] == kernel for n in c["nchunks"] for chunk in range(n)}
            assert max(walks) > 4 and len(walks) > 2, (kernel, walks)
            if kernel == "mfma":   # the two pipelined kernels: every look-ahead depth
                assert {1, 2, 3} <= walks, walks
            assert any(c["B"] % n for c in table if c["kernel"] == kernel for n in c["nchunks"]), kernel
