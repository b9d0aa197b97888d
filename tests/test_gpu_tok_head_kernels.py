"""GPU: the tokenizer and SimMIM head kernels alone -- msst_tokenize_fwd, msst_tokenize_bwd, msst_head_fwd, msst_head_bwd called through the
C ABI with ctypes, not through the engine, so that the chunk count nchunk is a parameter of the test -- against the float64 restatements
of tests/tok_head_util.py (pinned to the oracle by tests/test_tok_head_host.py).

tokenize_fwd_mfma, tokenize_bwd_mfma, tokenize_bwd_kernel<10 | 0>, head_bwd_mfma and head_bwd_kernel are persistent over the batch:
workgroup (block c, chunk) walks samples chunk, chunk + nchunk, ...; the two MFMA backward kernels look ahead in a software pipeline
and clamp the look-ahead sample at B - 1.  The engine's nchunk equals B for every B <= 8, the batch sizes of all other tests that compare
these kernels with a reference: there the walk has one sample and every look-ahead is the clamped dummy.  Here nchunk < B: walks of
11, 6 / 5, 3 / 3 / 3 / 2 samples, ragged chunk ends, dropout elements addressed by the sample index of a later iteration, the duplicate
loop of head_bwd_mfma, and the exactly-full / flushed reduce tables.

One bar: rel-L2 <= 2e-5 per tensor against float64 (relative 2e-5 for the loss scalar), the bar of
test_gpu_input_grad.py::test_tokenize_bwd_input_vs_float64 for this very fp32 arithmetic; the case tables hold only shapes at which fp32
autograd of the restatement on the CPU stays within 2e-5 / 3.5 (test_tok_head_host.py asserts it per case).  Every output and the whole
slab / partial scratch are prefilled with NaN and must come back finite (every word that is read was written); two identical calls give
the same bits; dy is bit-identical across the nchunk values of a case, nchunk = B included (the partition does not reach it); tensors whose float64 value is
identically zero are exactly 0.0.

The scene instances of the tokenizer kernels (msst_tokenize_scene_fwd_train / msst_tokenize_scene_bwd) are not run here:
tests/test_gpu_shifting_window.py ties them bit for bit to the batch instances tested here.

Measured on the MI355X: profiles/tok_head_kernels_parity_measured.jsonl (one row per case and nchunk)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from util import rel_l2, record
from dropout import keep_scaled
from tok_head_util import (BAR, BAND, DROP, GOUT, D, TOK_CASES, TOK_FWD_BIG, TOK_BY_NAME, TOK_GRADS, TOK_GRADS_NO_POS, HEAD_CASES, HEAD_BY_NAME,
                           tok_inputs, tok_grads_ref, tokenizer_ref, drop_scale, head_inputs, head_fwd_ref, head_grads_ref)

pytestmark = pytest.mark.gpu

TOK_BWD_PARAMS = [(c["name"], n) for c in TOK_CASES for n in c["nchunks"]]
HEAD_BWD_PARAMS = [(c["name"], n) for c in HEAD_CASES for n in c["nchunks"]]
_ids = lambda ps: [f"{name}-nchunk{n}" for name, n in ps]   # noqa: E731


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _f(t):
    return t.float().cuda().contiguous()


def _finite(t):
    return bool(torch.isfinite(t).all())


# ---------------------------------------------------------------------------------------------- tokenizer
@functools.lru_cache(maxsize=None)
def tok_dev(name):
    """the fp32 device copies of a case's inputs"""
    c, x = TOK_BY_NAME[name], tok_inputs(name)
    d = {k: _f(v) for k, v in x["q"].items()}
    d["pos_a"], d["pos_b"] = (_f(x["pos"][0]), _f(x["pos"][1])) if c["split"] else (_f(x["pos"]), None)
    d["img"] = _f(x["img"])
    d["dx0"] = _f(x["dx0"]) if x["dx0"] is not None else None
    d["masks"] = {k: m.to(torch.uint8).cuda() for k, m in x["masks"].items()}
    return d


def run_tok_fwd(lib, c, d, mask, drop, img=None):
    img = d["img"] if img is None else img
    B = img.shape[0]
    out = _nan(B, c["S"] * c["N"], D)
    rc = lib.msst_tokenize_fwd(_p(img), _p(d["pre_g"]), _p(d["pre_b"]), _p(d["w"]), _p(d["b"]), _p(d["post_g"]), _p(d["post_b"]),
                               _p(d["pos_a"]), _p(d["pos_b"]), c["split"], _p(d["mask_token"]), _p(mask), _p(out), B, c["S"], c["N"], c["P"],
                               drop[0], drop[1], _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out


def run_tok_bwd(lib, c, d, mask, drop, nchunk, with_pos=True):
    """-> ({gradient name: tensor}, slab); every output and the whole slab NaN before the call"""
    S, N, P, split = c["S"], c["N"], c["P"], c["split"]
    g = dict(dpre_g=_nan(P), dpre_b=_nan(P), dw_emb=_nan(S, D, P), db_emb=_nan(S, D), dpost_g=_nan(D), dpost_b=_nan(D))
    if with_pos:
        g["dpos_a"], g["dpos_b"] = (_nan(N, split), _nan(S, D - split)) if split else (_nan(S * N, D), None)
        g["dmask_token"] = _nan(D)
    slab = _nan(S * nchunk * (N * D + D * P + 4 * D + 32) + S * N * D)
    rc = lib.msst_tokenize_bwd(_p(d["img"]), _p(d["pre_g"]), _p(d["pre_b"]), _p(d["w"]), _p(d["b"]), _p(d["post_g"]), _p(d["post_b"]), _p(mask),
                               _p(d["dx0"]), _p(slab), nchunk, _p(g["dpre_g"]), _p(g["dpre_b"]), _p(g["dw_emb"]), _p(g["db_emb"]),
                               _p(g["dpost_g"]), _p(g["dpost_b"]), _p(g.get("dpos_a")), _p(g.get("dpos_b")), split, _p(g.get("dmask_token")),
                               c["B"], S, N, P, drop[0], drop[1], _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return g, slab


def host_keep(c, B, drop):
    """the keep mask times its scale [B, S N, 96] by the numpy restatement of the kernels' stateless dropout (tests/dropout.py): the
    embedding dropout is site 0 of layer 255, element group (b T + t) 24 + feature / 4"""
    T = c["S"] * c["N"]
    grp = np.arange(B * T, dtype=np.int64)[:, None] * 24 + np.arange(D)[None, :] // 4
    el = np.broadcast_to(np.arange(D)[None, :] % 4, grp.shape)
    return torch.from_numpy(keep_scaled(drop[0], drop[1], 255, 0, grp, el)).reshape(B, T, D)


@functools.lru_cache(maxsize=None)
def tok_keep(name, mname, drop):
    """the dropout keep mask times its scale, read back from msst_tokenize_fwd run with the same (p, seed) (non-zero position table and
    mask token: a dropped element is an exact 0, a kept one is not); 1.0 without dropout.  Checked: the realised drop rate, and every
    element against the host restatement of the mask (an element addressed by the wrong sample would show here)"""
    if not drop[0]:
        return 1.0
    from maskedsst_amd import _lib
    c, d = TOK_BY_NAME[name], tok_dev(name)
    out = run_tok_fwd(_lib.load(), c, d, d["masks"][mname], drop)
    assert _finite(out)
    keep = (out != 0).double().cpu()
    rate = 1.0 - float(keep.mean())
    assert abs(rate - drop[0]) < 0.01, rate
    keep = keep * drop_scale(drop[0])
    assert torch.equal(keep.float(), host_keep(c, c["B"], drop)), "the forward's dropout mask is not the stateless mask of (seed, element)"
    return keep


@functools.lru_cache(maxsize=None)
def tok_ref_grads(name, mname, drop):
    """the float64 reference of a (case, mask, dropout): computed once, shared by the nchunk values"""
    return tok_grads_ref(name, mname, tok_keep(name, mname, drop))


def check_tok_grads(got, ref, names, mname, where):
    """-> {tensor: rel-L2}; asserts finiteness, exact zeros and the bar"""
    errs = {}
    for k in names:
        if ref[k] is None:
            continue
        assert _finite(got[k]), (where, k)
        if k == "dmask_token" and mname == "none":
            # formed by subtracting two accumulators: an absolute bar, BAR x the norm of what it is subtracted from
            errs[k + "_abs"] = float(got[k].double().norm())
            assert float(ref[k].abs().max()) == 0.0
            assert errs[k + "_abs"] <= BAR * float(ref["dx0_colsum"].norm()), (where, k, errs[k + "_abs"])
        elif float(ref[k].abs().max()) == 0.0:
            assert float(got[k].abs().max()) == 0.0, (where, k)
        else:
            errs[k] = rel_l2(got[k], ref[k])
    bad = {k: v for k, v in errs.items() if not k.endswith("_abs") and not v <= BAR}
    assert not bad, (where, bad)
    return errs


@pytest.mark.parametrize("name,nchunk", TOK_BWD_PARAMS, ids=_ids(TOK_BWD_PARAMS))
def test_tokenize_bwd_vs_float64(name, nchunk):
    """msst_tokenize_bwd: dpre_g, dpre_b, dw_emb, db_emb, dpost_g, dpost_b, dpos_a[, dpos_b], dmask_token against float64 autograd of
    sum(tokenizer_ref dx0), per mask and dropout setting of the case, at this nchunk"""
    from maskedsst_amd import _lib
    lib = _lib.load()
    c, d = TOK_BY_NAME[name], tok_dev(name)
    worst = {}
    for mname in c["masks"]:
        for drop in c["drops"]:
            where = (name, nchunk, mname, drop)
            ref = tok_ref_grads(name, mname, drop)
            got, _ = run_tok_bwd(lib, c, d, d["masks"][mname], drop, nchunk)
            again, _ = run_tok_bwd(lib, c, d, d["masks"][mname], drop, nchunk)
            assert all(torch.equal(got[k], again[k]) for k in got if got[k] is not None), where
            errs = check_tok_grads(got, ref, TOK_GRADS, mname, where)
            print(where, {k: f"{v:.2e}" for k, v in errs.items()})
            for k, v in errs.items():
                worst[k] = max(worst.get(k, 0.0), v)
            if mname == "all":
                assert all(float(got[k].abs().max()) == 0.0 for k in TOK_GRADS_NO_POS), where
            if c["null_pos"]:   # the classification path: no position and no mask-token gradient; the other six keep their bits
                cls, _ = run_tok_bwd(lib, c, d, d["masks"][mname], drop, nchunk, with_pos=False)
                assert all(torch.equal(cls[k], got[k]) for k in TOK_GRADS_NO_POS), where
    record("tok_kernels_bwd", case=name, nchunk=nchunk, kernel=c["kernel"], **{"err_" + k: v for k, v in worst.items()})


def check_tok_fwd(lib, c, name, mname, drop):
    d, x = tok_dev(name), tok_inputs(name)
    out = run_tok_fwd(lib, c, d, d["masks"][mname], drop)
    again = run_tok_fwd(lib, c, d, d["masks"][mname], drop)
    assert _finite(out) and torch.equal(out, again), (name, mname, drop)
    keep = 1.0
    if drop[0]:   # the keep mask read back from the output itself, checked against the host restatement of the stateless mask
        got_keep = (out != 0).cpu()
        assert abs(1.0 - float(got_keep.double().mean()) - drop[0]) < 0.01 or got_keep.numel() < 40000   # 0.01 is 4 sigma from 33600 elements on
        assert torch.equal(got_keep, host_keep(c, c["B"], drop) != 0), (name, mname)
        keep = got_keep.double() * drop_scale(drop[0])
    worst = 0.0
    for b in range(c["B"]):   # sample by sample: the host stays small
        kb = keep[b:b + 1] if drop[0] else 1.0
        ref = tokenizer_ref(x["img"][b:b + 1], x["q"], x["masks"][mname][b:b + 1], x["pos"], kb)
        assert float((out[b:b + 1].cpu() == 0).double().sum()) == float((ref == 0).double().sum()), (name, mname, drop, b)
        worst = max(worst, rel_l2(out[b:b + 1], ref))
    assert worst <= BAR, (name, mname, drop, worst)
    return out, worst


@pytest.mark.parametrize("case", TOK_CASES + [TOK_FWD_BIG], ids=[c["name"] for c in TOK_CASES + [TOK_FWD_BIG]])
def test_tokenize_fwd_vs_float64(case):
    """msst_tokenize_fwd on the backward's cases, without and with dropout, against tokenizer_ref sample by sample; under dropout the zeros
    are exactly the host restatement's.  mfma_fwd_B35_S64: several samples per forward chunk (nchunk = 1024 // 64 = 16 < B); each
    sample is also run as a batch of one -- a walk of a single sample -- and must give the same bits"""
    from maskedsst_amd import _lib
    lib = _lib.load()
    name = case["name"]
    worst = 0.0
    for mname in case["masks"]:
        for drop in ((0.0, 0), DROP) if "nchunks" in case else case["drops"]:
            out, err = check_tok_fwd(lib, case, name, mname, drop)
            worst = max(worst, err)
            if drop[0] == 0.0 and case["kernel"] == "mfma":
                d = tok_dev(name)
                for b in range(case["B"]):
                    one = run_tok_fwd(lib, case, d, d["masks"][mname][b:b + 1].contiguous(), drop, img=d["img"][b:b + 1].contiguous())
                    assert torch.equal(one[0], out[b]), (name, mname, b)
    record("tok_kernels_fwd", case=name, nchunk=min(case["B"], 1024 // case["S"]) if case["kernel"] == "mfma" else case["B"],
           kernel=case["kernel"], err_out=worst)


# ---------------------------------------------------------------------------------------------- head
@functools.lru_cache(maxsize=None)
def head_dev(name):
    x = head_inputs(name)
    d = {k: _f(x[k]) for k in ("y", "img", "w_pix", "b_pix", "dpred")}
    d["idx"] = x["idx"].to(torch.int32).cuda()
    d["csr_ptr"], d["csr_pos"] = x["csr_ptr"].cuda(), x["csr_pos"].cuda()
    d["gout"] = torch.tensor([GOUT], device="cuda")
    return d


def run_head_bwd(lib, c, d, gscale, gout, nchunk):
    S, N, P, K = c["S"], c["N"], c["P"], c["K"]
    dy, dw, db = _nan(c["B"], S * N, D), torch.full_like(d["w_pix"], float("nan")), torch.full_like(d["b_pix"], float("nan"))
    slab = _nan(S * nchunk * (P * D + P))
    rc = lib.msst_head_bwd(_p(d["y"]), _p(d["dpred"]), _p(d["csr_ptr"]), _p(d["csr_pos"]), _p(d["w_pix"]), c["per_block"], gscale, _p(gout),
                           _p(dy), _p(slab), nchunk, _p(dw), _p(db), c["B"], S, N, P, K, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return dict(dy=dy, dw_pix=dw, db_pix=db), slab


@functools.lru_cache(maxsize=None)
def head_dy_unchunked(name, with_gout):
    """dy of the call with nchunk = B, one sample per workgroup and no walk: the value every nchunk of the case must reproduce bit for bit"""
    from maskedsst_amd import _lib
    c, d = HEAD_BY_NAME[name], head_dev(name)
    return run_head_bwd(_lib.load(), c, d, head_inputs(name)["gscale"], d["gout"] if with_gout else None, c["B"])[0]["dy"]


@pytest.mark.parametrize("name,nchunk", HEAD_BWD_PARAMS, ids=_ids(HEAD_BWD_PARAMS))
def test_head_bwd_vs_float64(name, nchunk):
    """msst_head_bwd: dy, dw_pix, db_pix against head_bwd_ref, gout null and a device scalar 0.37, dpred random normal"""
    from maskedsst_amd import _lib
    lib = _lib.load()
    c, d, x = HEAD_BY_NAME[name], head_dev(name), head_inputs(name)
    worst = {}
    for with_gout in (False, True):
        where = (name, nchunk, with_gout)
        ref = dict(zip(("dy", "dw_pix", "db_pix"), head_grads_ref(name, GOUT if with_gout else 1.0)))
        gout = d["gout"] if with_gout else None
        got, _ = run_head_bwd(lib, c, d, x["gscale"], gout, nchunk)
        again, _ = run_head_bwd(lib, c, d, x["gscale"], gout, nchunk)
        assert all(_finite(v) for v in got.values()), where
        assert all(torch.equal(got[k], again[k]) for k in got), where
        unnamed = (ref["dy"] == 0).all(dim=-1)
        assert bool(unnamed.any()) and float(got["dy"].cpu()[unnamed].abs().max()) == 0.0, (where, "tokens no index names")
        errs = {k: rel_l2(got[k], ref[k]) for k in got}
        print(where, {k: f"{v:.2e}" for k, v in errs.items()})
        assert max(errs.values()) <= BAR, (where, errs)
        assert torch.equal(got["dy"], head_dy_unchunked(name, with_gout)), (where, "dy depends on the partition")
        for k, v in errs.items():
            worst[k] = max(worst.get(k, 0.0), v)
    record("head_kernels_bwd", case=name, nchunk=nchunk, kernel=c["kernel"], **{"err_" + k: v for k, v in worst.items()})


def run_head_fwd(lib, c, d, want_pred):
    B, S, N, P, K = c["B"], c["S"], c["N"], c["P"], c["K"]
    dpred, pred, partial, loss = _nan(B, K, P), (_nan(B, K, P) if want_pred else None), _nan(B * ((K + 63) // 64)), _nan(1)
    rc = lib.msst_head_fwd(_p(d["y"]), _p(d["img"]), _p(d["idx"]), _p(d["w_pix"]), _p(d["b_pix"]), c["per_block"], _p(dpred), _p(pred),
                           _p(partial), _p(loss), B, S, N, P, K, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert _finite(dpred) and _finite(partial) and _finite(loss) and (pred is None or _finite(pred)), c["name"]
    return dpred, pred, loss


@pytest.mark.parametrize("case", HEAD_CASES, ids=[c["name"] for c in HEAD_CASES])
def test_head_fwd_vs_float64(case):
    """msst_head_fwd with pred given and null: dpred and loss bit-identical between the two; pred and loss against head_ref; dpred equal to
    sign(pred64 - target) wherever |pred64 - target| >= 1e-4 (the host test bounds the share of elements inside that band)"""
    from maskedsst_amd import _lib
    lib = _lib.load()
    name = case["name"]
    d = head_dev(name)
    pred64, target, loss64 = head_fwd_ref(name)
    dpred, pred, loss = run_head_fwd(lib, case, d, True)
    dpred0, _, loss0 = run_head_fwd(lib, case, d, False)
    dpred1, pred1, loss1 = run_head_fwd(lib, case, d, True)
    assert torch.equal(dpred, dpred0) and torch.equal(loss, loss0), name
    assert torch.equal(dpred, dpred1) and torch.equal(pred, pred1) and torch.equal(loss, loss1), name
    err_pred = rel_l2(pred, pred64)
    err_loss = abs(float(loss) - float(loss64)) / abs(float(loss64))
    print(name, f"pred {err_pred:.2e} loss {err_loss:.2e}")
    assert err_pred <= BAR and err_loss <= BAR, (name, err_pred, err_loss)
    diff = pred64 - target
    clear = diff.abs() >= BAND
    assert torch.equal(dpred.double().cpu()[clear], torch.sign(diff)[clear]), name
    assert bool(((dpred == 1) | (dpred == -1) | (dpred == 0)).all())
    record("head_kernels_fwd", case=name, nchunk=case["B"], kernel="head_fwd", err_pred=err_pred, err_loss=err_loss)
