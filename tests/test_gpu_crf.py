"""GPU: feature-guided CRF refinement -- msst_crf_affinity and msst_crf_step (maskedsst_amd/csrc/msst_crf.hip) and maskedsst_amd/crf.py
against the float64 restatement of tests/crf_util.py: the affinity exact on whole-number tables (no tolerance: every border and halo
position, every cause of a dead pixel), real-valued weights and probabilities against float64, the symmetry of the weights and the
structure of the refinement to the bit, the route through the model and the script.  The bars are 4 x the errors measured on the
MI355X (profiles/crf_parity_measured.jsonl); tests/test_crf_host.py checks on the CPU that they still tell the mutated
restatements apart.  Every output is prefilled with a sentinel, so that nothing may be left unwritten."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

import crf_util as cu
from test_gpu_pca import child, dev, make_model, same_bits

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5


def raw_affinity(feat, cover, R, a, s, g):
    """msst_crf_affinity with both outputs prefilled: (k [Bs, K, Hs, Ws] fp32, live bool) on the CPU"""
    from maskedsst_amd import _lib
    from maskedsst_amd.features import _p, _stream
    f = dev(feat)
    c = None if cover is None else dev(cover)
    Bs, _, Hs, Ws = f.shape
    K = (2 * R + 1) ** 2 - 1
    k = torch.full((Bs, K, Hs, Ws), SENTINEL, device="cuda")
    live = torch.full((Bs, Hs, Ws), 77, dtype=torch.uint8, device="cuda")
    at, st = (ctypes.c_float * K)(*[float(v) for v in a]), (ctypes.c_float * K)(*[float(v) for v in s])
    _lib.check(_lib.load().msst_crf_affinity(_p(f), _p(c), Bs, 96, Hs, Ws, R, ctypes.cast(at, ctypes.c_void_p), ctypes.cast(st, ctypes.c_void_p),
                                             float(g), _p(k), _p(live), _stream()), "msst_crf_affinity")
    k, live = k.cpu(), live.cpu()
    assert not bool((k == SENTINEL).any()) and bool((live <= 1).all())
    return k, live.bool()


def raw_step(scores, k, live, R, q_in=None, unary="logits", scale=1.0, prev=None):
    """msst_crf_step with every output prefilled: (q_out, classes int32, changed or None) on the CPU"""
    from maskedsst_amd import _lib
    from maskedsst_amd.features import _p, _stream
    sc, kd, lv = dev(scores), dev(k), dev(live)
    qi = None if q_in is None else dev(q_in)
    pv = None if prev is None else dev(prev.astype(np.int32))
    Bs, nc, Hs, Ws = sc.shape
    q = torch.full((Bs, nc, Hs, Ws), SENTINEL, device="cuda")
    cls = torch.full((Bs, Hs, Ws), -77, dtype=torch.int32, device="cuda")
    changed = torch.zeros(1, dtype=torch.int32, device="cuda") if prev is not None else None
    _lib.check(_lib.load().msst_crf_step(_p(sc), 0 if unary == "logits" else 1, float(scale), _p(qi), _p(kd), _p(lv), Bs, nc, Hs, Ws, R, _p(q),
                                         _p(cls), _p(pv), _p(changed), _stream()), "msst_crf_step")
    q, cls = q.cpu(), cls.cpu()
    assert not bool((q == SENTINEL).any()) and not bool((cls == -77).any())
    return q, cls, None if changed is None else int(changed.cpu()[0])


def t32(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def given_affinity(k, live, R):
    from maskedsst_amd import CrfAffinity
    return CrfAffinity(dev(k), dev(live), R)


# --------------------------------------------------------------------------------------------------- 1. the affinity, exact
@pytest.mark.parametrize("R", [1, 2, 3])
@pytest.mark.parametrize("shape", cu.INT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_affinity_is_exact_at_every_border_and_halo_position(shape, R):
    a, s = cu.int_tables(R)
    for kind in cu.DEAD_KINDS:
        feat, cover, dead = cu.int_case(shape, kind, seed=R)
        want, want_live = cu.affinity(feat, cover, R, a, s, 2.0)
        assert np.array_equal(want_live, ~dead)
        k, live = raw_affinity(feat, cover, R, a, s, 2.0)
        assert torch.equal(live, t32(want_live)), kind
        assert torch.equal(k, t32(want.astype(np.float32))), (kind, (k != t32(want.astype(np.float32))).nonzero()[:5])
        if kind == "none":                                          # without a cover map: the same
            k2, live2 = raw_affinity(feat, None, R, a, s, 2.0)
            assert torch.equal(k2, k) and torch.equal(live2, live)


# ----------------------------------------------------------------------------------------------- 2. the affinity, real-valued
@pytest.mark.parametrize("case", cu.AFF_REAL, ids=lambda c: f"R{c[0]}-{c[1]}")
def test_affinity_against_float64_and_symmetric_to_the_bit(case):
    R, form = case
    feat, cover, _ = cu.real_features(cu.AFF_REAL_SHAPE, form, 5)
    a, s, g = cu.tables(R)
    want, want_live = cu.affinity(feat, cover, R, a, s, g)
    assert (want > 0.9 * (a.max() + s.max())).mean() > 0.01         # cos near 1 is well represented
    k, live = raw_affinity(feat, cover, R, a, s, g)
    assert torch.equal(live, t32(want_live)) and torch.equal(k == 0, t32(want == 0))
    Bs, K, Hs, Ws = k.shape
    for j, (dy, dx) in enumerate(cu.offsets(R)):                    # k[p, j] and k[p + o_j, K - 1 - j]: the same bits
        ys, xs = slice(max(0, -dy), Hs - max(0, dy)), slice(max(0, -dx), Ws - max(0, dx))
        yq, xq = slice(max(0, -dy) + dy, Hs - max(0, dy) + dy), slice(max(0, -dx) + dx, Ws - max(0, dx) + dx)
        assert same_bits(k[:, j, ys, xs].contiguous(), k[:, K - 1 - j, yq, xq].contiguous()), (j, dy, dx)
    cu.check(f"affinity_R{R}_{form}", dict(k=cu.rel_err(k.numpy(), want)))


# --------------------------------------------------------------------------------------------------- 3. the step, real-valued
def classes_agree(cls, q64, live, gap):
    """the kernel's classes against float64's on every live pixel whose float64 margin reaches the gap; -1 exactly where dead"""
    want = cu.argmax(q64, live)
    sure = live & (cu.margin(q64, live) >= gap)
    got = cls.numpy().astype(np.int64)
    assert np.array_equal(got == -1, ~live)
    assert np.array_equal(got[sure], want[sure]), int((got[sure] != want[sure]).sum())
    assert (live & ~sure).sum() <= cu.MARGIN_SHARE * live.sum()


@pytest.mark.parametrize("unary", ["logits", "votes"])
@pytest.mark.parametrize("R", cu.STEP_R)
@pytest.mark.parametrize("nc", cu.STEP_NC)
def test_step_against_float64(nc, R, unary):
    scores, k, live, q0 = cu.step_case(nc, R, unary)
    lv = cu.live_refine(live, scores)
    assert 0 < (live & ~lv).sum() and (~live).sum() > 0
    U = cu.unaries(scores, unary, 1.0)
    want0 = cu.step(U, lv, k, None, R)
    want1 = cu.step(U, lv, k, q0, R)
    got0, cls0, _ = raw_step(scores, k, live, R, None, unary)
    got1, cls1, changed = raw_step(scores, k, live, R, q0, unary, prev=cls0.numpy())
    if unary == "logits" and nc > 1:                                # a class whose score is -inf: probability 0 throughout
        gone = np.isneginf(scores) & lv[:, None]
        assert gone.any() and bool((got0.numpy()[gone] == 0).all()) and bool((got1.numpy()[gone] == 0).all())
    half, _, _ = raw_step(scores, k, live, R, q0, unary, scale=0.5)   # the scale is applied to the unaries alone
    err = dict(q0=cu.rel_err(got0.numpy(), want0), q1=cu.rel_err(got1.numpy(), want1),
               q1_half_scale=cu.rel_err(half.numpy(), cu.step(cu.unaries(scores, unary, 0.5), lv, k, q0, R)))
    bar = cu.check(f"step_nc{nc}_R{R}_{unary}", err)
    assert changed == int((lv & (cls0.numpy() != cls1.numpy())).sum())
    if bar is not None:
        classes_agree(cls0, want0, lv, bar["q0"])
        classes_agree(cls1, want1, lv, bar["q1"])


@pytest.mark.parametrize("case", cu.REFINE_CASES, ids=lambda c: f"nc{c[0]}-R{c[1]}-{c[2]}")
def test_five_step_refinement_against_float64(case):
    from maskedsst_amd import crf_refine
    nc, R, unary = case
    scores, k, live = cu.refine_case(nc, R, unary)
    want_cls, want_q, want_hist, _, lv = cu.refine(scores, k, live, R, cu.REFINE_ITERS, unary)
    res = crf_refine(dev(scores), given_affinity(k, live, R), iters=cu.REFINE_ITERS, unary=unary)
    assert res.classes.dtype == torch.int64 and res.history.dtype == torch.int64 and not res.history.is_cuda
    bar = cu.check(f"refine_nc{nc}_R{R}_{unary}", dict(probs=cu.rel_err(res.probs.cpu().numpy(), want_q)))
    assert res.history.tolist() == want_hist.tolist()
    if bar is not None:
        classes_agree(res.classes.cpu(), want_q, lv, bar["probs"])


# ----------------------------------------------------------------------------------------------------- 4. structure, to the bit
def test_structure_to_the_bit():
    from maskedsst_amd import crf_affinity, crf_refine
    nc, R, unary = cu.REFINE_CASES[0]
    scores, k, live = cu.refine_case(nc, R, unary)
    sd = dev(scores)
    aff = given_affinity(k, live, R)
    # zero tables: the bits of step 0 at every step, and nothing changes
    zero = given_affinity(np.zeros_like(k), live, R)
    q0, cls0, _ = raw_step(scores, k, live, R, None, unary)
    for iters in (0, 1, 3):
        r = crf_refine(sd, zero, iters=iters, unary=unary)
        assert same_bits(r.probs.cpu(), q0) and torch.equal(r.classes.cpu(), cls0.long()) and r.history.tolist() == [0] * iters
    # iters = 0 through crf_refine is step 0, whatever the weights
    r0 = crf_refine(sd, aff, iters=0, unary=unary)
    assert same_bits(r0.probs.cpu(), q0) and torch.equal(r0.classes.cpu(), cls0.long()) and r0.history.tolist() == []
    # two calls: the same bits
    a = crf_refine(sd, aff, iters=3, unary=unary)
    b = crf_refine(sd, aff, iters=3, unary=unary)
    assert same_bits(a.probs, b.probs) and torch.equal(a.classes, b.classes) and torch.equal(a.history, b.history)
    # a scene alone and inside a batch of three: the same bits, affinity and refinement
    feat, cover, _ = cu.real_features((3,) + cu.REFINE_SHAPE[1:], "raw", 9)
    sc3 = dev(cu.real_scores(cu.fields((3,) + cu.REFINE_SHAPE[1:], 6, np.random.default_rng(1)), 7, "logits", 2))
    all3 = crf_affinity(dev(feat), dev(cover), radius=3)
    ref3 = crf_refine(sc3, all3, iters=2)
    for b in range(3):
        one = crf_affinity(dev(feat[b:b + 1]), dev(cover[b:b + 1]), radius=3)
        assert same_bits(one.weights, all3.weights[b:b + 1].contiguous()) and torch.equal(one.live, all3.live[b:b + 1])
        r = crf_refine(sc3[b:b + 1].contiguous(), one, iters=2)
        assert same_bits(r.probs, ref3.probs[b:b + 1].contiguous()) and torch.equal(r.classes, ref3.classes[b:b + 1])
    again = crf_affinity(dev(feat), dev(cover), radius=3)
    assert same_bits(again.weights, all3.weights) and torch.equal(again.live, all3.live)


@pytest.mark.parametrize("stride", [8, 5])
def test_refine_scene_through_the_model(stride):
    from maskedsst_amd import RefinedScene, crf_affinity, crf_refine, refine_scene
    model = make_model()
    model.train()
    g = torch.Generator().manual_seed(3)
    scene = torch.randn(2, 50, 16, 16, generator=g).cuda()
    _, logits = model.predict_scene(scene, stride=stride, return_logits=True)
    emb = model.encode_scene(scene, stride=stride, normalize=True)
    covered = emb.cover > 0
    assert bool(covered.all()) == (stride == 8)                     # stride 5: rows and columns 13 .. 15 lie in no window
    want = crf_refine(logits, crf_affinity(emb, radius=1), iters=3)
    res = model.refine_scene(scene, logits, stride=stride, iters=3, radius=1)
    assert isinstance(res, RefinedScene) and model.training and torch.equal(res.cover, emb.cover)
    assert res.classes.shape == (2, 16, 16) and res.probs.shape == (2, 5, 16, 16) and res.history.shape == (3,)
    assert torch.equal(res.classes, want.classes) and same_bits(res.probs, want.probs) and torch.equal(res.history, want.history)
    assert torch.equal(res.classes == -1, ~covered) and torch.equal(torch.isnan(res.probs).all(dim=1), ~covered)
    assert torch.equal(torch.isnan(res.probs).any(dim=1), ~covered)
    assert float((res.probs.sum(dim=1)[covered] - 1).abs().max()) < 1e-5
    other = refine_scene(model, scene, logits, embedding=emb, iters=3, radius=1)      # the embedding handed over: no second pass
    assert torch.equal(other.classes, res.classes) and same_bits(other.probs, res.probs)
    raw = model.encode_scene(scene, stride=stride, normalize=False)                  # a raw map works too: the kernel forms the norms
    r2 = model.refine_scene(scene, logits, embedding=raw, iters=3, radius=1)
    assert torch.equal(r2.classes == -1, ~covered) and float((r2.probs - res.probs)[covered[:, None].expand_as(res.probs)].abs().max()) < 1e-4


# --------------------------------------------------------------------------------------------------------------------- 5. script
def test_finetune_val_crf_script():
    """finetune.py --val-crf: one more line per validation pass"""
    out = child([sys.executable, "finetune.py", "--steps", "1", "--val-scenes", "4", "--val-every", "1", "--val-crf", "3", "--val-crf-radius", "1"], 600)
    lines = [l.split() for l in out.splitlines() if l.startswith("val-crf step ")]
    assert [e[2] for e in lines] == ["1"], out
    e = lines[0]
    assert e[3:7] == ["iters", "3", "radius", "1"] and e[7] == "acc_before" and 0.0 <= float(e[8]) <= 1.0, e
    assert e[9] == "acc_after" and 0.0 <= float(e[10]) <= 1.0 and e[11] == "changed" and int(e[12]) >= 0, e
    assert e[13] == "pixels" and int(e[14]) > 0 and e[15:] == ["scenes", "4"], e


def test_crf_time_script():
    """tools/crf_time.py --smoke: exit 0 and ONE JSON line, nothing appended"""
    out = child([sys.executable, os.path.join("tools", "crf_time.py"), "--smoke"], 300)
    lines = [l for l in out.splitlines() if l.strip()]
    assert len(lines) == 1, out
    row = json.loads(lines[0])
    assert row["tool"] == "crf_time" and row["shape"] == "4x64x64" and row["nc"] == 16 and row["radius"] == 1
    assert row["affinity_us"] > 0 and row["eager_affinity_us"] > 0 and row["step_us"] > 0 and row["eager_step_us"] > 0
    assert row["affinity_max_diff"] < 1e-3 and row["step_max_diff"] < 1e-4 and row["classes_agree"] > 0.999
