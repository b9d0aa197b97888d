"""GPU: the cross entropy with class weights, label smoothing and a confusion matrix (msst_loss.hip: the weighted instances of ce_fwd,
ce_finish and ce_bwd, and the unweighted ones behind the extended entry points; include/msst.h: msst_ce_ext_fwd, msst_ce_ext_bwd;
maskedsst_amd.ops.cross_entropy_stats(weight=, label_smoothing=,
confusion=), FusedCrossEntropy(weight, label_smoothing), confusion_report; maskedsst_amd.scene.scene_report).

Yardstick: float64 ``torch.nn.functional.cross_entropy(weight=, label_smoothing=, ignore_index=)`` and its autograd on the CPU (labels
outside [0, nc) are turned into ignored ones for it: torch refuses them, the kernels do not count them), and numpy for every integer
(the record; the confusion matrix against a ``bincount`` of ``label * nc + argmax``).  Bars (fused cross entropy
row): loss and dlogits (max-norm over max |dlogits|) within 1e-4 relative, the weight sum within 1e-6 relative, integers exact.
Where the weight sum is 0 (nothing counts, or every present class has weight 0) the loss is NaN on both sides and the kernels'
gradient is exact zeros, as in the existing "no row counts" case (torch's autograd divides 0 by 0 there and hands back NaN).
nc = 1: the gradient is zero in exact arithmetic (softmax = 1), so there is no max to be relative to; the bar is 1e-4 of the two
terms that cancel, ((1 - eps) w_y + eps W / nc) / weight sum.

Every shape runs every combination of labels {all valid, about 25 % ignored, all ignored, a few out of range}, weights {none, random
in [0.1, 3], one class at 0, all present classes at 0}, eps {0, 0.1} and logit scale {1, 100}, through the C ABI with every output
and the scratch prefilled with NaN bytes, twice (bit-identical).

Errors are handed to tests/util.py::record (MSST_RECORD=1 writes them out); measured on an MI355X:
profiles/ce_ext_parity_measured.jsonl."""
import ctypes

import numpy as np
import pytest
import torch

from util import record

pytestmark = pytest.mark.gpu

BAR, SUM_BAR = 1e-4, 1e-6
SHAPES = [(1, 1, 1), (3, 5, 1), (2, 8, 64), (1, 9, 7), (2, 20, 49), (2, 33, 5), (5, 8, 64), (1, 128, 3),
          (2, 16, 5), (2, 17, 5), (2, 32, 5)]   # the full 16 and 32 register buckets, the first class past the 16 bucket
LABELS = ["valid", "ignored25", "all_ignored", "bad"]
WEIGHTS = ["none", "random", "one_zero", "present_zero"]
EPS = [0.0, 0.1]
SCALES = [1.0, 100.0]


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t


# ------------------------------------------------------------------------------------------------ inputs and the yardstick
def make_inputs(shape, labels, weights, scale):
    """-> logits [R0, nc, M] fp32, labels [R0, M] int64, weight [nc] fp32 or None (CPU tensors)"""
    R0, nc, M = shape
    gen = torch.Generator().manual_seed(7 * R0 + 13 * nc + M + 101 * LABELS.index(labels) + 1009 * WEIGHTS.index(weights) + int(scale))
    x = torch.randn(R0, nc, M, generator=gen) * scale
    lab = torch.randint(0, nc, (R0, M), generator=gen)
    flat = lab.view(-1)
    n = flat.numel()
    if labels == "ignored25":
        flat[torch.rand(n, generator=gen) < 0.25] = -1
        if n >= 4:
            flat[1] = -1    # at least one ignored and one valid, whatever the draw
            flat[0] = max(int(flat[0]), 0)
    elif labels == "all_ignored":
        flat[:] = -1
    elif labels == "bad":
        pos = torch.randperm(n, generator=gen)[:max(1, n // 16)]
        flat[pos[0::2]] = nc
        flat[pos[1::2]] = -7
    w = None
    if weights != "none":
        w = torch.rand(nc, generator=gen) * 2.9 + 0.1
        if weights == "one_zero":
            w[int(torch.randint(0, nc, (1,), generator=gen))] = 0.0
        elif weights == "present_zero":
            present = torch.unique(flat[(flat >= 0) & (flat < nc)])
            w[present] = 0.0
    return x, lab, w


def reference(x, lab, w, eps):
    """float64 torch on the CPU and numpy counts.  -> dict(loss, dlogits [R0, nc, M] or None when the weight sum is 0, weight_sum,
    record [4 + 2 nc], confusion [nc, nc])"""
    R0, nc, M = x.shape
    counts = (lab >= 0) & (lab < nc)             # (-1 is the ignored label: it is outside too)
    bad = (lab != -1) & ~counts
    target = torch.where(counts, lab, torch.full_like(lab, -1))
    w64 = w.double() if w is not None else None
    xd = x.double().requires_grad_(True)
    loss = torch.nn.functional.cross_entropy(xd, target, weight=w64, ignore_index=-1, label_smoothing=eps)
    wy = (w64[lab[counts]] if w is not None else torch.ones(int(counts.sum()), dtype=torch.float64))
    weight_sum = float(wy.sum())
    dlogits = None
    if weight_sum > 0:
        loss.backward()
        dlogits = xd.grad.numpy()
    pred = np.argmax(x.numpy(), axis=1)          # the first maximum
    l, c = lab.numpy(), counts.numpy()
    hit = c & (pred == l)
    support = np.bincount(l[c], minlength=nc)
    correct = np.bincount(l[hit], minlength=nc)
    confusion = np.bincount(l[c] * nc + pred[c], minlength=nc * nc).reshape(nc, nc)
    rec = [int(c.sum()), int(hit.sum()), int(bad.sum()), 0] + support.tolist() + correct.tolist()
    return dict(loss=float(loss.detach()), dlogits=dlogits, weight_sum=weight_sum, record=rec, confusion=confusion,
                cancel=0.0 if weight_sum <= 0 else float(((1 - eps) * wy.max() + eps * (w64.sum() if w is not None else nc) / nc) / weight_sum))


# ------------------------------------------------------------------------------------------------ the C ABI, prefilled
def ext_abi(x, lab, w=None, eps=0.0, confusion=True, skip=None, gout=None, want_d=True):
    """msst_ce_ext_fwd + msst_ce_ext_bwd on cuda tensors, every output and the scratch prefilled with NaN (0xFF bytes for integers)
    -> dict(loss, record, sums, confusion, d, dlogits)"""
    from maskedsst_amd import _lib
    lib = _lib.load()
    R0, nc, M = x.shape
    nan = float("nan")
    loss = torch.full((), nan, device="cuda")
    rec = torch.full((5 + 2 * nc,), -1, dtype=torch.int64, device="cuda")
    sums = torch.full((2,), nan, dtype=torch.float64, device="cuda")
    cm = torch.full((nc, nc), -1, dtype=torch.int64, device="cuda") if confusion else None
    nbytes = lib.msst_ce_ext_scratch_bytes(R0, nc, M, int(confusion))
    assert nbytes == -(-R0 * M // 256) * (6 + 2 * nc + (nc * nc if confusion else 0)) * 4
    scratch = torch.full((nbytes + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    d = torch.full_like(x, nan) if want_d else None
    rc = lib.msst_ce_ext_fwd(P(x), P(lab), P(skip), -1, P(w), eps, P(d), P(loss), P(rec), P(sums), P(cm), P(scratch), R0, nc, M, stream())
    assert rc == 0, lib.msst_last_error()
    dl = None
    if want_d:
        dl = torch.full_like(x, nan)
        assert lib.msst_ce_ext_bwd(P(d), P(sums), P(gout), P(dl), R0, nc, M, stream()) == 0
    torch.cuda.synchronize()
    assert bool((scratch[nbytes:] == 0xFF).all()), "wrote past the scratch size it asked for"
    return dict(loss=loss, record=rec, sums=sums, confusion=cm, d=d, dlogits=dl)


def old_abi(x, lab, skip=None, gout=None, want_d=True):
    """the plain entry points, msst_ce_stats_fwd + msst_ce_bwd -> dict(loss, record, d, dlogits)"""
    from maskedsst_amd import _lib
    lib = _lib.load()
    R0, nc, M = x.shape
    loss = torch.full((), float("nan"), device="cuda")
    rec = torch.full((5 + 2 * nc,), -1, dtype=torch.int64, device="cuda")
    scratch = torch.full((lib.msst_ce_scratch_bytes(R0, nc, M),), 0xFF, dtype=torch.uint8, device="cuda")
    d = torch.full_like(x, float("nan")) if want_d else None
    assert lib.msst_ce_stats_fwd(P(x), P(lab), P(skip), -1, P(d), P(loss), P(rec), P(scratch), R0, nc, M, stream()) == 0
    dl = None
    if want_d:
        dl = torch.full_like(x, float("nan"))
        assert lib.msst_ce_bwd(P(d), P(rec), P(gout), P(dl), R0, nc, M, stream()) == 0
    torch.cuda.synchronize()
    return dict(loss=loss, record=rec, d=d, dlogits=dl)


def same_bits(a, b, keys, tag):
    for k in keys:
        assert torch.equal(bits(a[k]), bits(b[k])), (tag, k)


def compare(got, ref, nc, tag):
    """integers exact, the consistency of matrix and record, loss / dlogits / weight sum at their bars -> the three errors"""
    rec = got["record"].cpu()
    assert rec[1:].tolist() == ref["record"], (tag, rec[1:].tolist(), ref["record"])
    cm = got["confusion"].cpu().numpy()
    assert np.array_equal(cm, ref["confusion"]), (tag, cm, ref["confusion"])
    assert np.diag(cm).tolist() == rec[5 + nc:5 + 2 * nc].tolist() and cm.sum(axis=1).tolist() == rec[5:5 + nc].tolist(), tag
    loss, sums = float(got["loss"]), got["sums"].cpu().tolist()
    assert sums[0] == float(rec[:1].view(torch.float64)[0]), tag            # the loss sum, in both places
    g = got["dlogits"].double().cpu().numpy()
    scale = max(abs(ref["weight_sum"]), 1e-300)
    sum_err = abs(sums[1] - ref["weight_sum"]) / scale
    assert sum_err <= SUM_BAR, (tag, sums[1], ref["weight_sum"])
    if ref["weight_sum"] <= 0:
        assert sums[1] == 0.0 and loss != loss and ref["loss"] != ref["loss"], (tag, loss, ref["loss"], sums)
        assert not g.any(), tag                                              # exact zeros
        return 0.0, 0.0, sum_err
    assert np.isfinite(ref["loss"]) and np.isfinite(g).all(), tag
    lscale = max(abs(ref["loss"]), 1e-300)                                   # (one class: every row's loss is 0, on both sides exactly)
    loss_err = abs(loss - ref["loss"]) / lscale
    mean_err = abs(sums[0] / sums[1] - ref["loss"]) / lscale
    dmax = float(np.abs(ref["dlogits"]).max())
    dl_err = float(np.abs(g - ref["dlogits"]).max()) / (dmax if nc > 1 else ref["cancel"])
    print(f"{tag}: loss {loss:.9e} ref {ref['loss']:.9e} rel err {loss_err:.3e} (sums: {mean_err:.3e}), dlogits {dl_err:.3e}, "
          f"weight sum {sum_err:.3e}", flush=True)
    assert loss_err <= BAR and mean_err <= BAR, (tag, loss, ref["loss"])
    assert dl_err <= BAR, (tag, dl_err)
    return loss_err, dl_err, sum_err


# ------------------------------------------------------------------------------------------------ 1. kernels against float64 torch
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "R%d-nc%d-M%d" % s)
def test_ce_ext_kernels_vs_float64_torch(shape):
    R0, nc, M = shape
    worst = dict(loss_err=0.0, dlogits_err=0.0, weight_sum_err=0.0)
    for labels in LABELS:
        for weights in WEIGHTS:
            for scale in SCALES:
                x, lab, w = make_inputs(shape, labels, weights, scale)
                xc, lc, wc = x.cuda(), lab.cuda(), (w.cuda() if w is not None else None)
                for eps in EPS:
                    tag = "ce_ext R%d nc%d M%d %s w=%s eps%g x%g" % (*shape, labels, weights, eps, scale)
                    ref = reference(x, lab, w, eps)
                    if labels == "bad":
                        assert ref["record"][2] >= 1, tag
                    if labels == "ignored25" and R0 * M >= 4:
                        assert 0 < ref["record"][0] < R0 * M, tag
                    if weights == "present_zero" or labels == "all_ignored":
                        assert ref["weight_sum"] == 0.0, tag
                    got = ext_abi(xc, lc, wc, eps)
                    errs = compare(got, ref, nc, tag)
                    for k, e in zip(worst, errs):
                        worst[k] = max(worst[k], e)
                    again = ext_abi(xc, lc, wc, eps)
                    same_bits(got, again, ("loss", "record", "sums", "confusion", "d", "dlogits"), tag)
    record("ce_ext_vs_float64_torch", R0=R0, nc=nc, M=M, **worst)


def test_ce_ext_refuses_a_confusion_matrix_past_the_class_limit():
    """(1, limit + 1, 2): refused before anything is enqueued -- the prefilled outputs stay as they were; without the matrix the same
    shape runs"""
    from maskedsst_amd import _lib
    from maskedsst_amd.ops import cross_entropy_stats
    lib = _lib.load()
    nc = _lib.CE_CONFUSION_MAX_CLASSES + 1
    x, lab = torch.randn(1, nc, 2).cuda(), torch.tensor([[3, nc - 1]]).cuda()
    loss = torch.full((), 7.0, device="cuda")
    rec = torch.full((5 + 2 * nc,), -1, dtype=torch.int64, device="cuda")
    sums = torch.full((2,), 7.0, dtype=torch.float64, device="cuda")
    cm = torch.full((nc, nc), -1, dtype=torch.int64, device="cuda")
    scratch = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    assert lib.msst_ce_ext_scratch_bytes(1, nc, 2, 1) == 0
    rc = lib.msst_ce_ext_fwd(P(x), P(lab), None, -1, None, 0.0, None, P(loss), P(rec), P(sums), P(cm), P(scratch), 1, nc, 2, stream())
    torch.cuda.synchronize()
    assert rc == -2 and b"MSST_CE_CONFUSION_MAX_CLASSES" in lib.msst_last_error()
    assert float(loss) == 7.0 and bool((rec == -1).all()) and bool((cm == -1).all()) and sums.tolist() == [7.0, 7.0]
    with pytest.raises(_lib.MsstError, match="confusion"):
        cross_entropy_stats(x.reshape(1, nc, 1, 2), lab.reshape(1, 1, 2), confusion=True)
    w = torch.rand(nc).cuda() + 0.1
    ref = reference(x.cpu(), lab.cpu(), w.cpu(), 0.1)
    got = ext_abi(x, lab, w, 0.1, confusion=False)
    assert abs(float(got["loss"]) - ref["loss"]) <= BAR * abs(ref["loss"]) and got["record"][1:].tolist() == ref["record"]


# ------------------------------------------------------------------------------------------------ 2. the bits of the existing calls
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "R%d-nc%d-M%d" % s)
def test_ce_ext_without_weights_gives_the_bits_of_the_existing_calls(shape):
    """no weight, eps = 0: loss, record, d and dlogits of msst_ce_ext_* are those of msst_ce_stats_fwd / msst_ce_bwd bit for bit, with
    and without the confusion matrix, without d, and with a skip map and an incoming gradient; the Python op without the new
    arguments still goes through the plain calls, and with confusion=True alone it gives the same loss and gradient"""
    from maskedsst_amd.ops import cross_entropy_stats
    R0, nc, M = shape
    for labels in LABELS:
        for scale in SCALES:
            tag = "R%d nc%d M%d %s x%g" % (*shape, labels, scale)
            x, lab, _ = make_inputs(shape, labels, "none", scale)
            xc, lc = x.cuda(), lab.cuda()
            old = old_abi(xc, lc)
            same_bits(ext_abi(xc, lc, None, 0.0, confusion=False), old, ("loss", "record", "d", "dlogits"), tag)
            with_cm = ext_abi(xc, lc, None, 0.0, confusion=True)
            same_bits(with_cm, old, ("loss", "record", "d", "dlogits"), tag + " +confusion")
            assert with_cm["sums"][1] == old["record"][1], tag              # the weight sum is n_valid
            # through the Python op, [B, nc, H, W] with H = 1
            for kw in (dict(), dict(confusion=True)):
                px = xc.reshape(R0, nc, 1, M).clone().requires_grad_(True)
                loss, stats = cross_entropy_stats(px, lc.reshape(R0, 1, M), -1, **kw)
                loss.backward()
                torch.cuda.synchronize()
                assert torch.equal(bits(loss.detach()), bits(old["loss"])) and torch.equal(stats.record, old["record"]), (tag, kw)
                assert torch.equal(bits(px.grad.reshape(R0, nc, M)), bits(old["dlogits"])), (tag, kw)
                assert float(stats.weight_sum) == float(old["record"][1]) == stats.host().weight_sum, (tag, kw)
                if kw:
                    assert torch.equal(stats.confusion, with_cm["confusion"]) and stats.sums is not None
                    assert np.array_equal(stats.host().confusion, with_cm["confusion"].cpu().numpy())
                else:
                    assert stats.confusion is None and stats.sums is None and stats.host().confusion is None
    # once per shape: without d (loss and record), and with a skip map and an incoming gradient
    x, lab, _ = make_inputs(shape, "ignored25", "none", 1.0)
    xc, lc = x.cuda(), lab.cuda()
    same_bits(ext_abi(xc, lc, confusion=False, want_d=False), old_abi(xc, lc, want_d=False), ("loss", "record"), "R%d nc%d M%d no d" % shape)
    gen = torch.Generator().manual_seed(79)
    skip = torch.randint(0, nc, (R0, M), generator=gen)
    skip[torch.rand(R0, M, generator=gen) < 0.2] = -1
    sc, gout = skip.cuda(), torch.tensor(0.375, device="cuda")
    same_bits(ext_abi(xc, lc, skip=sc, gout=gout), old_abi(xc, lc, skip=sc, gout=gout), ("loss", "record", "d", "dlogits"),
              "R%d nc%d M%d skip gout" % shape)


def test_ce_ext_python_op_skip_map_and_incoming_gradient():
    """cross_entropy_stats(weight, label_smoothing, confusion, skip) gives the bits of the C ABI; host() agrees with the device
    properties; 3 x loss scales the gradient exactly; the no-gradient call writes the same loss and record"""
    from maskedsst_amd.ops import cross_entropy_stats
    shape = (2, 20, 49)
    x, lab, w = make_inputs(shape, "ignored25", "one_zero", 1.0)
    gen = torch.Generator().manual_seed(77)
    skip = torch.randint(0, 20, (2, 49), generator=gen)
    skip[torch.rand(2, 49, generator=gen) < 0.2] = -1
    xc, lc, wc, sc = x.cuda(), lab.cuda(), w.cuda(), skip.cuda()
    got = ext_abi(xc, lc, wc, 0.1, skip=sc)
    masked = torch.where(skip >= 0, lab, torch.full_like(lab, -1))
    compare(got, reference(x, masked, w, 0.1), 20, "ce_ext skip")
    a = xc.reshape(2, 20, 7, 7).clone().requires_grad_(True)
    loss, stats = cross_entropy_stats(a, lc.reshape(2, 7, 7), -1, skip=sc.reshape(2, 7, 7), weight=wc, label_smoothing=0.1, confusion=True)
    loss.backward()
    b = xc.reshape(2, 20, 7, 7).clone().requires_grad_(True)
    (3.0 * cross_entropy_stats(b, lc.reshape(2, 7, 7), -1, skip=sc.reshape(2, 7, 7), weight=wc, label_smoothing=0.1)[0]).backward()
    torch.cuda.synchronize()
    assert torch.equal(bits(loss.detach()), bits(got["loss"])) and torch.equal(stats.record, got["record"])
    assert torch.equal(bits(stats.sums), bits(got["sums"])) and torch.equal(stats.confusion, got["confusion"])
    assert torch.equal(bits(a.grad.reshape(shape)), bits(got["dlogits"])) and torch.equal(bits(3.0 * a.grad), bits(b.grad))
    h = stats.host()
    assert h.weight_sum == float(stats.weight_sum) == float(got["sums"][1]) and h.loss_sum == float(got["sums"][0])
    assert abs(h.loss - float(loss)) <= 1e-6 * abs(float(loss)) and h.n_valid == int(stats.n_valid) and h.confusion.sum() == h.n_valid
    nod = ext_abi(xc, lc, wc, 0.1, skip=sc, want_d=False)
    same_bits(nod, got, ("loss", "record", "sums", "confusion"), "no d")
    # a weight on the CPU, or in float64, is taken to the logits' device as fp32
    loss2, _ = cross_entropy_stats(xc.reshape(2, 20, 7, 7), lc.reshape(2, 7, 7), -1, skip=sc.reshape(2, 7, 7), weight=w.double(), label_smoothing=0.1)
    assert torch.equal(bits(loss2), bits(got["loss"]))


# ------------------------------------------------------------------------------------------------ 3. through a model
def test_weighted_smoothed_fused_criterion_matches_torch_through_a_model():
    """a tiny classifier (20 bands, depth 1, 2 heads, B = 2, fp32 mode): FusedCrossEntropy(weight, 0.1) against
    torch.nn.CrossEntropyLoss(weight, label_smoothing=0.1) on the same logits: loss within 1e-4, every parameter gradient within 2e-4
    of its tensor's max (the bars of test_gpu_ce.py)"""
    from test_gpu_scene import make_encoder
    from maskedsst_amd.ops import FusedCrossEntropy
    gen = torch.Generator().manual_seed(31)
    x = torch.randn(2, 20, 8, 8, generator=gen).cuda()
    label = torch.randint(-1, 6, (2, 8, 8), generator=gen).cuda()
    w = (torch.rand(6, generator=gen) * 2.9 + 0.1)
    w[4] = 0.0
    out = {}
    for kind in ("torch", "fused"):
        enc, _ = make_encoder(dict(bands=20, depth=1, heads=2, n_classes=6), "fp32")
        enc = enc.cuda().train()
        crit = (FusedCrossEntropy(-1, w, 0.1) if kind == "fused" else torch.nn.CrossEntropyLoss(w, ignore_index=-1, label_smoothing=0.1)).cuda()
        assert crit.weight.is_cuda
        logits = enc(x)
        loss = crit(logits, label)
        loss.backward()
        torch.cuda.synchronize()
        out[kind] = (float(loss.detach()), logits.detach().clone(), {n: p.grad.detach().double().cpu() for n, p in enc.named_parameters()})
    (lt, xt, gt), (lf, xf, gf) = out["torch"], out["fused"]
    assert torch.equal(xt, xf)   # the same logits
    loss_err = abs(lf - lt) / abs(lt)
    errs = {n: float((gf[n] - gt[n]).abs().max() / (gt[n].abs().max() + 1e-30)) for n in gt}
    worst = max(errs, key=errs.get)
    print(f"weighted + smoothed fused vs torch criterion: loss rel err {loss_err:.3e}, worst gradient {worst} {errs[worst]:.3e}", flush=True)
    assert loss_err <= 1e-4, (lt, lf)
    assert errs[worst] <= 2e-4, (worst, errs[worst])
    record("ce_ext_criterion_vs_torch", loss_err=loss_err, worst_grad=errs[worst], worst_grad_name=worst)


# ------------------------------------------------------------------------------------------------ 4. scene report
def test_scene_report_matches_scene_metrics_and_a_numpy_confusion_matrix():
    """a 2-scene 20 x 22 map (windows of 8: the last rows and columns are uncovered): the shared fields equal
    scene_metrics(fused=True); the report is confusion_report of the numpy matrix of the covered, labelled pixels"""
    from test_gpu_scene import make_encoder
    from maskedsst_amd.ops import confusion_report
    from maskedsst_amd.scene import scene_metrics, scene_report
    enc, scene = make_encoder(dict(bands=20, depth=1, heads=2, n_classes=6), "bf16", (2, 20, 20, 22))
    classes, logits = enc.cuda().predict_scene(scene.cuda(), return_logits=True)
    assert bool((classes == -1).any()) and bool((classes >= 0).any())
    labels = torch.randint(-1, 6, (2, 20, 22), generator=torch.Generator().manual_seed(3)).cuda()
    fused = scene_metrics(logits, classes, labels, fused=True)
    rep = scene_report(logits, classes, labels)
    assert (rep.loss, rep.acc, rep.macro_acc) == (fused.loss, fused.acc, fused.macro_acc), (rep[:3], fused)
    c, l = classes.cpu().numpy(), labels.cpu().numpy()
    counts = (c >= 0) & (l != -1)
    pred = np.argmax(logits.float().cpu().numpy(), axis=1)
    assert np.array_equal(pred[counts], c[counts])   # the class map is the argmax of the logit map
    cm = np.bincount(l[counts] * 6 + pred[counts], minlength=36).reshape(6, 6)
    want = confusion_report(cm)
    for key in ("oa", "aa", "kappa", "mean_f1", "mean_iou", "total"):
        a, b = getattr(rep.report, key), getattr(want, key)
        assert a == b or (a != a and b != b), (key, a, b)
    for key in ("precision", "recall", "f1", "iou", "support"):
        assert np.array_equal(getattr(rep.report, key), getattr(want, key)), key
    assert rep.report.total == int(counts.sum()) and abs(rep.report.oa - fused.acc) <= 1e-15 and abs(rep.report.aa - fused.macro_acc) <= 1e-15
    none = scene_report(logits, classes, torch.full_like(labels, -1))
    assert none.loss != none.loss and none.acc != none.acc and none.report.total == 0 and none.report.kappa != none.report.kappa
