"""GPU: the fused cross entropy (msst_loss.hip; maskedsst_amd.ops.cross_entropy_stats / FusedCrossEntropy) and what is built on it.

Yardstick: ``ce_reference`` below, a float64 numpy restatement of what the reference's ``CrossEntropyLoss(ignore_index)`` computes
(log-sum-exp cross entropy, mean over the counting rows) with the counts of its loops -- never torch's GPU kernel, never the code
under test.  Bars: every integer of the record exact; loss and dlogits (max-norm over max |dlogits|) within 1e-4 relative, the
project's fp32 bar.  Measured on an MI355X (profiles/ce_parity_measured.jsonl): loss <= 1.1e-7, dlogits <= 1.9e-7
over all cases; through the model the worst parameter gradient differs from the torch criterion's by 8.1e-7 of its tensor's max.

* the kernels against the yardstick over every shape / label variant / logit scale, through the C ABI with every output and the
  scratch prefilled with NaN bytes, twice (bit-identical), and through the Python op (the same bits);
* the argmax tie rule, NaN / +inf rows, a batch prefix, the incoming gradient, the launch count;
* through the model: FusedCrossEntropy against torch.nn.CrossEntropyLoss (three heads), two fused 5-step runs bit-identical;
* scene_metrics(fused=True) against fused=False.

Mutations of msst_loss.hip that this file must catch (each fails test_ce_kernels_vs_float64):
  1. drop the max subtraction (``expf(x - mx)`` -> ``expf(x)``, ``loss = logf(sum) - xl``): the scale-100 cases overflow;
  2. count ignored rows in n_valid (``cand`` without ``label != a.ignore_index``): n_valid, bad_labels and the loss move in every
     variant that has an ignored label."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import seed_all
from util import record

pytestmark = pytest.mark.gpu

BAR = 1e-4   # the project's fp32 bar


# ------------------------------------------------------------------------------------------------ the yardstick
def ce_reference(logits, labels, ignore_index=-1, skip=None):
    """float64.  logits [R0, nc, M], labels [R0, M] (numpy).  -> dict(loss, dlogits [R0, nc, M], counts ..., rows: counting mask,
    row_loss)"""
    x = logits.astype(np.float64)
    R0, nc, M = x.shape
    lab = labels.astype(np.int64)
    live = lab != ignore_index
    if skip is not None:
        live &= skip >= 0
    inrange = (lab >= 0) & (lab < nc)
    rows = live & inrange
    with np.errstate(all="ignore"):
        mx = x.max(axis=1)
        lse = np.log(np.exp(x - mx[:, None, :]).sum(axis=1)) + mx
        safe = np.where(inrange, lab, 0)
        xl = np.take_along_axis(x, safe[:, None, :], axis=1)[:, 0, :]
        row_loss = lse - xl
        soft = np.exp(x - lse[:, None, :])
    pred = np.argmax(x, axis=1)   # first maximum; a NaN is the maximum
    n = int(rows.sum())
    onehot = (np.arange(nc)[None, :, None] == safe[:, None, :]).astype(np.float64)
    with np.errstate(all="ignore"):
        d = np.where(rows[:, None, :], soft - onehot, 0.0)
        loss = row_loss[rows].sum() / n if n else float("nan")
    hit = rows & (pred == lab)
    return dict(loss=loss, d=d, dlogits=d / n if n else np.zeros_like(d), n_valid=n, n_correct=int(hit.sum()),
                bad_labels=int((live & ~inrange).sum()), nonfinite=int((rows & ~np.isfinite(row_loss)).sum()),
                support=[int((rows & (lab == c)).sum()) for c in range(nc)], correct=[int((hit & (lab == c)).sum()) for c in range(nc)],
                rows=rows, row_loss=row_loss)


def want_record(ref):
    return [ref["n_valid"], ref["n_correct"], ref["bad_labels"], ref["nonfinite"]] + ref["support"] + ref["correct"]


# ------------------------------------------------------------------------------------------------ the C ABI, prefilled
def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def ce_abi(logits3, labels, ignore_index=-1, skip=None, gout=None, want_d=True):
    """msst_ce_stats_fwd + msst_ce_bwd on [R0, nc, M] logits with loss, d, record, scratch and dlogits prefilled with NaN (0xFF bytes
    for the integer buffers) -> (loss, record int64 [5 + 2 nc], d, dlogits)"""
    from maskedsst_amd import _lib
    lib = _lib.load()
    R0, nc, M = logits3.shape
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    nan = float("nan")
    loss = torch.full((), nan, device="cuda")
    rec = torch.full((5 + 2 * nc,), -1, dtype=torch.int64, device="cuda")
    nbytes = lib.msst_ce_scratch_bytes(R0, nc, M)
    assert nbytes == -(-R0 * M // 256) * (5 + 2 * nc) * 4
    scratch = torch.full((nbytes + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    d = torch.full_like(logits3, nan) if want_d else None
    assert lib.msst_ce_stats_fwd(P(logits3), P(labels), P(skip), ignore_index, P(d), P(loss), P(rec), P(scratch), R0, nc, M, st) == 0
    assert bool((scratch[nbytes:] == 0xFF).all()), "wrote past the scratch size it asked for"
    dl = None
    if want_d:
        dl = torch.full_like(logits3, nan)
        assert lib.msst_ce_bwd(P(d), P(rec), P(gout), P(dl), R0, nc, M, st) == 0
    torch.cuda.synchronize()
    return loss, rec, d, dl


def relmax(got, ref):
    return float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-300))


def compare(got, ref, tag, finite_rows=None):
    """got = (loss, rec, d, dlogits) of ce_abi.  Integers exact; loss and dlogits at BAR.  finite_rows: compare dlogits on these rows
    only (the nonfinite test).  -> (loss error, dlogits error)"""
    loss, rec, d, dl = got
    assert rec[1:].tolist() == want_record(ref), (tag, rec[1:].tolist(), want_record(ref))
    loss = float(loss)
    loss_sum = float(rec[:1].view(torch.float64)[0])
    g = dl.double().cpu().numpy()
    dref = ref["dlogits"]
    if finite_rows is not None:
        g, dref = np.where(finite_rows[:, None, :], g, 0.0), np.where(finite_rows[:, None, :], dref, 0.0)
    if ref["n_valid"] == 0:
        assert loss != loss and loss_sum == 0.0, (tag, loss, loss_sum)
        assert not g.any() and not d.cpu().numpy().any(), tag   # exact zeros
        return 0.0, 0.0
    if not np.isfinite(ref["loss"]):
        assert not np.isfinite(loss), (tag, loss)
        loss_err = 0.0
    else:
        scale = max(abs(ref["loss"]), 1e-300)   # (one class: every row's loss is 0, on both sides exactly)
        loss_err = abs(loss - ref["loss"]) / scale
        sum_err = abs(loss_sum / ref["n_valid"] - ref["loss"]) / scale
        print(f"{tag}: loss {loss:.9e} ref {ref['loss']:.9e} rel err {loss_err:.3e} (from the record's sum: {sum_err:.3e})", flush=True)
        assert loss_err <= BAR and sum_err <= BAR, (tag, loss, ref["loss"])
    assert np.isfinite(g).all(), tag
    dl_err = relmax(g, dref)
    print(f"{tag}: dlogits max-norm rel err {dl_err:.3e}", flush=True)
    assert dl_err <= BAR, (tag, dl_err)
    # rows that do not count: exact zeros
    assert not np.where(ref["rows"][:, None, :], 0.0, dl.cpu().numpy()).any(), tag
    return loss_err, dl_err


# ------------------------------------------------------------------------------------------------ 1. kernels against float64
CASES = [(256, 8, 64), (32, 20, 64), (3, 8, 49), (256, 8, 1), (1, 8, 1), (5, 1, 64), (7, 2, 3), (2, 33, 64), (2, 40, 64), (2, 97, 5),
         (4, 8, 4096), (1, 1025, 3)]   # 1025 classes: a second CE_CHUNK histogram pass
VARIANTS = ["mixed", "none_ignored", "all_ignored", "bad_labels"]


def make_case(shape, variant, scale, seed=0):
    """-> (logits [R0, nc, M] cuda, labels [R0, M] cuda, skip or None).  (4, 8, 4096): a 64 x 64 map with a skip map that is -1 on a
    border of 3 pixels; (1, 8, 1) travels as [nc] through the Python op (python_shapes)."""
    R0, nc, M = shape
    gen = torch.Generator().manual_seed(1000 * seed + 7 * R0 + 13 * nc + M)
    logits = torch.randn(R0, nc, M, generator=gen) * scale
    labels = torch.randint(-1, nc, (R0, M), generator=gen)
    if variant == "none_ignored":
        labels = torch.randint(0, nc, (R0, M), generator=gen)
    elif variant == "all_ignored":
        labels = torch.full((R0, M), -1, dtype=torch.int64)
    elif variant == "bad_labels":
        flat = labels.view(-1)
        pos = torch.randperm(flat.numel(), generator=gen)[:max(2, flat.numel() // 50)]
        flat[pos[0::2]] = nc
        flat[pos[1::2]] = -7
    skip = None
    if M == 4096:
        skip = torch.randint(0, nc, (R0, 64, 64), generator=gen)
        skip[:, :3, :] = -1
        skip[:, -3:, :] = -1
        skip[:, :, :3] = -1
        skip[:, :, -3:] = -1
        skip = skip.reshape(R0, M).cuda()
    return logits.cuda(), labels.cuda(), skip


def python_shapes(shape, logits, labels, skip):
    """the tensors as the Python op takes them: [B, nc, H, W] / [B, nc] / [nc]"""
    R0, nc, M = shape
    if M == 1 and R0 == 1:
        return logits.reshape(nc), labels.reshape(()), None
    if M == 1:
        return logits.reshape(R0, nc), labels.reshape(R0), None
    H = int(round(M ** 0.5)) if int(round(M ** 0.5)) ** 2 == M else 1
    return logits.reshape(R0, nc, H, M // H), labels.reshape(R0, H, M // H), (skip.reshape(R0, H, M // H) if skip is not None else None)


@pytest.mark.parametrize("scale", [1.0, 100.0], ids=["scale1", "scale100"])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", CASES, ids=lambda s: "R%d-nc%d-M%d" % s)
def test_ce_kernels_vs_float64(shape, variant, scale):
    from maskedsst_amd.ops import cross_entropy_stats
    logits, labels, skip = make_case(shape, variant, scale)
    ref = ce_reference(logits.cpu().numpy(), labels.cpu().numpy(), -1, skip.cpu().numpy() if skip is not None else None)
    if variant == "bad_labels":
        assert ref["bad_labels"] >= 1
    if variant == "mixed" and shape[0] * shape[2] >= 64:
        assert 0 < ref["n_valid"] < shape[0] * shape[2]
    if scale == 100.0 and shape[1] > 1 and shape[0] * shape[2] >= 64:
        assert float(logits.max()) > 88.7   # exp overflows in fp32 without the max subtraction
    tag = "ce R%d nc%d M%d %s x%g" % (*shape, variant, scale)
    got = ce_abi(logits, labels, -1, skip)
    loss_err, dl_err = compare(got, ref, tag)
    # a second call: the same bits everywhere
    again = ce_abi(logits, labels, -1, skip)
    for a, b, name in zip(got, again, ("loss", "record", "d", "dlogits")):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), (tag, name)
    # without d: the same loss and record
    nod = ce_abi(logits, labels, -1, skip, want_d=False)
    assert torch.equal(nod[0].view(torch.int32), got[0].view(torch.int32)) and torch.equal(nod[1], got[1]), tag
    # through the Python op and autograd: the same bits
    pl, plab, pskip = python_shapes(shape, logits, labels, skip)
    pl = pl.clone().requires_grad_(True)
    loss, stats = cross_entropy_stats(pl, plab, -1, skip=pskip)
    loss.backward()
    torch.cuda.synchronize()
    assert loss.dim() == 0 and torch.equal(loss.detach().view(torch.int32), got[0].view(torch.int32)), tag
    assert torch.equal(stats.record, got[1]) and torch.equal(pl.grad.reshape(shape).view(torch.int32), got[3].view(torch.int32)), tag
    h = stats.host()
    assert [h.n_valid, h.n_correct, h.bad_labels, h.nonfinite] + h.support + h.correct == want_record(ref)
    assert int(stats.n_valid) == ref["n_valid"] and int(stats.bad_labels) == ref["bad_labels"] and int(stats.nonfinite) == ref["nonfinite"]
    if ref["n_valid"]:
        recall = [c / s for c, s in zip(ref["correct"], ref["support"]) if s]
        assert abs(float(stats.acc) - ref["n_correct"] / ref["n_valid"]) <= 1e-12 and abs(h.acc - ref["n_correct"] / ref["n_valid"]) <= 1e-12
        assert abs(float(stats.macro_acc) - sum(recall) / len(recall)) <= 1e-12 and abs(h.macro_acc - sum(recall) / len(recall)) <= 1e-12
    else:
        assert h.acc != h.acc and h.macro_acc != h.macro_acc and h.loss != h.loss
        assert bool(torch.isnan(stats.acc)) and bool(torch.isnan(stats.macro_acc))
    record("ce_vs_float64", R0=shape[0], nc=shape[1], M=shape[2], variant=variant, scale=scale, loss_err=loss_err, dlogits_err=dl_err)


# ------------------------------------------------------------------------------------------------ 2. ties, NaN / inf rows
@pytest.mark.parametrize("shape", [(32, 20, 64), (2, 40, 64), (256, 8, 1)], ids=lambda s: "R%d-nc%d-M%d" % s)
def test_ce_argmax_ties_take_the_lowest_index(shape):
    """two equal maxima in every row: n_correct and correct[] follow torch.argmax / numpy (the first)"""
    R0, nc, M = shape
    logits, labels, _ = make_case(shape, "none_ignored", 1.0, seed=3)
    gen = torch.Generator().manual_seed(9)
    x = logits.cpu()
    top = x.max(dim=1).values + 1.0
    c1 = torch.randint(0, nc, (R0, M), generator=gen)
    c2 = (c1 + torch.randint(1, nc, (R0, M), generator=gen)) % nc
    x.scatter_(1, c1[:, None, :], top[:, None, :])
    x.scatter_(1, c2[:, None, :], top[:, None, :])
    lo, hi = torch.minimum(c1, c2), torch.maximum(c1, c2)
    # labels: a third of the rows at the lower tied class (correct), a third at the higher (wrong), the rest as drawn
    pick = torch.randint(0, 3, (R0, M), generator=gen)
    lab = torch.where(pick == 0, lo, torch.where(pick == 1, hi, labels.cpu()))
    ref = ce_reference(x.numpy(), lab.numpy())
    assert ref["n_correct"] >= int((pick == 0).sum()) and ref["n_correct"] < ref["n_valid"] - int((pick == 1).sum()) + 1
    compare(ce_abi(x.cuda(), lab.cuda()), ref, "ce ties R%d nc%d M%d" % shape)


@pytest.mark.parametrize("shape", [(32, 20, 64), (2, 40, 64)], ids=lambda s: "R%d-nc%d-M%d" % s)
def test_ce_nonfinite_rows_are_counted(shape):
    """a NaN and a +inf planted in counting rows (and one NaN in an ignored row, which must not count): nonfinite = exactly those rows,
    the loss is not finite, every other row's gradient is untouched"""
    R0, nc, M = shape
    logits, labels, _ = make_case(shape, "mixed", 1.0, seed=5)
    x, lab = logits.cpu(), labels.cpu()
    counting = (lab >= 0).nonzero()
    ignored = (lab == -1).nonzero()
    (ra, ma), (rb, mb), (rc, mc) = counting[3].tolist(), counting[len(counting) // 2].tolist(), counting[-2].tolist()
    x[ra, 1, ma] = float("nan")
    x[rb, nc - 1, mb] = float("inf")
    x[rc, int(lab[rc, mc]), mc] = float("inf")      # +inf at the label itself: inf - inf
    ri, mi = ignored[0].tolist()
    x[ri, 0, mi] = float("nan")
    ref = ce_reference(x.numpy(), lab.numpy())
    assert ref["nonfinite"] == 3
    fine = ref["rows"] & np.isfinite(ref["row_loss"])
    got = ce_abi(x.cuda(), lab.cuda())
    compare(got, ref, "ce nonfinite R%d nc%d M%d" % shape, finite_rows=fine)
    assert int(got[1][4]) == 3


# ------------------------------------------------------------------------------------------------ 3. prefix, gout, launches
def test_ce_batch_prefix_rows_are_bit_identical():
    """d is row-local: the first half of the batch alone gives the same dlogits * n_valid rows as inside the whole batch.  Both
    n_valid are powers of two here (16384 rows, 8192 of the whole and 4096 of the prefix count), so dlogits * n_valid is d exactly and
    the comparison is on bits; d itself is compared too."""
    shape = (256, 8, 64)
    logits, labels, _ = make_case(shape, "none_ignored", 1.0, seed=11)
    lab = labels.clone()
    lab[:, ::2] = -1      # every other pixel ignored: half of every sample
    loss, rec, d, dl = ce_abi(logits, lab)
    loss_p, rec_p, d_p, dl_p = ce_abi(logits[:128].contiguous(), lab[:128].contiguous())
    assert int(rec[1]) == 8192 and int(rec_p[1]) == 4096
    assert torch.equal(d[:128].view(torch.int32), d_p.view(torch.int32))
    assert torch.equal((dl[:128] * 8192.0).view(torch.int32), (dl_p * 4096.0).view(torch.int32))
    assert torch.equal((dl * 8192.0).view(torch.int32), d.view(torch.int32))


def test_ce_incoming_gradient_scales_exactly():
    from maskedsst_amd.ops import cross_entropy_stats
    logits, labels, _ = make_case((32, 20, 64), "mixed", 1.0, seed=13)
    x = logits.reshape(32, 20, 8, 8)
    lab = labels.reshape(32, 8, 8)
    a = x.clone().requires_grad_(True)
    cross_entropy_stats(a, lab)[0].backward()
    b = x.clone().requires_grad_(True)
    (3.0 * cross_entropy_stats(b, lab)[0]).backward()
    torch.cuda.synchronize()
    assert a.grad.abs().max() > 0 and torch.equal((3.0 * a.grad).view(torch.int32), b.grad.view(torch.int32))
    # the ABI's optional gout: null is 1
    g1 = ce_abi(logits, labels)[3]
    gt = ce_abi(logits, labels, gout=torch.ones((), device="cuda"))[3]
    assert torch.equal(g1.view(torch.int32), gt.view(torch.int32)) and torch.equal(g1.view(torch.int32), a.grad.reshape(32, 20, 64).view(torch.int32))


def profiled(lib, fn):
    n = lib.msst_profile_kernels()
    ms, cnt = (ctypes.c_double * n)(), (ctypes.c_long * n)()
    torch.cuda.synchronize()
    lib.msst_profile_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
        assert lib.msst_profile_collect(ms, cnt) == 0
    finally:
        lib.msst_profile_enable(0)
    return {lib.msst_profile_name(i).decode(): int(cnt[i]) for i in range(n)}


def test_ce_launch_count():
    """forward + backward of the loss: three launches of the library and nothing else (two without a gradient)"""
    from maskedsst_amd import _lib
    from maskedsst_amd.ops import cross_entropy_stats
    lib = _lib.load()
    logits, labels, _ = make_case((32, 20, 64), "mixed", 1.0)
    x, lab = logits.reshape(32, 20, 8, 8), labels.reshape(32, 8, 8)

    def train():
        a = x.clone().requires_grad_(True)
        cross_entropy_stats(a, lab)[0].backward()

    def evaluate():
        with torch.no_grad():
            cross_entropy_stats(x, lab)

    got = profiled(lib, train)
    assert got["cross_entropy"] == 3 and sum(got.values()) == 3, got
    got = profiled(lib, evaluate)
    assert got["cross_entropy"] == 2 and sum(got.values()) == 2, got


# ------------------------------------------------------------------------------------------------ 4. through the model
def model_batch(head, B=6, n_classes=8):
    size = 7 if head == "pixel" else 8
    gen = torch.Generator().manual_seed(23)
    x = torch.randn(B, 50, size, size, generator=gen)
    label = torch.randint(-1, n_classes, (B,) if head == "pixel" else (B, size, size), generator=gen)
    if head == "pixel":
        label[0] = 3   # at least one valid sample
    return x.cuda(), label.cuda()


@pytest.mark.parametrize("head", ["default", "spectral", "pixel"])
def test_fused_criterion_matches_torch_through_the_model(head):
    """one forward + backward with FusedCrossEntropy and one with torch.nn.CrossEntropyLoss from the same seed and state (fp32 mode,
    dropout 0): acc equal, loss within 1e-4 relative, every parameter gradient within 2e-4 of its tensor's max.
    Gradients, not parameters after a step: Adam's first update is lr * sign(g) and amplifies a last-bit difference near g = 0."""
    from test_gpu_linear_eval import finetune_encoder
    from maskedsst_amd.ops import FusedCrossEntropy
    x, label = model_batch(head)
    out = {}
    for kind in ("torch", "fused"):
        enc = finetune_encoder(head, 50, 2, "fp32", 0.0).cuda().train()
        crit = FusedCrossEntropy(-1) if kind == "fused" else torch.nn.CrossEntropyLoss(ignore_index=-1)
        torch.manual_seed(99)
        logits = enc(x)
        if kind == "fused":
            loss, stats = crit(logits, label, return_stats=True)
            acc = stats.host().acc
        else:
            loss = crit(logits, label)
            valid = label != -1
            acc = float((logits.argmax(dim=1)[valid] == label[valid]).double().mean())
        loss.backward()
        torch.cuda.synchronize()
        out[kind] = (float(loss.detach()), acc, {n: p.grad.detach().double().cpu() for n, p in enc.named_parameters()})
    (lt, at, gt), (lf, af, gf) = out["torch"], out["fused"]
    assert at == af, (at, af)
    loss_err = abs(lf - lt) / abs(lt)
    errs = {n: float((gf[n] - gt[n]).abs().max() / (gt[n].abs().max() + 1e-30)) for n in gt}
    worst = max(errs, key=errs.get)
    print(f"fused vs torch criterion, {head} head: loss rel err {loss_err:.3e}, worst gradient {worst} {errs[worst]:.3e}", flush=True)
    assert loss_err <= 1e-4, (lt, lf)
    assert errs[worst] <= 2e-4, (worst, errs[worst])
    record("fused_criterion_vs_torch", head=head, loss_err=loss_err, worst_grad=errs[worst], worst_grad_name=worst)


def five_steps(kind, head="default"):
    from test_gpu_linear_eval import finetune_encoder
    from maskedsst_amd.config import Dotdict
    from maskedsst_amd.ops import FusedCrossEntropy
    from maskedsst_amd.optim import FusedAdam
    from maskedsst_amd.utils import train_step
    enc = finetune_encoder(head, 50, 2, "fp32", 0.0).cuda().train()
    opt = FusedAdam(enc, lr=1e-3, weight_decay=5e-3)
    crit = FusedCrossEntropy(-1) if kind == "fused" else torch.nn.CrossEntropyLoss(ignore_index=-1)
    cfg = Dotdict(dict(image_size=8, ignored_label=-1, pixelwise=False))
    gen = torch.Generator().manual_seed(41)
    seed_all(77)
    hist = []
    for _ in range(5):
        img = torch.randn(4, 50, 8, 8, generator=gen)
        label = torch.randint(-1, 8, (4, 8, 8), generator=gen)
        loss, acc, macro = train_step(img, label, enc, cfg, torch.device("cuda"), crit, opt)
        hist.append((loss.detach().clone(), float(acc), float(macro), label))
    torch.cuda.synchronize()
    return hist, {k: v.detach().clone() for k, v in enc.state_dict().items()}, enc


def test_two_fused_runs_of_five_train_steps_are_bit_identical():
    """loss and parameters, bit for bit (torch's 2-D NLL sums with float atomics: its loss scalar need not repeat)"""
    h1, p1, _ = five_steps("fused")
    h2, p2, _ = five_steps("fused")
    for (l1, a1, m1, _), (l2, a2, m2, _) in zip(h1, h2):
        assert torch.equal(l1.view(torch.int32), l2.view(torch.int32)) and a1 == a2 and m1 == m2
    assert all(torch.equal(p1[k], p2[k]) for k in p1)
    assert not torch.equal(h1[0][0], h1[-1][0])


def test_train_step_fused_numbers_against_the_eager_path():
    """the first step of both paths starts from the same state: the same acc; loss within 1e-4; macro_acc of the fused path is the
    mean per-class recall (the eager path repeats acc there); a batch without a valid label raises the reference's NaN error"""
    from maskedsst_amd.config import Dotdict
    from maskedsst_amd.ops import FusedCrossEntropy
    from maskedsst_amd.optim import FusedAdam
    from maskedsst_amd.utils import train_step
    hf, _, enc = five_steps("fused")
    ht, _, _ = five_steps("torch")
    (lf, af, mf, label), (lt, at, mt, _) = hf[0], ht[0]
    assert abs(af - at) <= 2.0 ** -24 and mt == at   # (the eager path divides in fp32)
    assert abs(float(lf) - float(lt)) <= 1e-4 * abs(float(lt))
    assert 0.0 <= mf <= 1.0
    # macro accuracy of step 1 from the logits of a fresh model (same seed, same dropout-free forward)
    from test_gpu_linear_eval import finetune_encoder
    fresh = finetune_encoder("default", 50, 2, "fp32", 0.0).cuda().train()
    gen = torch.Generator().manual_seed(41)
    img = torch.randn(4, 50, 8, 8, generator=gen)
    with torch.no_grad():
        pred = fresh(img.cuda()).argmax(dim=1).cpu().numpy()
    lab = label.numpy()
    recall = [float((pred[lab == c] == c).mean()) for c in range(8) if (lab == c).any()]
    assert abs(mf - sum(recall) / len(recall)) <= 1e-12, (mf, recall)
    cfg = Dotdict(dict(image_size=8, ignored_label=-1, pixelwise=False))
    opt = FusedAdam(enc, lr=1e-3)
    before = {k: v.detach().clone() for k, v in enc.state_dict().items()}
    with pytest.raises(ValueError, match="Loss is NaN"):
        train_step(img, torch.full((4, 8, 8), -1), enc, cfg, torch.device("cuda"), FusedCrossEntropy(-1), opt)
    torch.cuda.synchronize()
    assert all(torch.equal(v, before[k]) for k, v in enc.state_dict().items())   # raised before the backward and the optimizer step


# ------------------------------------------------------------------------------------------------ 5. scene validation
def test_scene_metrics_fused_matches_the_eager_path():
    from test_gpu_scene import make_encoder
    from maskedsst_amd.scene import scene_metrics
    enc, scene = make_encoder(dict(bands=50, depth=1, n_classes=6), "bf16", (2, 50, 21, 19))
    classes, logits = enc.cuda().predict_scene(scene.cuda(), return_logits=True)
    assert bool((classes == -1).any()) and bool((classes >= 0).any())   # an uncovered border
    labels = torch.randint(-1, 6, (2, 21, 19), generator=torch.Generator().manual_seed(3)).cuda()
    eager = scene_metrics(logits, classes, labels)
    fused = scene_metrics(logits, classes, labels, fused=True)
    print(f"scene_metrics eager {eager} fused {fused}", flush=True)
    assert abs(fused.acc - eager.acc) <= 1e-12 and abs(fused.macro_acc - eager.macro_acc) <= 1e-12
    assert abs(fused.loss - eager.loss) <= 1e-4 * abs(eager.loss)
    ref = ce_reference(logits.reshape(2, 6, -1).cpu().numpy(), labels.reshape(2, -1).cpu().numpy(), -1, classes.reshape(2, -1).cpu().numpy())
    assert abs(fused.loss - ref["loss"]) <= 1e-4 * abs(ref["loss"]) and abs(fused.acc - ref["n_correct"] / ref["n_valid"]) <= 1e-12
    record("scene_metrics_fused_vs_eager", loss_err=abs(fused.loss - eager.loss) / abs(eager.loss))
    none = torch.full_like(labels, -1)
    for m in (scene_metrics(logits, classes, none), scene_metrics(logits, classes, none, fused=True)):
        assert m.loss != m.loss and m.acc != m.acc and m.macro_acc != m.macro_acc
