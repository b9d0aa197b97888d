"""The linear probe restated in torch float64 (LayerNorm(96) -> Linear -> weighted-mean cross entropy -> torch.optim.Adam), the
deterministic fixtures of tests/test_gpu_probe.py with their conditioning asserts (run on the CPU, so a bad fixture fails here and
not on the GPU), the mutated references that the bars must still tell apart, and the committed bars themselves
(profiles/probe_parity_measured.jsonl: 4 x the error measured on the MI355X)."""
import functools
import json
import os

import torch
import torch.nn.functional as F

from conftest import ROOT

D = 96
GAP = 1e-4             # every row's float64 top-two logit gap exceeds this: the argmax, hence `correct`, is decided
MIN_GRAD_RATIO = 1e-7  # the smallest gradient component stays above this share of the largest: no component sits where g / (|g| + eps) flips
LR, WD, BETAS, EPS = 1e-2, 1e-4, (0.9, 0.999), 1e-8

# (M, n_classes) of the one-launch gradient test: both sides of the 16-row and 16-class MFMA tiles and of the 64-row workgroup tile,
# and more than 32,768 rows: two tiles per workgroup with a ragged end
GRAD_SHAPES = [(1, 2), (15, 3), (17, 5), (64, 16), (65, 17), (300, 5), (513, 33), (1000, 128), (32833, 5)]
GRAD_VARIANTS = ["plain", "weights", "constant_row", "slice"]
# (M, n_classes, batch, class weights?) of the trajectory test
TRAJ_CONFIGS = [(300, 5, None, False), (67, 3, None, True), (1000, 17, 128, False), (513, 33, None, False), (2048, 128, None, False)]
TRAJ_STEPS = [8, 32]
MUTANTS = ["no_weight_decay", "eps_x10", "no_bias_correction", "ln_eps_1e-6", "mean_over_rows"]
PARITY_FILE = os.path.join(ROOT, "profiles", "probe_parity_measured.jsonl")


def n_params(nc):
    return 2 * D + (D + 1) * nc


def split(theta, nc):
    return theta[:D], theta[D:2 * D], theta[2 * D:2 * D + D * nc].view(nc, D), theta[2 * D + D * nc:]


SEGMENTS = ("gamma", "beta", "W", "b")


# ------------------------------------------------------------------------------------------------------------------ fixtures
def make_fixture(M, nc, seed, scale=1.0):
    """labels arange(M) % nc permuted; features 0.6 centre[label] + N(0, 1) + 0.3 per channel, times `scale`, stored fp32; the initial
    theta: gamma 1 + 0.1 N, beta, W, b 0.1 N, rounded to fp32.  -> (x [M, 96] fp32, labels [M] int64, theta0 [192 + 97 nc] fp32)"""
    g = torch.Generator().manual_seed(seed)
    labels = (torch.arange(M) % nc)[torch.randperm(M, generator=g)]
    centre = torch.randn(nc, D, generator=g, dtype=torch.float64)
    x = ((0.6 * centre[labels] + torch.randn(M, D, generator=g, dtype=torch.float64) + 0.3) * scale).float()
    theta0 = torch.cat([1 + 0.1 * torch.randn(D, generator=g, dtype=torch.float64), 0.1 * torch.randn(D, generator=g, dtype=torch.float64),
                        0.1 * torch.randn(nc * D, generator=g, dtype=torch.float64), 0.1 * torch.randn(nc, generator=g, dtype=torch.float64)]).float()
    return x, labels, theta0


def traj_weights(nc):
    """the class weights of the weighted trajectory: positive, unequal"""
    return [0.5 + 0.75 * c for c in range(nc)]


# ---------------------------------------------------------------------------------------------------------- float64 restatement
def forward64(theta, x, nc, ln_eps=1e-5):
    g, b, W, bias = split(theta, nc)
    return F.layer_norm(x.double(), (D,), g, b, ln_eps) @ W.t() + bias


def loss64(theta, x, labels, cw, nc, ln_eps=1e-5, mean_over_rows=False):
    """-> (loss, weight sum, correct, logits): the weighted-mean cross entropy of torch's CrossEntropyLoss(weight=)"""
    logits = forward64(theta, x, nc, ln_eps)
    nll = F.cross_entropy(logits, labels, reduction="none")
    w = torch.ones(len(labels), dtype=torch.float64) if cw is None else torch.as_tensor(cw, dtype=torch.float64)[labels]
    wsum = w.sum()
    loss = (w * nll).sum() / (float(len(labels)) if mean_over_rows else wsum)
    return loss, wsum, int((logits.argmax(dim=1) == labels).sum()), logits


def top_two_gap(logits):
    t = logits.topk(2, dim=1).values if logits.shape[1] > 1 else None
    return float((t[:, 0] - t[:, 1]).min()) if t is not None else float("inf")


def grad64(theta0, x, labels, cw, nc):
    """float64 autograd of one launch: dict loss, weight_sum, correct, gamma, beta, W, b (the four gradients), gap"""
    theta = theta0.double().clone().requires_grad_(True)
    loss, wsum, correct, logits = loss64(theta, x, labels, cw, nc)
    loss.backward()
    out = dict(loss=float(loss.detach()), weight_sum=float(wsum), correct=correct, gap=top_two_gap(logits.detach()))
    out.update(zip(SEGMENTS, split(theta.grad, nc)))
    return out


def adam64(theta0, x, labels, cw, nc, walk, lr=LR, betas=BETAS, eps=EPS, wd=WD, mutant=None, check=False, close_allowed=0):
    """The float64 walk: per step the loss of the parameters as they are on rows [row0, row0 + rows), then Adam by hand in float64
    (tests/test_probe_host.py holds the unmutated walk against torch.optim.Adam).  A step whose weight sum is 0 is skipped whole.
    -> dict history [steps, 4] float64 (loss NaN for a skipped step), theta, m, v, min_gap, min_grad_ratio.
    check: assert the conditioning of the fixture on the way -- every gradient component above MIN_GRAD_RATIO of the largest at every
    step, and every row's top-two logit gap above GAP at every step, except for at most close_allowed row-steps (counted per step in
    `close`: the test lets `correct` differ by at most that many rows at that step, and demands it exact everywhere else)."""
    if mutant == "no_weight_decay":
        wd = 0.0
    if mutant == "eps_x10":
        eps = 10 * eps
    ln_eps = 1e-6 if mutant == "ln_eps_1e-6" else 1e-5
    theta = theta0.double().clone()
    m, v = torch.zeros_like(theta), torch.zeros_like(theta)
    t = 0
    hist = torch.zeros(len(walk), 4, dtype=torch.float64)
    min_gap, min_ratio = float("inf"), float("inf")
    close = []   # per step: the rows whose top-two gap does not exceed GAP (their argmax is not decided at fp32)
    for i, (row0, rows) in enumerate(walk):
        p = theta.clone().requires_grad_(True)
        xs, ys = x[row0:row0 + rows], labels[row0:row0 + rows]
        loss, wsum, correct, logits = loss64(p, xs, ys, cw, nc, ln_eps, mutant == "mean_over_rows")
        min_gap = min(min_gap, top_two_gap(logits.detach()))
        top = logits.detach().topk(2, dim=1).values
        close.append(int(((top[:, 0] - top[:, 1]) <= GAP).sum()))
        if float(wsum) == 0.0:
            hist[i] = torch.tensor([float("nan"), 0.0, correct, rows], dtype=torch.float64)
            continue
        hist[i] = torch.tensor([float(loss.detach()), float(wsum), correct, rows], dtype=torch.float64)
        loss.backward()
        g = p.grad
        min_ratio = min(min_ratio, float(g.abs().min() / g.abs().max()))
        g = g + wd * theta
        t += 1
        m = betas[0] * m + (1 - betas[0]) * g
        v = betas[1] * v + (1 - betas[1]) * g * g
        bc1, bc2 = (1.0, 1.0) if mutant == "no_bias_correction" else (1 - betas[0] ** t, 1 - betas[1] ** t)
        theta = theta - (lr / bc1) * m / (v.sqrt() / bc2 ** 0.5 + eps)
    if check:
        assert close_allowed or min_gap > GAP, f"fixture: a top-two logit gap of {min_gap:.3e} on the walk"
        assert sum(close) <= close_allowed, f"fixture: {sum(close)} row-steps with a top-two gap within {GAP}"
        assert min_ratio > MIN_GRAD_RATIO, f"fixture: a gradient component at {min_ratio:.3e} of the largest"
    return dict(history=hist, theta=theta, m=m, v=v, close=close, min_gap=min_gap, min_grad_ratio=min_ratio, steps_applied=t)


def slice_walk(M, batch, steps):
    from maskedsst_amd.probe import slice_walk as walk
    return walk(M, batch, steps)


# ------------------------------------------------------------------------------------------------------ the fixtures handed out
# Seeds are a property of the inputs alone, found on the CPU with this file: the first at which the conditioning asserts hold.
SEED_BUMP = {("grad", 513, 33): 2, ("grad", 32833, 5): 22, ("traj", 2048, 128): 24, ("fwd", 128, 65): 1}
# 2048 rows x 128 classes x 32 steps are 65,536 row-steps: no seed of 59 tried keeps every top-two gap above GAP there (the smallest
# lies between 1e-6 and 7e-5), so that configuration may hold its three undecided row-steps; the other four hold none.
CLOSE_ALLOWED = {(2048, 128): 3}


def grad_seed(M, nc):
    return 1000 + 7 * M + nc + 100000 * SEED_BUMP.get(("grad", M, nc), 0)


@functools.lru_cache(maxsize=None)
def grad_case(M, nc, variant):
    """-> dict x, labels, theta0, class_w (list or None), row0, rows, ref (grad64 of the slice).  Variants: plain; weights -- one
    class weighs 0 and one class is absent from the bank (its rows are relabelled, so the gradient of its W row comes from p alone);
    constant_row -- one all-constant row (variance 0); slice -- row0 != 0 and an end inside a 16-row tile."""
    x, labels, theta0 = make_fixture(M, nc, grad_seed(M, nc))
    x, labels = x.clone(), labels.clone()
    cw, row0, rows = None, 0, M
    if variant == "weights":
        cw = [0.25 + 0.5 * c for c in range(nc)]
        cw[0] = 0.0
        if nc > 2:
            labels[labels == nc - 1] = 1          # class nc - 1 is absent
        if not bool((labels != 0).any()):
            labels[0] = 1                         # (M = 1: keep one row that weighs something)
    elif variant == "constant_row":
        x[M // 2] = 0.75
    elif variant == "slice":
        row0 = min(3, M - 1)
        rows = max(1, M - row0 - (5 if M > 16 else 0))
    ref = grad64(theta0, x[row0:row0 + rows], labels[row0:row0 + rows], cw, nc)
    assert ref["gap"] > GAP, f"fixture ({M}, {nc}, {variant}): top-two logit gap {ref['gap']:.3e}"
    assert ref["weight_sum"] > 0
    return dict(x=x, labels=labels, theta0=theta0, class_w=cw, row0=row0, rows=rows, ref=ref)


def traj_seed(M, nc):
    return 2000 + 3 * M + nc + 100000 * SEED_BUMP.get(("traj", M, nc), 0)


@functools.lru_cache(maxsize=None)
def traj_case(M, nc, batch, weighted, steps, scale=1.0):
    """-> dict x, labels, theta0, class_w, walk, ref (adam64, conditioning asserted)"""
    x, labels, theta0 = make_fixture(M, nc, traj_seed(M, nc), scale)
    cw = traj_weights(nc) if weighted else None
    walk = slice_walk(M, batch, steps)
    ref = adam64(theta0, x, labels, cw, nc, walk, check=True, close_allowed=CLOSE_ALLOWED.get((M, nc), 0))
    return dict(x=x, labels=labels, theta0=theta0, class_w=cw, walk=walk, ref=ref)


def fwd_seed(nc, Q):
    return 4000 + 10 * nc + Q + 100000 * SEED_BUMP.get(("fwd", nc, Q), 0)


@functools.lru_cache(maxsize=None)
def forward_case(nc, Q):
    """2 Q rows (a map of two scenes with Q pixels each) with NaN rows -- one NaN in all 96 channels, one (Q > 1) in a single channel
    -- and the float64 logits of the others, their top-two gap asserted.  -> dict x [2 Q, 96], theta0, ok [2 Q] bool, ref [ok rows, nc]"""
    x, _, theta0 = make_fixture(2 * Q, nc, fwd_seed(nc, Q))
    nan_rows = sorted({0, (2 * Q) // 3}) if Q > 1 else [1]
    x = x.clone()
    for i, r in enumerate(nan_rows):
        if i == 0:
            x[r] = float("nan")
        else:
            x[r, 17] = float("nan")                                     # one channel is enough
    ok = torch.ones(2 * Q, dtype=torch.bool)
    ok[nan_rows] = False
    ref = forward64(theta0.double(), x[ok], nc)
    assert top_two_gap(ref) > GAP, f"fixture ({nc}, {Q}): top-two logit gap {top_two_gap(ref):.3e}"
    return dict(x=x, theta0=theta0, ok=ok, ref=ref)


def ln_eps_case(steps):
    """the fixture of the LayerNorm-eps mutant: the bank scaled by 0.01 (row variance about 1e-4, where eps 1e-5 against 1e-6 shows)"""
    return traj_case(300, 5, None, False, steps, 0.01)


# ------------------------------------------------------------------------------------------------------------------ comparison
def relmax(got, ref):
    """max abs error over max abs value of the float64 tensor"""
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def grad_errors(grad, row, ref, nc):
    """grad [192 + 97 nc] and row [4] of maskedsst_amd.probe_gradient against grad64 -> {loss, weight_sum, gamma, beta, W, b: error}"""
    err = dict(loss=relmax(row[0], ref["loss"]), weight_sum=relmax(row[1], ref["weight_sum"]))
    for name, g in zip(SEGMENTS, split(torch.as_tensor(grad).double().cpu(), nc)):
        err[name] = relmax(g, ref[name])
    return err


def traj_errors(history, theta, m, v, ref, nc):
    """-> {loss, theta.gamma .. theta.b, m.gamma .., v.gamma ..: error} against adam64 (or, ref against ref, a mutant's distance)"""
    h, rh = torch.as_tensor(history).double().cpu(), ref["history"]
    ok = ~torch.isnan(rh[:, 0])
    err = dict(loss=relmax(h[ok, 0], rh[ok, 0]))
    for what, got in (("theta", theta), ("m", m), ("v", v)):
        for name, a, b in zip(SEGMENTS, split(torch.as_tensor(got).double().cpu(), nc), split(ref[what], nc)):
            err[f"{what}.{name}"] = relmax(a, b)
    return err


# --------------------------------------------------------------------------------------------------------------- committed bars
@functools.lru_cache(maxsize=None)
def measured():
    """{test name: {quantity: the largest error measured on the MI355X over the test's cases}} from the committed file; {} without it"""
    out = {}
    if os.path.exists(PARITY_FILE):
        for line in open(PARITY_FILE):
            if line.strip():
                row = json.loads(line)
                out[row["test"]] = row["measured"]
    return out


def bars(test):
    """4 x the committed measurement per quantity (the project's convention)"""
    m = measured().get(test)
    assert m, f"no committed measurement for {test} in {PARITY_FILE}"
    return {k: 4.0 * val for k, val in m.items()}


def within(err, bar):
    """[(quantity, error, bar)] of the errors above their bar"""
    return [(k, e, bar[k]) for k, e in err.items() if not e <= bar[k]]
