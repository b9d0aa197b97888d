"""GPU: linear evaluation (reference finetune.py:110-136: everything outside mlp_head frozen) and the grouped Adam launch.

* msst_adam_groups against float64 torch.optim.Adam / AdamW, at a bar taken from torch's own fp32 Adam on the same inputs;
* the three head backwards with a null dy: the four head gradients bit for bit those of the call with a dy buffer;
* a linear-eval step against the full backward of an unfrozen copy (logits and head gradients bit-identical, body untouched),
  its launches (no block / tokenizer backward, one optimizer launch) and its memory;
* 30-step trajectories through FusedAdam against the CPU oracle with torch.optim.Adam (linear evaluation and full finetune);
* the optimizer's contract (state_dict round trip, lr changes, foreign gradients, a body unfrozen late) and the script."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, load_golden, oracle_cfg_from, seed_all
from util import record, relerr

pytestmark = pytest.mark.gpu


def ulp32(x):
    """one fp32 unit in the last place of |x| (x float64)"""
    a = x.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def bits(t):
    return t.view(torch.int32)


def backward_nodes(t):
    """names of the autograd nodes behind t"""
    seen, todo, names = set(), [t.grad_fn], set()
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        names.add(type(f).__name__)
        todo += [g for g, _ in f.next_functions]
    return names


# --------------------------------------------------------------------------------------------- 4. the kernel
def adam_groups_call(p, g, m, v, rows, betas=(0.9, 0.999), eps=1e-8, gscale=1.0, group_bytes=None):
    from maskedsst_amd import _lib
    lib = _lib.load()
    G = _lib.MsstAdamGroup
    t = (G * max(1, len(rows)))(*[G(*r) for r in rows])
    P = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    return lib.msst_adam_groups(P(p), P(g), P(m), P(v), t, len(rows), ctypes.sizeof(G) if group_bytes is None else group_bytes,
                                betas[0], betas[1], eps, gscale, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


# (start, end, lr, weight decay, first step, decoupled): lengths 1, 3, 5, 1023 and about 10^6, unaligned starts and ends, holes
ADAM_RANGES = [
    (3, 4, 1e-3, 0.0, 1, 0),
    (9, 12, 5e-3, 5e-3, 4, 0),
    (17, 22, 2e-3, 1e-2, 1, 1),
    (101, 1124, 5e-4, 5e-3, 2, 0),
    (2001, 2001 + 1000003, 5e-3, 5e-3, 1, 0),
    (1002008, 1002008 + 65536, 1e-3, 5e-2, 9, 1),     # 16-byte aligned at both ends
    (1100001, 1100001 + 70001, 1e-2, 0.0, 30, 1),
]


def test_adam_groups_kernel_against_float64_adam():
    """10 steps with fresh gradients over ADAM_RANGES (coupled and decoupled, own lr / wd / step each).  Yardstick: torch.optim.Adam /
    AdamW in float64 on the same slices.  Bar: torch's own fp32 Adam (foreach=False) on the same inputs -- its worst element error
    against the float64 run, per buffer (p, m, v) -- times two, plus one fp32 ulp of the value: both evaluate the same formula in fp32
    and differ only in where they round.  Everything outside the ranges keeps its bits (NaN planted in g, m, v there)."""
    n = 1200000
    gen = torch.Generator().manual_seed(7)
    p0 = torch.randn(n, generator=gen)
    inside = torch.zeros(n, dtype=torch.bool)
    for s, e, *_ in ADAM_RANGES:
        inside[s:e] = True
    nan = float("nan")
    p = p0.cuda()
    m = torch.where(inside, torch.zeros(n), torch.full((n,), nan)).cuda()
    v = m.clone()
    p_before, m_before, v_before = p.clone(), m.clone(), v.clone()

    def torch_side(dtype):
        out = []
        for s, e, lr, wd, step0, dec in ADAM_RANGES:
            q = p0[s:e].to(dtype).clone().requires_grad_(True)
            opt = (torch.optim.AdamW if dec else torch.optim.Adam)([q], lr=lr, weight_decay=wd, foreach=False)
            opt.state[q] = dict(step=torch.tensor(float(step0 - 1)), exp_avg=torch.zeros_like(q), exp_avg_sq=torch.zeros_like(q))
            out.append((q, opt))
        return out

    ref, t32 = torch_side(torch.float64), torch_side(torch.float32)
    for it in range(10):
        g = torch.randn(n, generator=gen) * (0.5 + it)
        for side in (ref, t32):
            for (q, opt), (s, e, *_) in zip(side, ADAM_RANGES):
                q.grad = g[s:e].to(q.dtype).clone()
                opt.step()
        gd = torch.where(inside, g, torch.full((n,), nan)).cuda()
        rows = [(s, e, lr, wd, step0 + it, dec) for s, e, lr, wd, step0, dec in ADAM_RANGES]
        assert adam_groups_call(p, gd, m, v, rows) == 0
    torch.cuda.synchronize()
    out = ~inside.cuda()
    for name, now, before in (("p", p, p_before), ("m", m, m_before), ("v", v, v_before)):
        assert torch.equal(bits(now)[out], bits(before)[out]), f"{name}: an element outside every range changed"
    got = dict(p=p.cpu().double(), m=m.cpu().double(), v=v.cpu().double())
    keys = dict(p=None, m="exp_avg", v="exp_avg_sq")
    worst = {}
    for name, key in keys.items():
        take = lambda side: torch.cat([(q.detach() if key is None else opt.state[q][key]).double() for q, opt in side])  # noqa: E731
        r64, r32 = take(ref), take(t32)
        mine = torch.cat([got[name][s:e] for s, e, *_ in ADAM_RANGES])
        assert torch.isfinite(mine).all()
        err_torch = float((r32 - r64).abs().max())
        excess = float(((mine - r64).abs() - ulp32(r64)).max())
        worst[name] = (float((mine - r64).abs().max()), err_torch, excess)
        print(f"adam_groups {name}: kernel worst abs err {worst[name][0]:.3e}, torch fp32 worst abs err {err_torch:.3e}", flush=True)
    for name, (err, err_torch, excess) in worst.items():
        assert excess <= 2 * err_torch, (name, err, err_torch)
    record("adam_groups_vs_float64", **{f"err_{k}": e[0] for k, e in worst.items()}, **{f"torch_fp32_{k}": e[1] for k, e in worst.items()})


def test_adam_groups_bad_tables_launch_nothing():
    n = 4096
    p = torch.randn(n, device="cuda")
    g, m, v = torch.randn(n, device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    keep = [t.clone() for t in (p, m, v)]
    ok = (0, 64, 1e-3, 0.0, 1, 0)
    from maskedsst_amd._lib import ADAM_MAX_GROUPS
    bad = [[ok, (32, 96, 1e-3, 0.0, 1, 0)], [(64, 128, 1e-3, 0.0, 1, 0), ok], [(0, 64, 1e-3, 0.0, 0, 0)], [(64, 0, 1e-3, 0.0, 1, 0)],
           [(i, i + 1, 1e-3, 0.0, 1, 0) for i in range(ADAM_MAX_GROUPS + 1)]]
    for rows in bad:
        assert adam_groups_call(p, g, m, v, rows) == -3, rows[:2]
    assert adam_groups_call(p, g, m, v, [ok], group_bytes=24) == -3
    assert adam_groups_call(p, g, m, v, []) == 0
    assert adam_groups_call(p, g, m, v, [(7, 7, 1e-3, 0.0, 1, 0)]) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(keep, (p, m, v)))
    assert adam_groups_call(p, g, m, v, [ok]) == 0
    torch.cuda.synchronize()
    assert not torch.equal(p[:64], keep[0][:64]) and torch.equal(p[64:], keep[0][64:])


# --------------------------------------------------------------------------------------------- 5. head backward without dy
NO_DY_CASES = [   # (head, B, S, N, n_classes): both ends of the class-count / S buckets of tests/test_gpu_head_variants.py
    ("spectral", 2, 1, 1, 1), ("spectral", 5, 10, 36, 16), ("spectral", 2, 11, 64, 17), ("spectral", 2, 64, 64, 20),
    ("spectral", 130, 1, 64, 3), ("spectral", 2, 22, 36, 32),
    ("pixel", 1, 1, 1, 1), ("pixel", 17, 10, 49, 9), ("pixel", 33, 22, 49, 32), ("pixel", 2, 64, 49, 5), ("pixel", 65, 42, 9, 31),
    ("default", 1, 1, 1, 1), ("default", 2, 6, 64, 8), ("default", 2, 43, 64, 33), ("default", 4, 64, 64, 40), ("default", 3, 2, 9, 97),
]


@pytest.mark.parametrize("case", NO_DY_CASES, ids=lambda c: "%s-B%d-S%d-N%d-nc%d" % c)
def test_head_backward_without_dy_is_bit_identical(case):
    from test_gpu_head_variants import HEADS, head_encoder
    kind, B, S, N, nc = case
    seed_all(11)
    enc = head_encoder(kind, S, N, nc).cuda()
    eng = enc.engine()
    eng.ensure()
    bwd = {"spectral": eng.spec_head_bwd, "pixel": eng.pix_head_bwd, "default": eng.cls_head_bwd}[kind]
    lin = HEADS[kind]["lin"]
    names = ["mlp_head.0.weight", "mlp_head.0.bias", lin + ".weight", lin + ".bias"]
    gen = torch.Generator(device="cuda").manual_seed(3)
    y = torch.randn(B, S * N, 96, device="cuda", generator=gen) * 2 + 0.5
    dl = torch.randn((B, nc) if kind == "pixel" else (B, nc, N), device="cuda", generator=gen)
    nan = float("nan")
    eng.fp.grad.fill_(nan)
    dy = torch.full_like(y, nan)
    assert bwd(y, dl, dy=dy) is dy
    with_dy = [eng.fp.view(n, eng.fp.grad).clone() for n in names]
    eng.fp.grad.fill_(nan)
    assert bwd(y, dl, want_dy=False) is None
    without = [eng.fp.view(n, eng.fp.grad).clone() for n in names]
    torch.cuda.synchronize()
    assert torch.isfinite(dy).all()
    for n, a, b in zip(names, with_dy, without):
        assert torch.isfinite(b).all(), (n, "not fully written")
        assert torch.equal(a, b), (case, n, float((a - b).abs().max()))


# --------------------------------------------------------------------------------------------- 6. the linear-eval step
HEAD_KW = {"default": {}, "spectral": dict(spectral_mlp_head=True), "pixel": dict(pixelwise=True)}


def finetune_encoder(head, bands, depth, prec, dropout, n_classes=8, seed=5):
    from maskedsst_amd import ViTSpatialSpectral
    seed_all(seed)
    return ViTSpatialSpectral(image_size=7 if head == "pixel" else 8, spatial_patch_size=1, spectral_patch_size=10, num_classes=n_classes,
                              dim=96, depth=depth, heads=8, mlp_dim=64, dropout=dropout, emb_dropout=dropout, channels=bands,
                              spectral_pos_embed=False, spectral_pos=torch.arange(bands // 10), blockwise_patch_embed=True,
                              precision=prec, **HEAD_KW[head])


def freeze_body(enc, frozen=True):
    for n, p in enc.named_parameters():
        p.requires_grad_("mlp_head" in n or not frozen)


def head_items(enc):
    return [(n, p) for n, p in enc.named_parameters() if "mlp_head" in n]


def linear_eval_vs_full(head, bands, depth, prec, dropout, B=4, x=None, label=None):
    """-> (frozen model, logits, loss, dict of what was compared)"""
    size = 7 if head == "pixel" else 8
    full = finetune_encoder(head, bands, depth, prec, dropout).cuda().train()
    lin = finetune_encoder(head, bands, depth, prec, dropout).cuda().train()
    freeze_body(lin)
    if x is None:
        gen = torch.Generator().manual_seed(17)
        x = torch.randn(B, bands, size, size, generator=gen)
        label = torch.randint(-1, 8, (B,) if head == "pixel" else (B, size, size), generator=gen)
        if head == "pixel":
            label = label.clamp_min(0)
    x, label = x.cuda(), label.cuda()

    def loss_of(model):
        torch.manual_seed(99)   # classify draws the dropout seed from the torch generator
        logits = model(x)
        out = logits if logits.dim() > 1 else logits[None]
        return logits, F.cross_entropy(out, label, ignore_index=-1)

    # the premise: the blocks compute the same y whether or not they also save rows for a backward (no_grad forward in training
    # mode against the forward of the full backward, same seed)
    with torch.no_grad():
        logits_ng, _ = loss_of(full)
    logits_f, loss_f = loss_of(full)
    premise = float((logits_ng - logits_f).abs().max())
    loss_f.backward()
    grads_f = {n: p.grad.clone() for n, p in head_items(full)}
    logits_l, loss_l = loss_of(lin)
    eng = lin.engine()
    sentinel = 123.0
    eng.fp.grad.fill_(sentinel)
    loss_l.backward()
    torch.cuda.synchronize()
    grads_l = {n: p.grad.clone() for n, p in head_items(lin)}
    assert "_HeadOnlyFnBackward" in backward_nodes(logits_l) and "_ClassifyFnBackward" in backward_nodes(logits_f)
    # the body: no .grad, and its slice of the flat gradient buffer untouched
    assert all(p.grad is None for n, p in lin.named_parameters() if "mlp_head" not in n)
    hi = max(o + k for nme, (o, k, _) in eng.fp.segments.items() if nme.startswith("mlp_head."))
    assert hi < eng.fp.total and bool((eng.fp.grad[hi:eng.fp.total] == sentinel).all())
    assert not bool((eng.fp.grad[:hi] == sentinel).any())
    diff = dict(logits=float((logits_l - logits_f).abs().max()), **{n: float((grads_l[n] - grads_f[n]).abs().max()) for n in grads_f})
    if premise == 0.0:
        assert torch.equal(logits_l, logits_f), diff
        assert all(torch.equal(grads_l[n], grads_f[n]) for n in grads_f), diff
    else:   # the two existing forwards already differ: compare at 1.5x their difference (relative to the logits' scale)
        tol = 1.5 * premise / float(logits_f.abs().max())
        assert relerr(logits_l, logits_f) <= tol, (premise, diff)
        assert all(relerr(grads_l[n], grads_f[n]) <= tol for n in grads_f), (premise, diff)
    record("linear_eval_vs_full_backward", head=head, bands=bands, depth=depth, precision=prec, dropout=dropout,
           premise_abs_dev=premise, logits_abs_dev=diff["logits"])
    return lin, logits_l, loss_l, x, label


@pytest.mark.parametrize("dropout", [0.0, 0.1])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("head", ["default", "spectral", "pixel"])
def test_linear_eval_step_matches_full_backward(head, prec, dropout):
    linear_eval_vs_full(head, 50, 2, prec, dropout)


@pytest.mark.parametrize("prec,dropout", [("fp32", 0.0), ("bf16", 0.1)])
def test_linear_eval_step_shipped_shape_and_oracle(prec, dropout):
    """200 bands, depth 4 (configs/finetune_config_enmap.yaml with configs/config.yaml); fp32 without dropout: the head gradients
    within the finetune test's 3e-4 of the oracle's, the loss within 1e-4 of the reference's recorded one"""
    from oracle import classify_forward
    g = load_golden("finetune_200b_L4_B2.npz")
    cfg = g["cfg"]
    seed_all(5)
    probe = finetune_encoder("default", cfg["bands"], cfg["depth"], "fp32", 0.0)   # the fixture's draw order: model, x, label
    x = torch.randn(cfg["B"], cfg["bands"], 8, 8)
    label = torch.randint(-1, cfg["n_classes"], (cfg["B"], 8, 8))
    np.testing.assert_array_equal(label.numpy().astype(np.int8), g["label"])
    assert cfg["n_classes"] == 8
    lin, logits, loss, _, _ = linear_eval_vs_full("default", cfg["bands"], cfg["depth"], prec, dropout, x=x, label=label)
    if prec != "fp32" or dropout:
        return
    params = {"encoder." + k: v.detach().clone().requires_grad_("mlp_head" in k) for k, v in probe.state_dict().items()}
    ref_loss = F.cross_entropy(classify_forward(params, x, oracle_cfg_from(cfg)), label, ignore_index=-1)
    ref_loss.backward()
    assert abs(loss.item() - float(g["loss"])) <= 1e-4 * abs(float(g["loss"]))
    errs = {n: relerr(p.grad, params["encoder." + n].grad) for n, p in head_items(lin)}
    assert all(e < 3e-4 for e in errs.values()), errs
    record("linear_eval_head_grads_vs_oracle", **{"err_" + n.replace(".", "_"): e for n, e in errs.items()})


# --------------------------------------------------------------------------------------------- 7. launches
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


BACKWARD_KERNELS = ("block_bwd_attn", "block_bwd_mlp", "block_bwd_ln1", "block_bwd_ln1mlp", "attn_slab_reduce", "tokenize_bwd")


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_linear_eval_launch_accounting(prec):
    from maskedsst_amd.optim import FusedAdam
    depth = 2
    enc = finetune_encoder("default", 50, depth, prec, 0.1).cuda().train()
    opt = FusedAdam(enc, lr=1e-3, weight_decay=5e-3)
    lib = enc.engine().lib
    x = torch.randn(4, 50, 8, 8).cuda()
    label = torch.randint(0, 8, (4, 8, 8)).cuda()

    def step():
        opt.zero_grad()
        F.cross_entropy(enc(x), label).backward()
        opt.step()

    def eval_forward():
        with torch.no_grad():
            enc(x)

    step()   # weight copies, moments
    full = profiled(lib, step)
    freeze_body(enc)
    step()
    lin = profiled(lib, step)
    ev = profiled(lib, eval_forward)
    assert [lin[k] for k in BACKWARD_KERNELS] == [0] * len(BACKWARD_KERNELS), lin
    assert full["block_bwd_attn"] > 0 and full["tokenize_bwd"] > 0 and full["attn_slab_reduce"] + full["reduce_slabs"] > 1, full
    assert full["block_bwd_mlp"] + full["block_bwd_ln1mlp"] > 0 and full["block_bwd_ln1"] + full["block_bwd_ln1mlp"] > 0, full
    assert lin["reduce_slabs"] == 1 < full["reduce_slabs"], (lin, full)     # the head's own partial sums, nothing else
    assert lin["block_fwd"] == 2 * depth and lin["tokenize_fwd"] == ev["tokenize_fwd"] > 0, (lin, ev)
    if prec == "fp32":   # (bf16: an eval forward of so few tiles runs each stack as one launch; the blocks are the same)
        assert lin["block_fwd"] == ev["block_fwd"], (lin, ev)
    assert lin["adam_groups"] == 1 and full["adam_groups"] == 1 and lin["adamw"] == 0, (lin, full)


# --------------------------------------------------------------------------------------------- 8. memory
def test_linear_eval_step_memory():
    """B = 64, 200 bands, depth 4, bf16; A = one fp32 residual stream.  A linear-eval step peaks at two token buffers, the input
    cube (about A / 10), logits and the head's partial sums: at most 4 A, and below a full step (2L+1 fp32 streams and the saved
    bf16 rows: 17 A)."""
    from maskedsst_amd.optim import FusedAdam
    B = 64
    enc = finetune_encoder("default", 200, 4, "bf16", 0.1).cuda().train()
    opt = FusedAdam(enc, lr=1e-3, weight_decay=5e-3)
    x = torch.randn(B, 200, 8, 8).pin_memory()
    label = torch.randint(0, 8, (B, 8, 8)).cuda()
    A = B * 20 * 64 * 96 * 4

    def step():
        opt.zero_grad()
        F.cross_entropy(enc(x.cuda()), label).backward()
        opt.step()

    def peak():
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        step()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    step()
    freeze_body(enc)
    step()
    lin = peak()
    freeze_body(enc, False)
    step()
    full = peak()
    print(f"linear-eval step peak {lin / A:.2f} A, full step peak {full / A:.2f} A (A = {A} bytes)", flush=True)
    record("linear_eval_memory", A_bytes=A, linear_eval_peak_bytes=int(lin), full_peak_bytes=int(full))
    assert lin <= 4 * A, (lin / A, full / A)
    assert lin < full, (lin / A, full / A)


# --------------------------------------------------------------------------------------------- 9 / 10. trajectories
def make_batch(gen, B, bands, n_classes, amp=1.0):
    """the learnable synthetic task of test_gpu_boundary.py::test_config5_short_finetune_accuracy_vs_oracle: every pixel gets a
    random class c and its spectrum a class signature (+amp on band c of every 10-band spectral patch); ~10 % of the pixels ignored"""
    img = torch.randn(B, bands, 8, 8, generator=gen)
    label = torch.randint(0, n_classes, (B, 8, 8), generator=gen)
    onehot = F.one_hot(label, n_classes).permute(0, 3, 1, 2).float()
    pat = torch.zeros(B, 10, 8, 8)
    pat[:, :n_classes] = onehot
    img = img + amp * pat.repeat(1, bands // 10, 1, 1)
    drop = torch.rand(B, 8, 8, generator=gen) < 0.1
    return img, torch.where(drop, torch.full_like(label, -1), label)


def accuracy(logits, y):
    valid = y != -1
    return float((logits.argmax(dim=1)[valid] == y[valid]).float().mean())


def trajectory(shape, linear_eval):
    """-> (oracle losses, oracle accuracy, {prec: (accuracy, losses, model, initial state)}): the oracle with torch.optim.Adam on the
    CPU, the product with FusedAdam, same batches"""
    from oracle import classify_forward
    from maskedsst_amd.optim import FusedAdam
    cfg = dict(bands=shape["bands"], depth=shape["depth"], B=shape["B"], n_classes=8, spectral_pos_embed=False)
    ocfg = oracle_cfg_from(cfg)
    gen = torch.Generator().manual_seed(123)
    batches = [make_batch(gen, cfg["B"], cfg["bands"], 8) for _ in range(shape["steps"])]
    held, held_y = make_batch(gen, 64, cfg["bands"], 8)
    enc = finetune_encoder("default", cfg["bands"], cfg["depth"], "fp32", 0.0)
    params = {"encoder." + k: v.detach().clone().requires_grad_(not linear_eval or "mlp_head" in k) for k, v in enc.state_dict().items()}
    head = [v for k, v in params.items() if "mlp_head" in k]
    body = [v for k, v in params.items() if "mlp_head" not in k]
    if linear_eval:
        opt = torch.optim.Adam(head, lr=5e-3, weight_decay=5e-3)
    else:
        opt = torch.optim.Adam([{"params": body}, {"params": head, "lr": 5e-3}], lr=5e-4, weight_decay=5e-3)
    ref_losses = []
    for img, y in batches:
        opt.zero_grad()
        loss = F.cross_entropy(classify_forward(params, img, ocfg), y, ignore_index=-1)
        loss.backward()
        opt.step()
        ref_losses.append(loss.item())
    with torch.no_grad():
        ref_acc = accuracy(classify_forward(params, held, ocfg), held_y)
    got = {}
    for prec in ("fp32", "bf16"):
        enc = finetune_encoder("default", cfg["bands"], cfg["depth"], prec, 0.0).cuda()
        initial = {k: v.detach().clone() for k, v in enc.state_dict().items()}
        head = [p for n, p in enc.named_parameters() if "mlp_head" in n]
        body = [p for n, p in enc.named_parameters() if "mlp_head" not in n]
        if linear_eval:
            freeze_body(enc)
            opt = FusedAdam(enc, head, lr=5e-3, weight_decay=5e-3)
        else:
            opt = FusedAdam(enc, [{"params": body}, {"params": head, "lr": 5e-3}], lr=5e-4, weight_decay=5e-3)
        enc.train()
        losses = []
        for img, y in batches:
            opt.zero_grad()
            loss = F.cross_entropy(enc(img.cuda()), y.cuda(), ignore_index=-1)
            loss.backward()
            opt.step()
            losses.append(loss.item())
        enc.eval()
        with torch.no_grad():
            acc = accuracy(enc(held.cuda()).cpu(), held_y)
        got[prec] = (acc, losses, enc, initial)
    return ref_losses, ref_acc, got


def test_linear_eval_trajectory_vs_oracle():
    """30 Adam steps on the head alone (lr 5e-3 = the shipped mlp_head_lr, wd 5e-3), body frozen, 80 bands, depth 2, B = 8.  The
    values were chosen on the CPU oracle: with them its loss goes 2.170 -> 1.304 (0.60x) and its held-out accuracy reaches 0.584
    against 0.125 chance, so a linear head on the randomly initialised frozen body does learn in 30 steps."""
    shape = dict(bands=80, depth=2, B=8, steps=30)
    ref_losses, ref_acc, got = trajectory(shape, linear_eval=True)
    record("linear_eval_trajectory", shape=shape, ref_acc=ref_acc, acc_fp32=got["fp32"][0], acc_bf16=got["bf16"][0],
           ref_loss_first=ref_losses[0], ref_loss_last=ref_losses[-1], loss_fp32_last=got["fp32"][1][-1], loss_bf16_last=got["bf16"][1][-1])
    assert ref_losses[-1] < 0.9 * ref_losses[0] and ref_acc > 0.125 + 0.1, (ref_losses[0], ref_losses[-1], ref_acc)
    np.testing.assert_allclose(got["fp32"][1], ref_losses, rtol=2e-3)
    assert abs(got["fp32"][0] - ref_acc) <= 0.01, (got["fp32"][0], ref_acc)
    assert abs(got["bf16"][0] - ref_acc) <= 0.01, (got["bf16"][0], ref_acc)
    for prec, (_, _, enc, initial) in got.items():
        now = enc.state_dict()
        assert all(torch.equal(now[k], initial[k]) for k in now if "mlp_head" not in k), prec
        assert all(not torch.equal(now[k], initial[k]) for k in now if "mlp_head" in k), prec


@pytest.mark.parametrize("shape", [dict(bands=80, depth=2, B=8, steps=30), dict(bands=200, depth=4, B=4, steps=24)],
                         ids=["80b-L2", "shipped-200b-L4"])
def test_full_finetune_trajectory_through_fused_adam(shape):
    """test_config5_short_finetune_accuracy_vs_oracle with the product's optimizer replaced by FusedAdam (lr 5e-4 body / 5e-3 head,
    wd 5e-3): the same bars"""
    ref_losses, ref_acc, got = trajectory(shape, linear_eval=False)
    record("fused_adam_finetune_trajectory", shape=shape, ref_acc=ref_acc, acc_fp32=got["fp32"][0], acc_bf16=got["bf16"][0],
           ref_loss_last=ref_losses[-1], loss_fp32_last=got["fp32"][1][-1], loss_bf16_last=got["bf16"][1][-1])
    assert ref_losses[-1] < 0.6 * ref_losses[0] and 0.4 < ref_acc < 0.97, (ref_losses[0], ref_losses[-1], ref_acc)
    np.testing.assert_allclose(got["fp32"][1], ref_losses, rtol=2e-3)
    assert abs(got["fp32"][0] - ref_acc) <= 0.01, (got["fp32"][0], ref_acc)
    assert abs(got["bf16"][0] - ref_acc) <= 0.01, (got["bf16"][0], ref_acc)


# --------------------------------------------------------------------------------------------- 11. the optimizer's contract
def small_problem(n=5):
    gen = torch.Generator().manual_seed(31)
    return [make_batch(gen, 4, 50, 8) for _ in range(n)]


def ce_rows(logits, y):
    """CE(ignore_index=-1) over pixels as rows: torch's kernel for [B, C, H, W] logits sums the loss with float atomics (the printed
    scalar then moves by an ulp from run to run; the gradient does not), its kernel for [rows, C] reduces in a fixed order"""
    return F.cross_entropy(logits.permute(0, 2, 3, 1).reshape(-1, logits.shape[1]), y.reshape(-1), ignore_index=-1)


def train(enc, opt, batches, criterion=None):
    losses = []
    for img, y in batches:
        opt.zero_grad()
        loss = (criterion or (lambda o, t: F.cross_entropy(o, t, ignore_index=-1)))(enc(img.cuda()), y.cuda())
        loss.backward()
        opt.step()
        losses.append(loss.item())
    return losses


def two_rate(enc):
    head = [p for n, p in enc.named_parameters() if "mlp_head" in n]
    body = [p for n, p in enc.named_parameters() if "mlp_head" not in n]
    return [{"params": body}, {"params": head, "lr": 5e-3}]


def test_fused_adam_state_dict_resumes_bit_identically():
    from maskedsst_amd.optim import FusedAdam
    batches = small_problem()
    enc = finetune_encoder("default", 50, 2, "fp32", 0.0).cuda().train()
    opt = FusedAdam(enc, two_rate(enc), lr=5e-4, weight_decay=5e-3)
    train(enc, opt, batches[:3], ce_rows)
    model_sd = {k: v.detach().clone() for k, v in enc.state_dict().items()}
    opt_sd = opt.state_dict()
    assert sorted(s["step"] for s in opt_sd["state"].values()) == [3] * len(list(enc.parameters()))
    want = train(enc, opt, batches[3:], ce_rows)
    assert sorted(s["step"] for s in opt_sd["state"].values()) == [3] * len(list(enc.parameters()))   # a snapshot, not the live state
    enc2 = finetune_encoder("default", 50, 2, "fp32", 0.0, seed=6).cuda().train()
    enc2.load_state_dict(model_sd)
    opt2 = FusedAdam(enc2, two_rate(enc2), lr=1.0, weight_decay=0.0)   # every hyper-parameter comes back from the state dict
    with pytest.raises(KeyError):
        opt2.load_state_dict({k: v for k, v in opt_sd.items() if k != "fused"})
    bad = dict(opt_sd, fused=dict(m=torch.zeros(3), v=torch.zeros(3)))
    with pytest.raises(ValueError):
        opt2.load_state_dict(bad)
    assert opt2.param_groups[0]["lr"] == 1.0   # a refused load leaves the optimizer as it was
    opt2.load_state_dict(opt_sd)
    assert [g["lr"] for g in opt2.param_groups] == [5e-4, 5e-3]
    assert train(enc2, opt2, batches[3:], ce_rows) == want
    torch.cuda.synchronize()
    now, then = enc2.state_dict(), enc.state_dict()
    assert all(torch.equal(now[k], then[k]) for k in then)


def test_fused_adam_follows_lr_changes_like_torch_adam():
    """synthetic gradients through the flat buffer, lr of both groups changed between steps (what ReduceLROnPlateau does): against
    float64 torch.optim.Adam given the same change, at the kernel test's bar (twice torch's own fp32 error, plus one ulp)"""
    from maskedsst_amd.optim import FusedAdam
    enc = finetune_encoder("default", 50, 2, "fp32", 0.0, n_classes=7).cuda()   # 7 classes: an unaligned head | body boundary
    eng = enc.engine()
    eng.ensure()
    fp = eng.fp
    opt = FusedAdam(enc, two_rate(enc), lr=5e-4, weight_decay=5e-3)
    names = [n for n, _ in enc.named_parameters()]

    def torch_side(dtype):
        ps = {n: p.detach().cpu().to(dtype).clone().requires_grad_(True) for n, p in enc.named_parameters()}
        o = torch.optim.Adam([{"params": [ps[n] for n in names if "mlp_head" not in n]},
                              {"params": [ps[n] for n in names if "mlp_head" in n], "lr": 5e-3}], lr=5e-4, weight_decay=5e-3, foreach=False)
        return ps, o

    (p64, o64), (p32, o32) = torch_side(torch.float64), torch_side(torch.float32)
    gen = torch.Generator().manual_seed(4)
    for it in range(6):
        g = torch.randn(fp.flat.numel(), generator=gen)
        fp.grad.copy_(g)
        for n, p in enc.named_parameters():
            off = (p.data_ptr() - fp.flat.data_ptr()) // 4
            p.grad = fp.grad[off:off + p.numel()].view(p.shape)
            for ps in (p64, p32):
                ps[n].grad = g[off:off + p.numel()].view(p.shape).to(ps[n].dtype).clone()
        if it == 3:
            for o in (opt, o64, o32):
                for grp in o.param_groups:
                    grp["lr"] *= 0.1
        opt.step()
        o64.step()
        o32.step()
    torch.cuda.synchronize()
    mine = torch.cat([p.detach().cpu().double().reshape(-1) for _, p in enc.named_parameters()])
    r64 = torch.cat([p64[n].detach().reshape(-1) for n in names])
    r32 = torch.cat([p32[n].detach().double().reshape(-1) for n in names])
    err, err_torch = float((mine - r64).abs().max()), float((r32 - r64).abs().max())
    assert float(((mine - r64).abs() - ulp32(r64)).max()) <= 2 * err_torch, (err, err_torch)
    record("fused_adam_lr_change_vs_float64", err_p=err, torch_fp32_p=err_torch)


def test_fused_adam_refuses_a_foreign_gradient():
    from maskedsst_amd.optim import FusedAdam
    (img, y), = small_problem(n=1)
    enc = finetune_encoder("default", 50, 2, "fp32", 0.0).cuda().train()
    opt = FusedAdam(enc, lr=5e-4)
    for replace_first in (True, False):   # on the step that builds the table, and on a later one that reuses it
        opt.zero_grad()
        F.cross_entropy(enc(img.cuda()), y.cuda(), ignore_index=-1).backward()
        if not replace_first:
            opt.step()
            opt.zero_grad()
            F.cross_entropy(enc(img.cuda()), y.cuda(), ignore_index=-1).backward()
        p = dict(enc.named_parameters())["mlp_head.1.weight"]
        p.grad = p.grad.clone()
        with pytest.raises(RuntimeError, match="no view of the flat gradient buffer"):
            opt.step()


def test_unfreezing_after_linear_eval_restarts_the_body_at_step_one():
    from maskedsst_amd.optim import FusedAdam
    batches = small_problem(n=4)
    enc = finetune_encoder("default", 50, 2, "fp32", 0.0).cuda().train()
    freeze_body(enc)
    opt = FusedAdam(enc, two_rate(enc), lr=5e-4, weight_decay=5e-3)
    train(enc, opt, batches[:3])
    body = [(n, p) for n, p in enc.named_parameters() if "mlp_head" not in n]
    assert all(p not in opt.state or "step" not in opt.state[p] for _, p in body)
    assert all(opt.state[p]["step"] == 3 for _, p in head_items(enc))
    freeze_body(enc, False)
    img, y = batches[3]
    opt.zero_grad()
    logits = enc(img.cuda())
    assert "_ClassifyFnBackward" in backward_nodes(logits)   # the full backward again
    F.cross_entropy(logits, y.cuda(), ignore_index=-1).backward()
    before = {n: p.detach().double().clone() for n, p in body}
    grads = {n: p.grad.detach().double().clone() for n, p in body}
    assert all(g.abs().max() > 0 for g in grads.values())
    opt.step()
    torch.cuda.synchronize()
    assert all(opt.state[p]["step"] == 1 for _, p in body) and all(opt.state[p]["step"] == 4 for _, p in head_items(enc))
    assert [(r.step, len(r.params)) for r in opt._ranges] == [(5, 4), (2, len(body))]   # the next step's table: head | body
    # torch's first Adam step of a parameter (zero moments, t = 1): p - lr g' / (|g'| + eps), g' = g + wd p.  Bar: one fp32 ulp of
    # the result, plus what the fp32 rounding of g' itself (two roundings: delta = 2 * 2^-23 (|g| + wd |p|)) does to the update,
    # |d update / d g'| = lr eps / (|g'| + eps)^2 -- the update is a steep function of g' where g' is within a few eps of zero
    worst = -1.0
    for n, p in body:
        gp = grads[n] + 5e-3 * before[n]
        want = before[n] - 5e-4 * gp / (gp.abs() + 1e-8)
        delta = 2 * 2.0 ** -23 * (grads[n].abs() + 5e-3 * before[n].abs())
        bar = ulp32(want.cpu()) + (5e-4 * 1e-8 * delta / (gp.abs() + 1e-8) ** 2).cpu() + 1e-9
        worst = max(worst, float(((p.detach().double() - want).abs().cpu() - bar).max()))
    assert worst <= 0, worst


# --------------------------------------------------------------------------------------------- 12. the script
def test_finetune_script_linear_eval_with_fused_adam():
    e = dict(os.environ)
    e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
    cmd = [sys.executable, "finetune.py", "enmap", "--linear-eval", "--optimizer", "fused", "--steps", "10", "--batch-size", "4"]
    r = subprocess.run(cmd, cwd=ROOT, env=e, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, f"--- stdout\n{r.stdout[-4000:]}\n--- stderr\n{r.stderr[-4000:]}"
    last = [l for l in r.stdout.splitlines() if l.startswith("step 10 ")]
    assert last and math.isfinite(float(last[0].split()[3])), r.stdout
