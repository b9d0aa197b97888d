"""GPU: gradient accumulation and the global-norm clip on the flat buffers.

* msst_grad_accumulate / msst_grad_finalize on torch buffers: the sums bit for bit those torch forms in fp32, the norm and the clipped
  gradient against a float64 restatement, nothing outside the ranges touched, two calls the same bits, non-finite values counted;
* ``GradAccumulator`` end to end in fp32 without dropout: K micro-batches against the torch-formed mean of their gradients (bit for bit)
  and against the float64 oracle gradient of the whole batch, linear evaluation, the hand-off to ``FusedAdamW``, ``steps=1`` against
  ``clip_grad_norm_``, and what it refuses."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from conftest import oracle_cfg_from, seed_all
from util import build_product, relerr

pytestmark = pytest.mark.gpu

SENTINEL = -7777.25
BIG = 4 * 256 * 2048 + 7      # more than one trip of the launches' strided loop (512 workgroups x 256 lanes x four float4)

# range tables: one range of length 1, 3, 4, 5, 1023 and BIG; ranges that start at element 1, 2 and 3 with unaligned heads and tails;
# three ranges with holes, the middle one shorter than 4
TABLES = {
    "len1": [(8, 9)], "len3": [(8, 11)], "len4": [(8, 12)], "len5": [(8, 13)], "len1023": [(8, 1031)], "big": [(0, BIG)],
    "start1": [(1, 1 + 1030)], "start2": [(2, 2 + 517)], "start3": [(3, 3 + 2050)],
    "holes": [(5, 130), (133, 135), (141, 1500)],
}


def bits(t):
    return t.view(torch.int32)


def lib_and_table(rows):
    from maskedsst_amd import _lib
    G = _lib.MsstGradRange
    return _lib.load(), (G * len(rows))(*[G(a, b) for a, b in rows]), ctypes.sizeof(G)


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def accumulate(acc, g, rows, first, out=None, scale=1.0, scratch=None):
    lib, t, nbytes = lib_and_table(rows)
    rc = lib.msst_grad_accumulate(P(acc), P(g), t, len(rows), nbytes, int(first), P(out), scale, P(scratch), stream())
    assert rc == 0, (rc, lib.msst_last_error())


def finalize(acc, g, rows, scale, max_norm, scratch, record):
    lib, t, nbytes = lib_and_table(rows)
    rc = lib.msst_grad_finalize(P(acc), P(g), t, len(rows), nbytes, scale, max_norm, P(scratch), P(record), stream())
    assert rc == 0, (rc, lib.msst_last_error())


def new_scratch(rows):
    """a scratch of the size the library asks for, filled with a pattern: nothing has to be zeroed beforehand"""
    from maskedsst_amd import _lib
    n = _lib.load().msst_grad_accum_scratch_bytes(len(rows))
    assert n > 0 and n % 8 == 0
    return torch.full((n // 8,), 0x5555555555555555, dtype=torch.int64, device="cuda")


def mixed(n, gen):
    """random fp32 values of mixed magnitude, 1e-6 .. 1e3, both signs"""
    mag = 10.0 ** (torch.rand(n, generator=gen, device="cuda", dtype=torch.float64) * 9.0 - 6.0)
    sign = torch.where(torch.rand(n, generator=gen, device="cuda") < 0.5, -1.0, 1.0)
    return (mag * sign).float()


def size_of(rows):
    return (rows[-1][1] + 19) // 4 * 4


def inside(rows, n):
    m = torch.zeros(n, dtype=torch.bool, device="cuda")
    for a, b in rows:
        m[a:b] = True
    return m


@pytest.mark.parametrize("name", list(TABLES))
def test_accumulate_is_the_fp32_sum_bit_for_bit(name):
    rows = TABLES[name]
    n = size_of(rows)
    gen = torch.Generator(device="cuda").manual_seed(7)
    g1, g2, g3 = (mixed(n, gen) for _ in range(3))
    m = inside(rows, n)
    scale = 0.3
    acc = torch.full((n,), SENTINEL, device="cuda")
    out = torch.full((n,), SENTINEL, device="cuda")
    keep = [t.clone() for t in (g1, g2, g3)]
    accumulate(acc, g1, rows, first=1)
    assert torch.equal(bits(acc[m]), bits(g1[m]))
    accumulate(acc, g2, rows, first=0)
    accumulate(acc, g3, rows, first=0, out=out, scale=scale)
    want = (g1 + g2) + g3
    want_out = want * torch.tensor(scale, dtype=torch.float32, device="cuda")
    assert torch.equal(bits(acc[m]), bits(want[m]))
    assert torch.equal(bits(out[m]), bits(want_out[m]))
    # nothing outside the ranges is written, in any buffer; the gradients are only read
    assert bool((acc[~m] == SENTINEL).all()) and bool((out[~m] == SENTINEL).all())
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip((g1, g2, g3), keep))
    # out == g: every element is read before it is written
    acc2 = torch.full((n,), SENTINEL, device="cuda")
    accumulate(acc2, g1, rows, first=1)
    accumulate(acc2, g2, rows, first=0)
    g3c = g3.clone()
    accumulate(acc2, g3c, rows, first=0, out=g3c, scale=scale)
    assert torch.equal(bits(acc2[m]), bits(want[m])) and torch.equal(bits(g3c[m]), bits(want_out[m]))
    assert torch.equal(bits(g3c[~m]), bits(g3[~m])) and bool((acc2[~m] == SENTINEL).all())
    # first with out: the scaled copy
    out3 = torch.full((n,), SENTINEL, device="cuda")
    accumulate(acc2, g2, rows, first=1, out=out3, scale=scale)
    assert torch.equal(bits(acc2[m]), bits(g2[m]))
    assert torch.equal(bits(out3[m]), bits((g2 * torch.tensor(scale, dtype=torch.float32, device="cuda"))[m]))


def norm_setup(rows, seed=11):
    n = size_of(rows)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    src = mixed(n, gen)
    src[rows[0][0]] = 517.25   # the norm stays far above clip_grad_norm_'s 1e-6, so that a clipped gradient's norm is max_norm
    acc = torch.full((n,), SENTINEL, device="cuda")
    scratch = new_scratch(rows)
    accumulate(acc, src, rows, first=1, scratch=scratch)
    return n, src, acc, scratch


@pytest.mark.parametrize("name", list(TABLES))
def test_finalize_against_float64(name):
    """record[0] carries one fp32 rounding of a double sum (6e-8), (acc * scale) * coef at most four fp32 roundings (2.4e-7): rtol 1e-6"""
    rows = TABLES[name]
    n, src, acc, scratch = norm_setup(rows)
    m = inside(rows, n)
    scale = 0.25 if name != "start2" else 1.0 / 3.0
    scale32 = torch.tensor(scale, dtype=torch.float32)
    a64 = acc[m].double()
    norm64 = float(scale32.double()) * float(a64.pow(2).sum().sqrt())
    assert norm64 > 100.0
    # max_norm above the norm, and no clip at all: coef == 1.0 exactly, g = acc * scale bit for bit
    for max_norm in (2.0 * norm64, 0.0):
        g = torch.full((n,), SENTINEL, device="cuda")
        rec = torch.full((4,), SENTINEL, device="cuda")
        finalize(acc, g, rows, scale, max_norm, scratch, rec)
        r = rec.tolist()
        print(f"{name}: norm {r[0]!r} (float64 {norm64!r}, rel {abs(r[0] - norm64) / norm64:.2e}), coef {r[1]!r}")
        assert abs(r[0] - norm64) <= 1e-6 * norm64
        assert r[1] == 1.0 and r[2] == 0.0 and r[3] == 0.0
        assert torch.equal(bits(g[m]), bits((acc * scale32.cuda())[m]))
        assert bool((g[~m] == SENTINEL).all()) and bool((acc[~m] == SENTINEL).all())
    # max_norm below the norm
    max_norm = norm64 / 3.0
    g = torch.full((n,), SENTINEL, device="cuda")
    rec = torch.full((4,), SENTINEL, device="cuda")
    finalize(acc, g, rows, scale, max_norm, scratch, rec)
    r = rec.tolist()
    max32 = float(torch.tensor(max_norm, dtype=torch.float32))
    coef64 = max32 / (norm64 + 1e-6)
    want = a64 * float(scale32.double()) * coef64
    err = float(((g[m].double() - want).abs() / want.abs()).max())
    gnorm = float(g[m].double().pow(2).sum().sqrt())
    print(f"{name}: clipped: coef {r[1]!r} (float64 {coef64!r}), worst element rel {err:.2e}, |g| {gnorm!r} vs max_norm {max32!r}")
    assert abs(r[0] - norm64) <= 1e-6 * norm64 and abs(r[1] - coef64) <= 1e-6 * coef64
    assert err <= 1e-6
    assert abs(gnorm - max32) <= 1e-6 * max32
    assert bool((g[~m] == SENTINEL).all())


@pytest.mark.parametrize("name", ["len5", "holes", "big"])
def test_two_calls_give_the_same_bits(name):
    rows = TABLES[name]
    outs = []
    for _ in range(2):
        n, src, acc, scratch = norm_setup(rows)
        g = torch.full((n,), SENTINEL, device="cuda")
        rec = torch.full((4,), SENTINEL, device="cuda")
        finalize(acc, g, rows, 0.25, 3.0, scratch, rec)
        outs.append((bits(g).clone(), bits(rec).clone(), scratch.clone()))
    torch.cuda.synchronize()
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert not torch.equal(outs[0][2], torch.full_like(outs[0][2], 0x5555555555555555))


@pytest.mark.parametrize("name", ["len1023", "holes", "big"])
def test_nonfinite_values_are_counted(name):
    rows = TABLES[name]
    n = size_of(rows)
    gen = torch.Generator(device="cuda").manual_seed(3)
    src = mixed(n, gen)
    a, b = rows[-1]
    src[rows[0][0]] = float("nan")          # a ragged head or the first aligned piece
    src[b - 1] = float("inf")               # the tail
    src[(a + b) // 2] = float("-inf")       # the interior
    src[rows[-1][1] + 1] = float("nan")     # outside every range: not counted
    acc = torch.full((n,), SENTINEL, device="cuda")
    scratch = new_scratch(rows)
    accumulate(acc, src, rows, first=1, scratch=scratch)
    g = torch.full((n,), SENTINEL, device="cuda")
    rec = torch.zeros(4, device="cuda")
    finalize(acc, g, rows, 1.0, 1.0, scratch, rec)
    assert rec[2].item() == 3.0


# ----------------------------------------------------------------------------------------------- GradAccumulator, end to end
CFG = dict(bands=20, depth=1, B=8, heads=2)


def micro_cycle(model, x, masks, K, acc, dp_scale=1.0):
    """K micro-batches through acc; -> (clones of the K flat micro-gradients, micro-losses, what the last add() returned)"""
    from maskedsst_amd import micro_masks
    fp = model.engine().fp
    m = x.shape[0] // K
    clones, losses, ready = [], [], None
    for k in range(K):
        loss = model(x[k * m:(k + 1) * m].cuda(), masks=micro_masks(masks, k, K))
        loss.backward()
        clones.append(fp.grad.clone())
        losses.append(loss.detach())
        ready = acc.add(dp_scale=dp_scale)
        assert ready == (k == K - 1)
    return clones, losses, ready


def test_four_micro_batches_are_the_mean_and_the_whole_batch_gradient():
    from maskedsst_amd import GradAccumulator
    from oracle import simmim_forward
    model, params, x = build_product(CFG, precision="fp32", device="cuda")
    masks = model.draw_masks(CFG["B"])
    acc = GradAccumulator(model, steps=4)
    clones, losses, _ = micro_cycle(model, x, masks, 4, acc)
    fp = model.engine().fp
    n = fp.n_trainable
    want = (((clones[0] + clones[1]) + clones[2]) + clones[3]) * 0.25
    torch.cuda.synchronize()
    assert torch.equal(bits(fp.grad[:n]), bits(want[:n]))
    assert torch.equal(bits(fp.accum[:n]), bits((((clones[0] + clones[1]) + clones[2]) + clones[3])[:n]))
    # the float64 oracle on the whole batch of 8 with the same masks (tests/test_gpu_backward.py::test_param_grads_fp32 and its bar)
    for p in params.values():
        p.requires_grad_(True)
    ref = simmim_forward(params, x, oracle_cfg_from(CFG), masks=masks)
    ref["loss"].backward()
    lr = ref["loss"].item()
    mean_loss = float(torch.stack(losses).double().mean())
    print(f"mean of the micro-losses {mean_loss!r}, oracle {lr!r}")
    assert abs(mean_loss - lr) <= 1e-4 * abs(lr)
    bad, worst = [], 0.0
    for name, p in model.named_parameters():
        g_ref = params[name].grad
        if g_ref is None:
            assert p.grad is None, name
            continue
        # the parameters keep their views of the flat gradient buffer
        assert p.grad is not None and p.grad.data_ptr() - fp.grad.data_ptr() == p.data_ptr() - fp.flat.data_ptr(), name
        e = relerr(p.grad, g_ref)
        worst = max(worst, e)
        if not e < 2e-4:
            bad.append((name, e))
    print(f"worst parameter gradient against the oracle: {worst:.3e}")
    assert not bad, bad


def test_linear_eval_touches_the_head_range_only():
    from maskedsst_amd import GradAccumulator, ViTSpatialSpectral
    seed_all(5)
    enc = ViTSpatialSpectral(image_size=8, spatial_patch_size=1, spectral_patch_size=10, num_classes=8, dim=96, depth=1, heads=2, mlp_dim=64,
                             dropout=0.0, emb_dropout=0.0, channels=20, spectral_pos_embed=False, spectral_pos=torch.arange(2),
                             blockwise_patch_embed=True, precision="fp32").cuda().train()
    for name, p in enc.named_parameters():
        p.requires_grad_("mlp_head" in name)
    gen = torch.Generator().manual_seed(17)
    x = torch.randn(4, 20, 8, 8, generator=gen).cuda()
    label = torch.randint(-1, 8, (4, 8, 8), generator=gen).cuda()
    eng = enc.engine()
    eng.ensure()
    fp = eng.fp
    fp.grad.fill_(SENTINEL)
    fp.accum_buffer().fill_(SENTINEL)
    acc = GradAccumulator(enc, steps=2, track_norm=True)
    clones = []
    for k in range(2):
        loss = F.cross_entropy(enc(x[2 * k:2 * k + 2]), label[2 * k:2 * k + 2], ignore_index=-1)
        loss.backward()
        clones.append(fp.grad.clone())
        assert acc.add() == (k == 1)
    hi = max(o + c for nme, (o, c, _) in fp.segments.items() if nme.startswith("mlp_head."))
    assert 0 < hi < fp.total
    torch.cuda.synchronize()
    assert bool((fp.grad[hi:] == SENTINEL).all()) and bool((fp.accum[hi:] == SENTINEL).all())
    want = (clones[0] + clones[1]) * 0.5
    assert torch.equal(bits(fp.grad[:hi]), bits(want[:hi]))
    assert all(p.grad is None for name, p in enc.named_parameters() if "mlp_head" not in name)
    norm, coef, bad = acc.record()
    norm64 = float(want[:hi].double().pow(2).sum().sqrt())   # the head alone: the sentinels of the body would dwarf it
    assert abs(norm - norm64) <= 1e-6 * norm64 and coef == 1.0 and bad == 0


def test_fused_adamw_steps_on_the_accumulated_mean():
    from maskedsst_amd import GradAccumulator
    from maskedsst_amd.optim import FusedAdamW
    model, _, x = build_product(CFG, precision="fp32", device="cuda")
    masks = model.draw_masks(CFG["B"])
    opt = FusedAdamW(model, lr=1e-3, weight_decay=1e-2, grad_clamp=1.0)
    clones, _, _ = micro_cycle(model, x, masks, 2, GradAccumulator(model, steps=2))
    opt.step()
    opt.zero_grad()
    # the same step on a gradient buffer filled by hand with the torch-formed mean of the same two micro-gradients
    other, _, _ = build_product(CFG, precision="fp32", device="cuda")
    from maskedsst_amd import micro_masks
    other(x[:4].cuda(), masks=micro_masks(masks, 0, 2)).backward()
    fp = other.engine().fp
    fp.grad.copy_((clones[0] + clones[1]) * 0.5)
    opt2 = FusedAdamW(other, lr=1e-3, weight_decay=1e-2, grad_clamp=1.0)
    opt2.step()
    torch.cuda.synchronize()
    moved = 0
    before = dict(build_product(CFG, precision="fp32")[0].named_parameters())
    for (name, p), (_, q) in zip(model.named_parameters(), other.named_parameters()):
        assert torch.equal(bits(p.detach()), bits(q.detach())), name
        moved += int(not torch.equal(p.detach().cpu(), before[name].detach()))
    assert moved > 10


def test_one_step_with_max_norm_is_clip_grad_norm():
    from maskedsst_amd import GradAccumulator
    model, _, x = build_product(CFG, precision="fp32", device="cuda")
    masks = model.draw_masks(CFG["B"])
    model(x.cuda(), masks=masks).backward()
    named = [(name, p) for name, p in model.named_parameters() if p.grad is not None]
    twins = [torch.nn.Parameter(torch.zeros_like(p)) for _, p in named]
    for t, (_, p) in zip(twins, named):
        t.grad = p.grad.clone()
    unclipped = float(torch.nn.utils.clip_grad_norm_(twins, 1e30))
    max_norm = 0.5 * unclipped
    total = float(torch.nn.utils.clip_grad_norm_(twins, max_norm))
    acc = GradAccumulator(model, steps=1, max_norm=max_norm)
    assert acc.add() is True
    norm, coef, bad = acc.record()
    print(f"norm {norm!r}, clip_grad_norm_ {total!r}; coef {coef!r}")
    assert abs(norm - total) <= 1e-6 * total and bad == 0
    assert abs(coef - max_norm / (total + 1e-6)) <= 1e-6 * coef
    for t, (name, p) in zip(twins, named):
        assert torch.allclose(p.grad, t.grad, rtol=1e-6, atol=0.0), (name, relerr(p.grad, t.grad))


def test_what_is_refused():
    from maskedsst_amd import GradAccumulator, micro_masks
    model, _, x = build_product(CFG, precision="fp32", device="cuda")
    masks = model.draw_masks(CFG["B"])
    acc = GradAccumulator(model, steps=2)
    with pytest.raises(RuntimeError, match="backward"):   # add() before any backward
        acc.add()
    assert acc.count == 0
    half = lambda k: model(x[4 * k:4 * k + 4].cuda(), masks=micro_masks(masks, k, 2))  # noqa: E731
    half(0).backward()
    with pytest.raises(RuntimeError, match="accumulation"):   # a second backward without add() in between: still refused
        half(1).backward()
    assert acc.add() is False
    # a changed frozen pattern inside the cycle
    model.encoder.to_patch_embedding.pre_norm.weight.requires_grad_(False)
    half(1).backward()
    with pytest.raises(RuntimeError, match="changed inside an accumulation cycle"):
        acc.add()
    acc.reset()
    assert acc.add() is False   # the same gradients open a new cycle
    with pytest.raises(ValueError):
        GradAccumulator(model, steps=0)
    with pytest.raises(ValueError):
        GradAccumulator(model, max_norm=0.0)
