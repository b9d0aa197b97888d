"""GPU: SimMIM masks drawn on the device (msst_draw_masks, SimMIMSpatialSpectral.draw_masks_device, mask_source = "device").

* the kernel against the numpy restatement (tests/mask_util.py), bit for bit in all four outputs, into sentinel-filled buffers with
  sentinel tails; two calls the same bits; a row the same bits whatever row0 and the batch are, 64-bit rows included;
* through the model: a DeviceMasks against the host path on the same masks -- loss and every parameter gradient bit for bit, fp32 and
  bf16, with and without dropout, forward / forward_at with orient / reconstruct;
* no host work on the device path, the device source in use, the host source untouched;
* data parallel placement and gradient accumulation over micro_masks slices."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import oracle_cfg_from, seed_all
from util import build_product, relerr
import mask_util as mu

pytestmark = pytest.mark.gpu

SEED = 20240917
TAIL = 64          # sentinel elements behind every output
S8, S32 = 0xA5, -1515870811   # 0xA5A5A5A5 as int32


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def draw(cfg, lo, hi, seed=SEED):
    """msst_draw_masks for global rows lo .. hi - 1 into sentinel-filled buffers -> the four outputs (mask as uint8), after checking
    that the tails came back untouched and that every element was written"""
    from maskedsst_amd import _lib
    lib = _lib.load()
    rows, T, K = hi - lo, cfg.S * cfg.N, cfg.K
    sizes = (rows * T, rows * K, rows * (T + 1), rows * K)
    bufs = [torch.full((sizes[0] + TAIL,), S8, dtype=torch.uint8, device="cuda")]
    bufs += [torch.full((n + TAIL,), S32, dtype=torch.int32, device="cuda") for n in sizes[1:]]
    rc = lib.msst_draw_masks(*(ctypes.c_void_p(b.data_ptr()) for b in bufs), seed, lo, rows, cfg.S, cfg.N, K, cfg.mode, cfg.rand_size,
                             cfg.scale, cfg.mask_count, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, (rc, lib.msst_last_error())
    torch.cuda.synchronize()
    out = []
    for b, n, sentinel, shape in zip(bufs, sizes, (S8, S32, S32, S32), ((rows, T), (rows, K), (rows, T + 1), (rows, K))):
        h = b.cpu()
        assert (h[n:] == sentinel).all(), "wrote behind an output"
        assert not (h[:n] == sentinel).any(), "left an output element unwritten"
        out.append(h[:n].reshape(shape).numpy())
    return out


def assert_same(got, want, what):
    for name, g, w in zip(("mask", "idx", "csr_ptr", "csr_pos"), got, want):
        assert np.array_equal(g.astype(np.int64), np.asarray(w).astype(np.int64)), (what, name)


# image, S, mask_patch_size, ratio, tube, rows
KERNEL_CASES = [
    (4, 3, 1, 0.5, False, 16),      # A: T = 48
    (6, 7, 1, 0.7, False, 16),      # A: T = 252, no multiple of 64
    (8, 20, 1, 0.5, False, 16),     # A: T = 1280
    (8, 64, 1, 0.5, False, 2),      # A: T = 4096 (N = 64, S = 64)
    (8, 20, 4, 0.7, False, 16),     # B: R = 960 > K = 896, misaligned rows
    (8, 20, 2, 0.5, False, 16),     # B: R = K, aligned
    (4, 3, 2, 0.7, False, 16),      # B: R = 36 > K = 33, duplicates inside index rows
    (8, 20, 4, 0.7, True, 16),      # C: the same three, tube
    (8, 20, 2, 0.5, True, 16),
    (4, 3, 2, 0.7, True, 16),
]


@pytest.mark.parametrize("image,S,mps,ratio,tube,rows", KERNEL_CASES)
def test_kernel_against_the_restatement(image, S, mps, ratio, tube, rows):
    """Duplicates: an index row is the tail of one mask row followed by the head of the next, and a rank's spectral block is
    rank // (trues per block) in every row, so a token can occur twice only where R - K is smaller than the trues per block.  At
    image 8, mask_patch_size 4, S = 20, ratio 0.7 (R - K = 64, 48 per block) no generator can produce one; that case asserts the
    misalignment, and the duplicate is asserted at image 4, mask_patch_size 2, S = 3, ratio 0.7 (R - K = 3, 12 per block)."""
    cfg = mu.make_cfg(image, S, mps, ratio, tube)
    got = draw(cfg, 0, rows)
    want = mu.device_masks(SEED, cfg, 0, rows)
    assert_same(got, want, cfg)
    R, K = mu.trues_per_row(cfg), cfg.K
    assert (got[0].sum(1) == R).all() and (got[2][:, -1] == K).all() and (got[2][:, 0] == 0).all()
    if cfg.mode == mu.TOPK:
        assert (got[3] == np.arange(K)).all() and (np.diff(got[1], axis=1) > 0).all()
    elif R > K:
        own = np.stack([np.nonzero(r)[0][:K] for r in got[0]])
        assert not np.array_equal(got[1][1:], own[1:])                       # index rows cut across mask rows
        if (image, mps) == (4, 2):
            assert any(len(set(r)) < len(r) for r in got[1].tolist())        # a token twice in one index row
            assert np.diff(got[2], axis=1).max() == 2
        else:
            assert R - K >= cfg.mask_count * cfg.scale ** 2 and all(len(set(r)) == len(r) for r in got[1].tolist())
    again = draw(cfg, 0, rows)
    assert_same(again, got, "second call")


@pytest.mark.parametrize("image,S,mps,ratio,tube", [(4, 3, 1, 0.5, False), (8, 20, 4, 0.7, False), (4, 3, 2, 0.7, False), (8, 20, 4, 0.7, True)])
def test_rows_do_not_depend_on_row0_or_the_batch(image, S, mps, ratio, tube):
    cfg = mu.make_cfg(image, S, mps, ratio, tube)
    whole = draw(cfg, 0, 8)
    part = draw(cfg, 5, 8)
    assert_same(part, [w[5:8] for w in whole], "rows 5 .. 7")
    lone = draw(cfg, 7, 8)
    assert_same(lone, [w[7:8] for w in whole], "row 7 alone")
    big = 2 ** 33 + 3
    far = draw(cfg, big, big + 3)
    assert_same(far, mu.device_masks(SEED, cfg, big, big + 3, closed_form=True), "row0 = 2^33 + 3")
    if cfg.mode == mu.TOPK:
        assert not np.array_equal(far[0], whole[0][3:6])                     # the high word of the row counts
    other = draw(cfg, 0, 8, seed=SEED + 1)
    assert not np.array_equal(other[0], whole[0])


# ------------------------------------------------------------------------------------------------------------ through the model
MODEL_CFGS = {
    "A": dict(bands=30, depth=1, B=4, heads=2, image_size=4, mask_patch_size=1, masking_ratio=0.5, tube_masking=False),
    "B": dict(bands=30, depth=1, B=4, heads=2, image_size=4, mask_patch_size=2, masking_ratio=0.7, tube_masking=False),
    "C": dict(bands=20, depth=1, B=3, heads=2),                              # image 8, mask_patch_size 4, tube, ratio 0.7
}


def loss_and_grads(model, call, seed=None):
    model.zero_grad(set_to_none=True)
    if seed is not None:
        torch.manual_seed(seed)
    loss = call()
    loss.backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    model.zero_grad(set_to_none=True)
    return loss.detach().clone(), grads


def assert_same_bits(a, b):
    assert torch.equal(bits(a[0]), bits(b[0])), (a[0].item(), b[0].item())
    assert a[1].keys() == b[1].keys() and len(a[1]) > 4
    for n in a[1]:
        assert torch.equal(bits(a[1][n]), bits(b[1][n])), n


def leaves(x):
    """the tensors of a nest of tuples and lists"""
    if torch.is_tensor(x):
        return [x]
    return [] if x is None else [t for y in x for t in leaves(y)]


def host_pair(dm):
    return dm.bool_mask.cpu(), dm.idx.cpu().long()


@pytest.mark.parametrize("dropout", [0.0, 0.1])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("mode", ["A", "B", "C"])
def test_device_masks_through_the_model(mode, precision, dropout):
    """model(img, masks=dm) against the existing host path on the same masks: loss and every parameter gradient bit for bit; the same
    for forward_at with orient, and all four outputs of reconstruct"""
    from maskedsst_amd import DeviceMasks, random_orients
    cfg = MODEL_CFGS[mode]
    model, _, x = build_product(cfg, precision=precision, device="cuda")
    model.encoder.dropout_p = dropout
    model.train()
    x = x.cuda()
    B = cfg["B"]
    dm = model.draw_masks_device(B, seed=SEED)
    assert isinstance(dm, DeviceMasks) and dm.seed == SEED and dm.row0 == 0 and dm.bool_mask.dtype == torch.bool
    want = mu.device_masks(SEED, mu.cfg_of(model), 0, B)
    assert_same([t.cpu().numpy() for t in dm[:4]], want, "draw_masks_device")
    pair = host_pair(dm)
    a = loss_and_grads(model, lambda: model(x, masks=dm), seed=31)
    assert model.last_masks is dm
    b = loss_and_grads(model, lambda: model(x, masks=pair), seed=31)
    assert_same_bits(a, b)
    # listed windows, oriented: two tiles of 11 x 9, windows anywhere
    s = cfg.get("image_size", 8)
    gen = torch.Generator().manual_seed(3)
    tiles = torch.randn(2, cfg["bands"], s + 3, s + 1, generator=gen).cuda()
    origins = torch.tensor([[i % 2, (2 * i) % 4, i % 2] for i in range(B)], dtype=torch.int32)
    orient = random_orients(B, generator=gen)
    a = loss_and_grads(model, lambda: model.forward_at(tiles, origins, masks=dm, orient=orient), seed=32)
    b = loss_and_grads(model, lambda: model.forward_at(tiles, origins, masks=pair, orient=orient), seed=32)
    assert_same_bits(a, b)
    if dropout == 0.0:
        ra, rb = model.reconstruct(x, masks=dm), model.reconstruct(x, masks=pair)
        for fa, fb in zip(ra, rb):
            assert fa.dtype == fb.dtype and torch.equal(fa, fb)
        ma, mb = model.attention_maps(x, masks=dm), model.attention_maps(x, masks=pair)
        la, lb = leaves(ma), leaves(mb)
        assert len(la) == len(lb) > 0 and all(torch.equal(fa, fb) for fa, fb in zip(la, lb))


def test_no_host_work_on_the_device_path(monkeypatch):
    import maskedsst_amd.masking
    from maskedsst_amd.engine import Engine
    model, _, x = build_product(MODEL_CFGS["B"], precision="bf16", device="cuda")
    x = x.cuda()

    def refuse(*a, **k):
        raise AssertionError("host work on the device path")

    monkeypatch.setattr(maskedsst_amd.masking, "inverse_csr", refuse)
    monkeypatch.setattr(Engine, "_upload", refuse)
    model.mask_source = "device"
    model.train()
    loss = model(x)
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)
    with torch.no_grad():
        assert torch.isfinite(model(x))
    model.zero_grad(set_to_none=True)
    model.mask_source = "host"
    with pytest.raises(AssertionError, match="host work"):
        model(x)


@pytest.mark.parametrize("mode", ["A", "B", "C"])
def test_device_source_in_use(mode):
    from maskedsst_amd import DeviceMasks
    cfg = MODEL_CFGS[mode]
    model, _, x = build_product(cfg, precision="fp32", device="cuda")
    x = x.cuda()
    model.eval()
    # the host source: the parent behaviour, whether the attribute was never touched or set back
    seed_all(11)
    masks = model.draw_masks(cfg["B"])
    with torch.no_grad():
        want = model(x, masks=masks)
        seed_all(11)
        untouched = model(x)
        assert isinstance(model.last_masks, tuple) and not isinstance(model.last_masks, DeviceMasks)
        model.mask_source = "device"
        model.mask_source = "host"
        seed_all(11)
        back = model(x)
        assert torch.equal(bits(want), bits(untouched)) and torch.equal(bits(want), bits(back))
        # the device source: reproduced by torch.manual_seed, changed by another seed
        model.mask_source = "device"
        torch.manual_seed(41)
        l1 = model(x)
        first = model.last_masks
        assert isinstance(first, DeviceMasks) and first.row0 == 0 and first.bool_mask.is_cuda
        torch.manual_seed(41)
        l2 = model(x)
        assert model.last_masks.seed == first.seed and torch.equal(model.last_masks.idx, first.idx)
        torch.manual_seed(42)
        l3 = model(x)
        assert model.last_masks.seed != first.seed
        assert torch.equal(bits(l1), bits(l2)) and not torch.equal(bits(l1), bits(l3))
        assert_same([t.cpu().numpy() for t in first[:4]], mu.device_masks(first.seed, mu.cfg_of(model), 0, cfg["B"]), "forward's draw")
        # the other entry points draw from the device source too
        torch.manual_seed(41)
        rec = model.reconstruct(x)
        assert isinstance(model.last_masks, DeviceMasks) and model.last_masks.seed == first.seed
        assert torch.equal(rec.cube, model.reconstruct(x, masks=first).cube)
        s = cfg.get("image_size", 8)
        tiles = torch.randn(2, cfg["bands"], 2 * s, s + 2, generator=torch.Generator().manual_seed(5)).cuda()
        torch.manual_seed(43)
        lw = model.forward_windows(tiles)
        dmw = model.last_masks
        assert isinstance(dmw, DeviceMasks) and dmw.bool_mask.shape[0] == 4
        origins = torch.tensor([(b, y, 0) for b in range(2) for y in (0, s)], dtype=torch.int32)
        assert torch.equal(bits(lw), bits(model.forward_at(tiles, origins, masks=dmw)))
        torch.manual_seed(44)
        sc = model.reconstruct_scene(tiles)
        assert isinstance(model.last_masks, DeviceMasks) and model.last_masks.bool_mask.shape[0] == 4 and torch.isfinite(sc.cube).all()


# ------------------------------------------------------------------------------------------ data parallel and accumulation
@pytest.mark.parametrize("mode", ["A", "B", "C"])
def test_a_rank_draws_its_rows_of_the_global_batch(mode):
    """one process, the placement set by hand: rank r's draw of b rows is rows [r b, (r + 1) b) of a single-process draw of 4 b"""
    cfg = dict(bands=200, depth=1, B=2, heads=2, mask_patch_size={"A": 1, "B": 4, "C": 4}[mode], masking_ratio=0.5 if mode == "A" else 0.7,
               tube_masking=mode == "C")
    model, _, _ = build_product(cfg, precision="bf16", device="cuda")
    b = 2
    whole = model.draw_masks_device(4 * b, seed=SEED)
    mc = mu.cfg_of(model)
    reached_back = False
    for r in range(4):
        model.dp_rank, model.dp_world = r, 4
        mine = model.draw_masks_device(b, seed=SEED)
        assert mine.row0 == r * b and mine.bool_mask.shape[0] == b
        for got, w in zip(mine[:4], whole[:4]):
            assert torch.equal(got, w[r * b:(r + 1) * b])
        reached_back |= (mc.K * mine.row0) // mu.trues_per_row(mc) < mine.row0     # its index rows start in an earlier rank's mask rows
    model.dp_rank, model.dp_world = 0, 1
    if mode == "B":
        assert mu.trues_per_row(mc) > mc.K and reached_back
    # identically seeded ranks agree on the seed they draw
    torch.manual_seed(9)
    s0 = model.draw_masks_device(b).seed
    model.dp_rank, model.dp_world = 3, 4
    torch.manual_seed(9)
    assert model.draw_masks_device(b).seed == s0
    model.dp_rank, model.dp_world = 0, 1


ACC_CFG = dict(bands=20, depth=1, B=8, heads=2, mask_patch_size=4, masking_ratio=0.7, tube_masking=False)


def test_micro_masks_slices_accumulate_to_the_large_batch():
    """micro_masks slices of one device draw through GradAccumulator against the float64 oracle gradient of the whole batch on the same
    masks, at the fp32 bars of tests/test_gpu_grad_accum.py (loss 1e-4, every parameter gradient 2e-4 of its largest element), and
    against the product's own gradient of the whole batch at the same bar"""
    from maskedsst_amd import GradAccumulator, micro_masks
    from oracle import simmim_forward
    model, params, x = build_product(ACC_CFG, precision="fp32", device="cuda")
    dm = model.draw_masks_device(ACC_CFG["B"], seed=SEED)
    K = 4
    m = ACC_CFG["B"] // K
    whole = loss_and_grads(model, lambda: model(x.cuda(), masks=dm))
    acc = GradAccumulator(model, steps=K)
    losses = []
    for k in range(K):
        part = micro_masks(dm, k, K)
        assert part.row0 == k * m
        loss = model(x[k * m:(k + 1) * m].cuda(), masks=part)
        loss.backward()
        losses.append(loss.detach())
        assert acc.add() == (k == K - 1)
    torch.cuda.synchronize()
    for p in params.values():
        p.requires_grad_(True)
    ref = simmim_forward(params, x, oracle_cfg_from(ACC_CFG), masks=host_pair(dm))
    ref["loss"].backward()
    lr = ref["loss"].item()
    mean_loss = float(torch.stack(losses).double().mean())
    print(f"mean of the micro-losses {mean_loss!r}, oracle {lr!r}, whole batch {whole[0].item()!r}")
    assert abs(mean_loss - lr) <= 1e-4 * abs(lr) and abs(whole[0].item() - lr) <= 1e-4 * abs(lr)
    bad, worst = [], 0.0
    for name, p in model.named_parameters():
        g_ref = params[name].grad
        if g_ref is None:
            assert p.grad is None, name
            continue
        e = max(relerr(p.grad, g_ref), relerr(p.grad, whole[1][name]))
        worst = max(worst, e)
        if not e < 2e-4:
            bad.append((name, e))
    print(f"worst parameter gradient against the oracle and the whole batch: {worst:.3e}")
    assert not bad, bad
