"""GPU: every kernel variant the three classifier heads dispatch to, alone through the engine (cls_head_*, spec_head_*, pix_head_*),
against float64 autograd of the reference formulas (tests/util.py).  The launchers pick a kernel from the problem shape:
  spectral head  spec_head_fwd / _bwd_rows <NQ, RPW> by S (<= 5 / 10 / 21 / 42 / 64), spec_head_wgrad <NCB> by n_classes (<= 8 / 16 / 32),
                 and a static row partition of R = B N into G = min(ceil(R / 32), 128) chunks of RC = ceil(R / G) rows;
  pixelwise head pix_head_logits <NCB> (16 / 8 / 4 samples per workgroup) and pix_head_bwd <NCB> over groups of 32 samples;
  default head   one workgroup per sample, any n_classes (the backward stages dlogits 32 classes at a time).
The cases hit both ends of every bucket.  For each: logits, dy and the four head gradients against float64; outputs prefilled with NaN
(every element is written, nothing accumulated); two backward calls bitwise equal; a prefix of the batch gives the same logit and dy
rows bit for bit (the gradients are summed over a B-dependent partition, so they are not compared)."""
import math

import pytest
import torch

from conftest import seed_all
from util import record, relerr, cls_head_ref, spectral_head_ref, pix_head_ref

pytestmark = pytest.mark.gpu

# (B, S, N, n_classes)
SPEC_CASES = [
    (2, 1, 1, 1),        # NQ 2 (S <= 5), one position, one class
    (3, 5, 9, 3),        # NQ 2 upper end; n_classes not a multiple of 4
    (2, 6, 9, 9),        # NQ 4 lower end; wgrad NCB 16 lower end
    (5, 10, 36, 16),     # NQ 4 upper end; NCB 16 upper end
    (2, 11, 64, 17),     # NQ 8 lower end; NCB 32 lower end
    (3, 21, 9, 31),      # NQ 8 upper end
    (2, 22, 36, 32),     # NQ 16 lower end; n_classes 32
    (1, 42, 64, 8),      # NQ 16 upper end; B = 1
    (2, 43, 9, 5),       # NQ 24 lower end
    (2, 64, 64, 20),     # NQ 24 upper end: LayerNorm over 6144 features
    (1, 64, 1, 1),       # S = 64 at one position
    (3, 32, 36, 1),
    (4, 16, 9, 24),
    (2, 50, 9, 16),
    (7, 4, 36, 12),      # R = 252: G = 8, RC = 32, last chunk 28 rows
    (100, 7, 36, 2),     # R = 3600: G = 113, RC = 32, last chunk 16 rows
    (33, 2, 64, 8),      # R = 2112: G = 66, RC = 32, even
    (130, 1, 64, 3),     # R = 8320: G = 128, RC = 65 (> 64: two row tiles per chunk), even
    (911, 3, 9, 9),      # R = 8199: RC = 65, chunk 126 holds 9 rows, chunk 127 none
    (5000, 1, 9, 4),     # R = 45000: RC = 352, last chunk 296 rows
]

PIX_CASES = [
    (1, 1, 1, 1),        # logits NCB 8: 16 samples per workgroup
    (15, 5, 9, 8),
    (16, 6, 25, 3),
    (17, 10, 49, 9),     # NCB 16: 8 samples per workgroup
    (31, 11, 9, 16),
    (32, 21, 25, 17),    # NCB 32: 4 samples per workgroup; one full backward group
    (33, 22, 49, 32),    # a second backward group of one sample
    (65, 42, 9, 31),     # three groups, the last of one sample
    (65, 43, 1, 8),      # N = 1
    (2, 64, 49, 5),      # S = 64
    (33, 3, 49, 12),
    (7, 64, 25, 32),
    (64, 2, 9, 1),
    (40, 8, 1, 20),
    (1, 30, 49, 16),
    (9, 15, 25, 9),
]

CLS_CASES = [
    (1, 1, 1, 1),
    (3, 5, 9, 3),
    (2, 6, 64, 8),
    (4, 10, 36, 9),
    (2, 11, 16, 16),
    (5, 21, 64, 17),
    (2, 22, 1, 31),
    (3, 42, 49, 32),
    (2, 43, 64, 33),     # n_classes > 32: two dlogits chunks in the backward
    (4, 64, 64, 40),
    (2, 64, 1, 64),
    (6, 3, 25, 64),
    (1, 20, 64, 40),
    (3, 2, 9, 97),       # four chunks, the last of one class
]

# per head: the encoder keyword, the Linear's parameter prefix (the LayerNorm is mlp_head.0) and the reference, logits as the kernels lay them out
HEADS = {
    "spectral": dict(kw=dict(spectral_mlp_head=True), lin="mlp_head.1", ref=lambda y, p, S, N: spectral_head_ref(y, *p, S, math.isqrt(N)).reshape(y.shape[0], -1, N)),
    "pixel": dict(kw=dict(pixelwise=True), lin="mlp_head.2", ref=lambda y, p, S, N: pix_head_ref(y, *p, S, N)),
    "default": dict(kw={}, lin="mlp_head.1", ref=lambda y, p, S, N: cls_head_ref(y, *p, S, N)),
}


def head_encoder(kind, S, N, nc):
    from maskedsst_amd import ViTSpatialSpectral
    return ViTSpatialSpectral(image_size=math.isqrt(N), spatial_patch_size=1, spectral_patch_size=10, num_classes=nc, dim=96, depth=1,
                              heads=2, mlp_dim=64, channels=10 * S, spectral_pos_embed=False, spectral_pos=torch.arange(S),
                              precision="fp32", **HEADS[kind]["kw"])


def run_head(kind, B, S, N, nc):
    seed_all(11)
    enc = head_encoder(kind, S, N, nc)
    lin = HEADS[kind]["lin"]
    names = ["mlp_head.0.weight", "mlp_head.0.bias", lin + ".weight", lin + ".bias"]
    F = enc.state_dict()["mlp_head.0.weight"].numel()
    with torch.no_grad():   # a non-trivial affine LayerNorm and bias
        sd = enc.state_dict()
        sd["mlp_head.0.weight"].copy_(1 + 0.5 * torch.randn(F))
        sd["mlp_head.0.bias"].copy_(0.3 * torch.randn(F))
        sd[lin + ".bias"].copy_(torch.randn(nc))
    enc = enc.cuda()
    eng = enc.engine()
    eng.ensure()
    fwd, bwd = {"spectral": (eng.spec_head_fwd, eng.spec_head_bwd), "pixel": (eng.pix_head_fwd, eng.pix_head_bwd),
                "default": (eng.cls_head_fwd, eng.cls_head_bwd)}[kind]
    lshape = (B, nc) if kind == "pixel" else (B, nc, N)
    gen = torch.Generator(device="cuda").manual_seed(3)
    y = torch.randn(B, S * N, 96, device="cuda", generator=gen) * 2 + 0.5
    dl = torch.randn(lshape, device="cuda", generator=gen)
    nan = float("nan")

    def backward(y_, dl_):
        eng.fp.grad.fill_(nan)
        dy = torch.full_like(y_, nan)
        assert bwd(y_, dl_, dy=dy) is dy
        return dy, [eng.fp.view(n, eng.fp.grad).clone() for n in names]

    logits = torch.full(lshape, nan, device="cuda")
    assert fwd(y, logits=logits) is logits
    dy, grads = backward(y, dl)
    dy2, grads2 = backward(y, dl)
    Bp = max(1, B // 2) if B > 1 else 1
    logits_p = torch.full((Bp,) + lshape[1:], nan, device="cuda")
    fwd(y[:Bp].contiguous(), logits=logits_p)
    dy_p, _ = backward(y[:Bp].contiguous(), dl[:Bp].contiguous())
    torch.cuda.synchronize()
    for what, t in [("logits", logits), ("dy", dy)] + list(zip(names, grads)):
        assert torch.isfinite(t).all(), (what, "not fully written")
    y64 = y.double().requires_grad_(True)
    p64 = [eng.fp.view(n).detach().double().requires_grad_(True) for n in names]
    ref = HEADS[kind]["ref"](y64, p64, S, N)
    ref.backward(dl.double())
    errs = dict(logits=relerr(logits, ref), dy=relerr(dy, y64.grad))
    for n, g, p in zip(names, grads, p64):
        errs[n] = relerr(g, p.grad)
    same = dict(dy=torch.equal(dy, dy2), grads=all(torch.equal(a, b) for a, b in zip(grads, grads2)),
                logits_prefix=torch.equal(logits_p, logits[:Bp]), dy_prefix=torch.equal(dy_p, dy[:Bp]))
    return errs, same


def check(kind, case, bar=1e-4):
    errs, same = run_head(kind, *case)
    assert all(same.values()), (case, same)
    assert all(e < bar for e in errs.values()), (case, errs)
    record(f"head_variants_{kind}", case=list(case), **{"err_" + k.replace(".", "_"): v for k, v in errs.items()})


@pytest.mark.parametrize("case", SPEC_CASES, ids=lambda c: "B%d-S%d-N%d-nc%d" % c)
def test_spectral_head_variants(case):
    check("spectral", case)


@pytest.mark.parametrize("case", PIX_CASES, ids=lambda c: "B%d-S%d-N%d-nc%d" % c)
def test_pixelwise_head_variants(case):
    check("pixel", case)


@pytest.mark.parametrize("case", CLS_CASES, ids=lambda c: "B%d-S%d-N%d-nc%d" % c)
def test_default_head_variants(case):
    check("default", case)


def test_default_head_40_classes_trains():
    """a default-head model with 40 classes: the classifier step's loss.backward() completes (the backward used to refuse more than
    32 classes), its head gradients match float64 autograd of the reference head on the same encoder output within 1e-4, and a
    second step gives bitwise identical gradients"""
    import torch.nn.functional as F
    nc, S = 40, 5
    seed_all(5)
    enc = head_encoder("default", S, 64, nc).cuda()
    x = torch.randn(3, 10 * S, 8, 8).cuda()
    label = torch.randint(-1, nc, (3, 8, 8)).cuda()
    names = ["mlp_head.0.weight", "mlp_head.0.bias", "mlp_head.1.weight", "mlp_head.1.bias"]
    grads = []
    for _ in range(2):
        enc.zero_grad(set_to_none=True)
        logits = enc(x)
        assert logits.shape == (3, nc, 8, 8)
        F.cross_entropy(logits, label, ignore_index=-1).backward()
        torch.cuda.synchronize()
        grads.append({k: p.grad.clone() for k, p in enc.named_parameters() if k in names})
    assert all(torch.equal(grads[0][k], grads[1][k]) for k in names)
    # the head against float64 on the encoder output (the fused eval forward_features: the same kernels, fp32 round-off apart)
    with torch.no_grad():
        y = enc.engine().features(x)
    sd = dict(enc.named_parameters())
    y64 = y.double().requires_grad_(True)
    p64 = [sd[n].detach().double().requires_grad_(True) for n in names]
    ref = cls_head_ref(y64, *p64, S, 64).reshape(3, nc, 8, 8)
    F.cross_entropy(ref, label, ignore_index=-1).backward()
    errs = {n: relerr(grads[0][n], p.grad) for n, p in zip(names, p64)}
    errs["logits"] = relerr(logits, ref)
    assert all(e < 1e-4 for e in errs.values()), errs
    record("default_head_40_classes_trains", **{"err_" + k.replace(".", "_"): v for k, v in errs.items()})
