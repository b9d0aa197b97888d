"""Input gradients, host side (no GPU needed): the oracle's img.grad against the reference's fixture value, the float64 restatement of
the loss's target term, the helpers of maskedsst_amd.saliency on stub models, and the C ABI of the three new entry points (additive
under MSST_VERSION 109)."""
import ctypes
import re
import subprocess

import pytest
import torch

from util import relerr
from input_grad_util import CASES, QUIRK, fixture, oracle_run, target_term_ref, with_duplicates

BADARG, UNSUPPORTED = -3, -2
CALLS = {"msst_tokenize_bwd_input": 18, "msst_head_bwd_target": 11, "msst_tokenize_scene_bwd_input": 21}


@pytest.mark.parametrize("name", CASES)
def test_oracle_img_grad_matches_the_reference(name):
    """pins the comparison value of the GPU tests: fp32 on the CPU both sides"""
    fx, got = fixture(name), oracle_run(name)
    assert abs(got["loss"] - fx["loss"]) <= 1e-5 * abs(fx["loss"])
    err = relerr(got["img_grad"], fx["img_grad"])
    assert err <= 1e-5, err


def test_target_term_restatement_and_the_index_quirk():
    """the target term alone: autograd of the L1 loss with the encoder output held fixed equals the index_add restatement, on the
    fixture's indices (a row names tokens of another row's mask) and on a variant in which a token is named three times"""
    fx = fixture(QUIRK)
    cfg = fx["cfg"]
    S, N, P = cfg["bands"] // 10, 64, 10
    bm, idx = fx["bool_mask"], fx["idx"]
    B, K = idx.shape
    foreign = [b for b in range(B) if (~bm[b][idx[b]]).any()]
    assert foreign, "no row of the quirk fixture names a token outside its own mask"
    dup = with_duplicates(idx, S * N)
    assert any(len(set(r.tolist())) < K for r in dup)
    gen = torch.Generator().manual_seed(3)
    for ix in (idx, dup):
        x = fx["x"].double().clone().requires_grad_(True)
        pred = torch.randn(B, K, P, generator=gen, dtype=torch.float64)
        patches = x.reshape(B, S, P, N).permute(0, 1, 3, 2).reshape(B, S * N, P)
        target = patches[torch.arange(B)[:, None], ix]
        ((pred - target).abs().mean() / K).backward()
        want = target_term_ref(torch.sign(pred - target).detach(), ix, S, N, P).reshape(x.shape)
        assert relerr(want, x.grad) <= 1e-12


class _Linear(torch.nn.Module):
    """logits[b, k, h, w] = sum_c w[k, c] x[b, c, h, w] + bias[k]: integrated gradients are exact for it"""

    def __init__(self, nc=4, C=6):
        super().__init__()
        g = torch.Generator().manual_seed(1)
        self.w = torch.nn.Parameter(torch.randn(nc, C, generator=g, dtype=torch.float64))
        self.b = torch.nn.Parameter(torch.randn(nc, generator=g, dtype=torch.float64))

    def forward(self, x):
        return torch.einsum("kc,bchw->bkhw", self.w, x) + self.b.view(1, -1, 1, 1)


def test_helpers_on_a_stub_model():
    from maskedsst_amd import input_gradient, band_importance, integrated_gradients
    m = _Linear()
    x = torch.randn(3, 6, 5, 5, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    # flags, mode and .grad are left as found
    m.w.requires_grad_(False)
    m.b.grad = torch.ones_like(m.b)
    m.train()
    g = input_gradient(m, x, 2)
    assert m.training and not m.w.requires_grad and m.b.requires_grad and m.w.grad is None and torch.equal(m.b.grad, torch.ones(4).double())
    assert not x.requires_grad and g.shape == x.shape
    assert torch.allclose(g, m.w[2].detach().view(1, 6, 1, 1).expand_as(x))
    # per-sample and per-position targets, -1 = skip
    g = input_gradient(m, x, torch.tensor([0, 1, 3]))
    assert torch.allclose(g[1], m.w[1].detach().view(6, 1, 1).expand(6, 5, 5))
    t = torch.full((3, 5, 5), -1)
    t[0, 2, 3] = 1
    g = input_gradient(m, x, t)
    assert torch.allclose(g[0, :, 2, 3], m.w[1].detach()) and float(g.abs().sum()) == pytest.approx(float(m.w[1].abs().sum()))
    assert torch.equal(input_gradient(m, x), input_gradient(m, x, m(x).argmax(1)))
    with pytest.raises(ValueError):
        input_gradient(m, x, torch.zeros(2, dtype=torch.int64))
    # band_importance: shapes and modes
    a, b = band_importance(m, x, 2), band_importance(m, x, 2, mode="abs_grad")
    assert a.shape == b.shape == (3, 6)
    assert torch.allclose(a, m.w[2].detach() * x.sum(dim=(2, 3))) and torch.allclose(b, 25 * m.w[2].detach().abs().expand(3, 6))
    with pytest.raises(ValueError):
        band_importance(m, x, 2, mode="nope")
    # integrated gradients: complete on a linear model, whatever the steps and the chunking
    base = torch.randn(3, 6, 5, 5, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    for steps, mb in ((1, 256), (16, 256), (5, 7)):
        attr, gap = integrated_gradients(m, x, 1, baseline=base, steps=steps, max_batch=mb)
        assert attr.shape == x.shape and gap.shape == (3,) and float(gap.max()) <= 1e-6
        assert torch.allclose(attr, (x - base) * m.w[1].detach().view(1, 6, 1, 1))
    attr, gap = integrated_gradients(m, x, None)
    assert float(gap.max()) <= 1e-6


def declared_arguments(header, name):
    m = re.search(r"^(?:int|long) %s\(([^;]*)\);" % name, header, re.M)
    assert m, name
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return len([a for a in args.split(",") if a.strip()])


def test_c_abi_declares_and_exports_the_input_gradient_calls():
    from maskedsst_amd import _lib
    header = open(_lib.HEADER_PATH).read()
    assert _lib.header_version() == 109   # additive: the revision does not move
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name, n in CALLS.items():
        assert name in _lib.declared_symbols() and re.search(r" T %s$" % name, out, re.M), name
        assert declared_arguments(header, name) == n == len(_lib._SIGS[name][1]) == len(getattr(lib, name).argtypes), name
    names = [lib.msst_profile_name(i).decode() for i in range(lib.msst_profile_kernels())]
    assert "tokenize_bwd_input" in names and "head_bwd_target" in names and "?" not in names


def test_input_gradient_calls_refuse_bad_arguments_before_launch():
    """the checks run before any HIP call: null buffers and no device are enough to see them"""
    from maskedsst_amd import _lib
    lib = _lib.load()
    anchor = ctypes.create_string_buffer(8)
    p = ctypes.c_void_p(ctypes.addressof(anchor))   # a non-null address that nothing dereferences: every call below is refused first

    def tok(B, S, N, P, img=p, dimg=p):
        return lib.msst_tokenize_bwd_input(img, p, p, p, p, p, p, None, p, None, dimg, B, S, N, P, 0.0, 0, None)

    def tgt(B, S, N, P, K, dpred=p):
        return lib.msst_head_bwd_target(dpred, p, p, None, p, B, S, N, P, K, None)

    def scene(Bs, Hs, Ws, win, stride, win0, nwin, S, P, scene_=p):
        return lib.msst_tokenize_scene_bwd_input(scene_, p, p, p, p, p, p, p, p, Bs, Hs, Ws, win, stride, win0, nwin, S, P, 0.0, 0, None)

    for shape in [(0, 5, 64, 10), (2, 0, 64, 10), (2, 5, 0, 10), (2, 5, 64, 0), (-1, 5, 64, 10)]:
        assert tok(*shape) == BADARG and tgt(*shape, 7) == BADARG, shape
    assert tgt(2, 5, 64, 10, 0) == BADARG
    for shape in [(2, 5, 65, 10), (2, 65, 64, 10), (2, 5, 64, 17)]:
        assert tok(*shape) == UNSUPPORTED and tgt(*shape, 7) == UNSUPPORTED, shape
    assert tok(2, 5, 64, 10, img=None) == BADARG and tok(2, 5, 64, 10, dimg=None) == BADARG and tgt(2, 5, 64, 10, 7, dpred=None) == BADARG
    assert b"msst_tokenize_bwd_input" in lib.msst_last_error() or b"msst_head_bwd_target" in lib.msst_last_error()
    assert scene(2, 19, 17, 8, 4, 0, 8, 5, 10) == UNSUPPORTED          # overlapping windows
    assert scene(2, 19, 17, 8, 8, 0, 9, 5, 10) == BADARG               # 2 x 2 x 2 = 8 windows in all
    assert scene(0, 19, 17, 8, 8, 0, 8, 5, 10) == BADARG and scene(2, 19, 17, 8, 8, 0, 8, 5, 10, scene_=None) == BADARG
    assert scene(2, 19, 17, 9, 9, 0, 2, 5, 10) == UNSUPPORTED          # more than 64 pixels per window
