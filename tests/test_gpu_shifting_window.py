"""GPU: shifting_window finetuning -- training on every window of whole tiles.  The tile tokenizer kernels
(msst_tokenize_scene_fwd_train / msst_tokenize_scene_bwd) bit for bit against msst_tokenize_fwd / msst_tokenize_bwd on the stacked copy of
the windows; ViTSpatialSpectral.forward_windows bit for bit against forward(stack_image_batch(...)) for the three heads, both
precisions, full finetune and linear evaluation, with dropout on; against the oracle at the classification path's bars; and
utils.train_step with shifting_window=True on 64 x 64 tiles."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from conftest import oracle_cfg_from, seed_all
from util import pix_head_ref, relerr, spectral_head_ref

pytestmark = pytest.mark.gpu

D = 96
# (name, P, S, window, stride, Bs, Hs, Ws, pos_split): P = 10 and window 8 run the fp32-MFMA kernels, everything else the generic ones
KERNEL_CASES = [
    ("fast_learned", 10, 2, 8, 8, 2, 16, 16, 0),
    ("fast_split", 10, 2, 8, 8, 2, 16, 16, 64),
    ("w7_cutoff2", 10, 2, 7, 7, 2, 16, 16, 0),
    ("w7_cutoff2_split", 10, 2, 7, 7, 2, 16, 16, 48),
    ("w4_9x13", 10, 2, 4, 4, 2, 9, 13, 0),
    ("w4_stride3", 10, 2, 4, 3, 1, 9, 13, 0),
    ("P5", 5, 3, 8, 8, 2, 16, 16, 0),
    ("P16_w4", 16, 2, 4, 4, 2, 9, 13, 32),
]


def _V(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _kernel_inputs(P, S, window, stride, Bs, Hs, Ws, split):
    from maskedsst_amd.scene import scene_windows
    gen = torch.Generator(device="cuda").manual_seed(1000 * P + 10 * window + split)
    r = lambda *shape: torch.randn(*shape, device="cuda", generator=gen)   # noqa: E731
    N = window * window
    w = dict(pre_g=1 + 0.3 * r(P), pre_b=0.2 * r(P), w_emb=0.4 * r(S, D, P), b_emb=0.1 * r(S, D), post_g=1 + 0.3 * r(D), post_b=0.2 * r(D))
    if split:
        w["pos_a"], w["pos_b"] = r(N, split), r(S, D - split)
    else:
        w["pos_a"], w["pos_b"] = r(S * N, D), None
    scene = r(Bs, S * P, Hs, Ws)
    org = scene_windows(Hs, Ws, window, stride)
    stacked = torch.stack([scene[b, :, y:y + window, x:x + window] for b in range(Bs) for y, x in org]).contiguous()
    return w, scene, stacked


def _tok_fwd(lib, w, img, split, p, seed):
    B, C, win, _ = img.shape
    P = w["pre_g"].numel()
    S, N = C // P, win * win
    out = torch.full((B, S * N, D), float("nan"), device="cuda")
    mask = torch.zeros(B * S * N, dtype=torch.uint8, device="cuda")
    rc = lib.msst_tokenize_fwd(_V(img), _V(w["pre_g"]), _V(w["pre_b"]), _V(w["w_emb"]), _V(w["b_emb"]), _V(w["post_g"]), _V(w["post_b"]),
                               _V(w["pos_a"]), _V(w["pos_b"]), split, _V(w["post_b"]), _V(mask), _V(out), B, S, N, P, p, seed, _stream())
    assert rc == 0
    return out


def _tok_scene_fwd(lib, w, scene, window, stride, win0, nwin, split, p, seed):
    Bs, C, Hs, Ws = scene.shape
    P = w["pre_g"].numel()
    S, N = C // P, window * window
    out = torch.full((nwin, S * N, D), float("nan"), device="cuda")
    rc = lib.msst_tokenize_scene_fwd_train(_V(scene), _V(w["pre_g"]), _V(w["pre_b"]), _V(w["w_emb"]), _V(w["b_emb"]), _V(w["post_g"]),
                                           _V(w["post_b"]), _V(w["pos_a"]), _V(w["pos_b"]), split, _V(out), Bs, Hs, Ws, window, stride,
                                           win0, nwin, S, P, p, seed, _stream())
    assert rc == 0
    return out


def _grad_bufs(P, S, N, split):
    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")   # noqa: E731
    g = dict(dpre_g=nan(P), dpre_b=nan(P), dw_emb=nan(S, D, P), db_emb=nan(S, D), dpost_g=nan(D), dpost_b=nan(D))
    g["dpos_a"], g["dpos_b"] = (nan(N, split), nan(S, D - split)) if split else (nan(S * N, D), None)
    return g


def _slab(P, S, N, nchunk):
    return torch.full((S * nchunk * (N * D + D * P + 4 * D + 32) + S * N * D,), float("nan"), device="cuda")


def _tok_bwd(lib, w, img, dx0, nchunk, split, p, seed):
    B, C, win, _ = img.shape
    P = w["pre_g"].numel()
    S, N = C // P, win * win
    g = _grad_bufs(P, S, N, split)
    mask = torch.zeros(B * S * N, dtype=torch.uint8, device="cuda")
    rc = lib.msst_tokenize_bwd(_V(img), _V(w["pre_g"]), _V(w["pre_b"]), _V(w["w_emb"]), _V(w["b_emb"]), _V(w["post_g"]), _V(w["post_b"]),
                               _V(mask), _V(dx0), _V(_slab(P, S, N, nchunk)), nchunk, _V(g["dpre_g"]), _V(g["dpre_b"]), _V(g["dw_emb"]),
                               _V(g["db_emb"]), _V(g["dpost_g"]), _V(g["dpost_b"]), _V(g["dpos_a"]), _V(g["dpos_b"]), split, None,
                               B, S, N, P, p, seed, _stream())
    assert rc == 0
    return g


def _tok_scene_bwd(lib, w, scene, window, stride, win0, nwin, dx0, nchunk, split, p, seed):
    Bs, C, Hs, Ws = scene.shape
    P = w["pre_g"].numel()
    S, N = C // P, window * window
    g = _grad_bufs(P, S, N, split)
    rc = lib.msst_tokenize_scene_bwd(_V(scene), _V(w["pre_g"]), _V(w["pre_b"]), _V(w["w_emb"]), _V(w["b_emb"]), _V(w["post_g"]),
                                     _V(w["post_b"]), _V(dx0), _V(_slab(P, S, N, nchunk)), nchunk, _V(g["dpre_g"]), _V(g["dpre_b"]),
                                     _V(g["dw_emb"]), _V(g["db_emb"]), _V(g["dpost_g"]), _V(g["dpost_b"]), _V(g["dpos_a"]), _V(g["dpos_b"]),
                                     split, Bs, Hs, Ws, window, stride, win0, nwin, S, P, p, seed, _stream())
    assert rc == 0
    return g


def _same(a, b):
    """bitwise equal and free of the NaN prefill"""
    return a is b is None or (torch.equal(a, b) and bool(torch.isfinite(a).all()))


@pytest.mark.parametrize("case", KERNEL_CASES, ids=[c[0] for c in KERNEL_CASES])
def test_tile_tokenizer_forward_is_the_stacked_forward(case):
    from maskedsst_amd import _lib
    lib = _lib.load()
    _, P, S, window, stride, Bs, Hs, Ws, split = case
    w, scene, stacked = _kernel_inputs(P, S, window, stride, Bs, Hs, Ws, split)
    total = stacked.shape[0]
    assert total > 1
    tail = total // 2 + 1   # a call that starts inside the batch and covers its tail only
    for p, seed in ((0.0, 0), (0.1, 12345)):
        want = _tok_fwd(lib, w, stacked, split, p, seed)
        got = _tok_scene_fwd(lib, w, scene, window, stride, 0, total, split, p, seed)
        want_tail = _tok_fwd(lib, w, stacked[tail:].contiguous(), split, p, seed)
        got_tail = _tok_scene_fwd(lib, w, scene, window, stride, tail, total - tail, split, p, seed)
        torch.cuda.synchronize()
        assert _same(got, want), (case[0], p)
        assert _same(got_tail, want_tail), (case[0], p, "tail")
        if p:
            dropped = float((got == 0).float().mean())
            assert 0.05 < dropped < 0.15, dropped   # the dropout is on: a tenth of the elements are zero
        else:
            assert torch.equal(got[tail:], got_tail)   # without dropout a window's tokens do not depend on the call that made them


@pytest.mark.parametrize("case", KERNEL_CASES, ids=[c[0] for c in KERNEL_CASES])
def test_tile_tokenizer_backward_is_the_stacked_backward(case):
    from maskedsst_amd import _lib
    lib = _lib.load()
    _, P, S, window, stride, Bs, Hs, Ws, split = case
    w, scene, stacked = _kernel_inputs(P, S, window, stride, Bs, Hs, Ws, split)
    total = stacked.shape[0]
    tail = total // 2 + 1
    gen = torch.Generator(device="cuda").manual_seed(77)
    dx0 = torch.randn(total, S * window * window, D, device="cuda", generator=gen)
    nchunk = 3   # uneven over the windows
    for p, seed in ((0.0, 0), (0.1, 12345)):
        want = _tok_bwd(lib, w, stacked, dx0, nchunk, split, p, seed)
        got = _tok_scene_bwd(lib, w, scene, window, stride, 0, total, dx0, nchunk, split, p, seed)
        again = _tok_scene_bwd(lib, w, scene, window, stride, 0, total, dx0, nchunk, split, p, seed)
        dtail = dx0[tail:].contiguous()
        want_tail = _tok_bwd(lib, w, stacked[tail:].contiguous(), dtail, 2, split, p, seed)
        got_tail = _tok_scene_bwd(lib, w, scene, window, stride, tail, total - tail, dtail, 2, split, p, seed)
        torch.cuda.synchronize()
        for k in want:
            assert _same(got[k], want[k]), (case[0], p, k)
            assert _same(again[k], got[k]), (case[0], p, k, "second call")
            assert _same(got_tail[k], want_tail[k]), (case[0], p, k, "tail")


# ------------------------------------------------------------------------------------------ model level
HEADS = {"default": dict(), "spectral": dict(spectral_mlp_head=True), "pixelwise": dict(pixelwise=True)}


def _encoder(head, precision="fp32", dropout=0.0, depth=1, heads=2, n_classes=5):
    from maskedsst_amd import ViTSpatialSpectral
    return ViTSpatialSpectral(
        image_size=7 if head == "pixelwise" else 8, spatial_patch_size=1, spectral_patch_size=10, num_classes=n_classes, dim=96,
        depth=depth, heads=heads, mlp_dim=64, dropout=dropout, emb_dropout=dropout, channels=20, spectral_pos_embed=False,
        spectral_pos=torch.arange(2), blockwise_patch_embed=True, precision=precision, **HEADS[head])


def _tiles(head, B=2):
    """16 x 16 tiles of 8 x 8 windows; pixelwise: 15 x 15 tiles of 7 x 7 windows (cutoff 1) -- 4 windows per tile"""
    side = 15 if head == "pixelwise" else 16
    return torch.randn(B, 20, side, side)


def _stack(tiles, head):
    from maskedsst_amd.config import Dotdict
    from maskedsst_amd.utils import stack_image_batch
    cfg = Dotdict(dict(image_size=8, patch_sub=1 if head == "pixelwise" else 0))
    return stack_image_batch(cfg, tiles, tiles[:, 0])[0].contiguous()


@pytest.mark.parametrize("linear_eval", [False, True], ids=["full", "linear_eval"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("head", list(HEADS))
def test_forward_windows_is_forward_of_the_stacked_batch(head, precision, linear_eval):
    seed_all(5)
    enc = _encoder(head, precision, dropout=0.1).cuda()
    if linear_eval:
        for n, q in enc.named_parameters():
            q.requires_grad_("mlp_head" in n)
    tiles = _tiles(head).cuda()
    stacked = _stack(tiles, head)
    assert stacked.shape[0] == 8
    enc.eval()
    with torch.no_grad():
        a, b = enc.forward_windows(tiles), enc(stacked)
    assert a.shape == b.shape == ((8, 5) if head == "pixelwise" else (8, 5, 8, 8)) and torch.equal(a, b)
    assert bool(torch.isfinite(a).all())
    enc.train()
    cot = torch.randn(a.shape, device="cuda")
    runs = []
    for fwd, x in ((enc.forward_windows, tiles), (enc, stacked)):
        enc.zero_grad(set_to_none=True)
        torch.manual_seed(11)
        out = fwd(x)
        (out * cot).sum().backward()
        torch.cuda.synchronize()
        runs.append((out.detach().clone(), {n: q.grad.clone() for n, q in enc.named_parameters() if q.grad is not None}))
    (out_t, g_t), (out_s, g_s) = runs
    assert torch.equal(out_t, out_s) and not torch.equal(out_t, a)   # the same dropout masks, and dropout was on
    want = [n for n, q in enc.named_parameters() if q.requires_grad]
    assert sorted(g_t) == sorted(g_s) == sorted(want) and (not linear_eval or all("mlp_head" in n for n in want))
    bad = [n for n in want if not (torch.equal(g_t[n], g_s[n]) and bool(torch.isfinite(g_t[n]).all()))]
    assert not bad, bad
    assert any(float(g_t[n].abs().max()) > 0 for n in want)


def test_forward_windows_keeps_the_refusals():
    """an encoder wrapped in SimMIM under grad, and gradient accumulation, are refused as in forward"""
    from maskedsst_amd import SimMIMSpatialSpectral
    seed_all(5)
    enc = _encoder("default").cuda()
    tiles = _tiles("default").cuda()
    enc.forward_windows(tiles).sum().backward()
    with pytest.raises(RuntimeError, match="accumulation"):
        enc.forward_windows(tiles).sum().backward()
    enc2 = _encoder("default")
    mim = SimMIMSpatialSpectral(encoder=enc2, masking_ratio=0.7, mask_patch_size=4, tube_masking=True,
                                to_pixels_per_spectral_block=True).cuda()   # kept alive: the encoder holds its wrapper weakly
    assert mim.encoder is enc2
    with pytest.raises(NotImplementedError):
        enc2.forward_windows(tiles)
    with torch.no_grad():
        assert enc2.forward_windows(tiles).shape == (8, 5, 8, 8)


def _oracle_logits(params, img, head, cfg):
    from oracle import classify_forward
    from oracle.model import encoder_embed, pos_table, transformer_forward
    ocfg = oracle_cfg_from(cfg)
    if head == "default":
        return classify_forward(params, img, ocfg)
    _, tok = encoder_embed(params, img, ocfg)
    y = transformer_forward(params, tok + pos_table(params, ocfg), ocfg)
    i = 2 if head == "pixelwise" else 1
    args = (y, params["encoder.mlp_head.0.weight"], params["encoder.mlp_head.0.bias"], params[f"encoder.mlp_head.{i}.weight"],
            params[f"encoder.mlp_head.{i}.bias"], ocfg.S)
    return pix_head_ref(*args, ocfg.Nsq ** 2) if head == "pixelwise" else spectral_head_ref(*args, ocfg.Nsq)


@pytest.mark.parametrize("head", list(HEADS))
def test_forward_windows_fp32_vs_oracle(head):
    """the classification path's bars: logits 1e-4, CE loss 1e-4, every gradient 3e-4 of the tensor's maximum --
    the oracle runs on the stacked windows"""
    seed_all(5)
    cfg = dict(bands=20, depth=1, heads=2, n_classes=5, image_size=7 if head == "pixelwise" else 8)
    enc = _encoder(head)
    tiles = _tiles(head)
    stacked = _stack(tiles, head)
    s = stacked.shape[-1]
    label = torch.randint(-1, 5, (8, s, s))
    if head == "pixelwise":
        label = label[:, s // 2, s // 2]
    params = {"encoder." + k: v.detach().clone().requires_grad_(True) for k, v in enc.state_dict().items()}
    ref_logits = _oracle_logits(params, stacked, head, cfg)
    ref_loss = F.cross_entropy(ref_logits, label, ignore_index=-1)
    ref_loss.backward()
    enc = enc.cuda()
    logits = enc.forward_windows(tiles.cuda())
    loss = F.cross_entropy(logits, label.cuda(), ignore_index=-1)
    loss.backward()
    torch.cuda.synchronize()
    errs = dict(logits=relerr(logits, ref_logits), loss=abs(loss.item() - ref_loss.item()) / abs(ref_loss.item()))
    grads = {k: relerr(q.grad, params["encoder." + k].grad) for k, q in enc.named_parameters()}
    print(head, errs, "worst gradient", max(grads.items(), key=lambda kv: kv[1]))
    assert errs["logits"] < 1e-4 and errs["loss"] < 1e-4, errs
    bad = {k: e for k, e in grads.items() if not e < 3e-4}
    assert not bad, bad


# ------------------------------------------------------------------------------------------ train_step
class _Recording(torch.nn.Module):
    """a FusedCrossEntropy that keeps the statistics of its last call"""
    fused_stats = True

    def __init__(self, inner):
        super().__init__()
        self.inner, self.stats = inner, None

    def unit_gradient(self, device):
        return self.inner.unit_gradient(device)

    def forward(self, logits, labels, return_stats=False):
        loss, self.stats = self.inner(logits, labels, return_stats=True)
        return (loss, self.stats) if return_stats else loss


@pytest.mark.parametrize("pixelwise", [False, True], ids=["default", "pixelwise"])
def test_train_step_trains_on_every_window_of_the_tile(pixelwise):
    """shifting_window=True, image_size 8, one 64 x 64 tile: the step's loss is the CE over all 64 windows (81 centre pixels of 7 x 7
    windows for a pixelwise model) -- on the code before this flag was honoured it is the CE of one random crop"""
    from maskedsst_amd.config import Dotdict
    from maskedsst_amd.ops import FusedCrossEntropy
    from maskedsst_amd.utils import stack_image_batch, train_step
    head = "pixelwise" if pixelwise else "default"
    cfg = Dotdict(dict(image_size=8, patch_sub=1 if pixelwise else 0, pixelwise=pixelwise, ignored_label=-1, shifting_window=True))
    seed_all(5)
    enc = _encoder(head).cuda()
    img, label = torch.randn(1, 20, 64, 64), torch.randint(-1, 5, (1, 64, 64))
    simg, slabel = stack_image_batch(cfg, img, label)
    n = 81 if pixelwise else 64
    assert simg.shape[0] == n
    if pixelwise:
        slabel = slabel[:, 3, 3]
    enc.eval()
    with torch.no_grad():
        ref_logits = enc(simg.contiguous().cuda())
    want = F.cross_entropy(ref_logits, slabel.cuda(), ignore_index=-1)
    valid = int((slabel != -1).sum())
    enc.train()
    opt = torch.optim.Adam(enc.parameters(), lr=1e-3)
    before = {k: q.detach().clone() for k, q in enc.named_parameters()}
    loss, acc, _ = train_step(img, label, enc, cfg, "cuda", torch.nn.CrossEntropyLoss(ignore_index=-1), opt)
    torch.cuda.synchronize()
    print(head, "loss", loss.item(), "CE over all windows", want.item())
    assert abs(loss.item() - want.item()) <= 1e-6 * abs(want.item())   # the same logits: only the mean's summation order may differ
    assert 0.0 <= float(acc) <= 1.0
    moved = [k for k, q in enc.named_parameters() if not torch.equal(q, before[k])]
    assert len(moved) == len(before), set(before) - set(moved)
    # the fused criterion counts the valid labels of the whole tile
    with torch.no_grad():
        for k, q in enc.named_parameters():
            q.copy_(before[k])
    crit = _Recording(FusedCrossEntropy(ignore_index=-1))
    loss_f, _, _ = train_step(img, label, enc, cfg, "cuda", crit, torch.optim.Adam(enc.parameters(), lr=1e-3))
    h = crit.stats.host()
    print(head, "fused loss", loss_f.item(), "n_valid", h.n_valid, "valid labels", valid)
    assert h.n_valid == valid
    assert abs(loss_f.item() - want.item()) <= 1e-5 * abs(want.item())   # one-pass fp32 loss kernel against torch's


def test_train_step_flag_off_is_the_step_without_the_key():
    from maskedsst_amd.config import Dotdict
    from maskedsst_amd.utils import train_step
    img, label = torch.randn(2, 20, 64, 64), torch.randint(-1, 5, (2, 64, 64))
    outs = []
    for extra in (dict(shifting_window=False), dict()):
        cfg = Dotdict(dict(image_size=8, patch_sub=0, pixelwise=False, ignored_label=-1, **extra))
        seed_all(5)
        enc = _encoder("default", dropout=0.1).cuda().train()
        opt = torch.optim.Adam(enc.parameters(), lr=1e-3)
        torch.manual_seed(3)
        loss, acc, _ = train_step(img, label, enc, cfg, "cuda", torch.nn.CrossEntropyLoss(ignore_index=-1), opt)
        torch.cuda.synchronize()
        outs.append((loss.detach().clone(), torch.as_tensor(acc).clone(), [q.detach().clone() for q in enc.parameters()]))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert all(torch.equal(a, b) for a, b in zip(outs[0][2], outs[1][2]))
