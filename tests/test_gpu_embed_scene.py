"""GPU: whole-scene embedding maps -- msst_pool_spectral_fwd against float64, msst_scene_embed_assemble against a float64 host fold
(bit equality where windows do not overlap, the rounding of k - 1 fp32 additions and one division where they do, the cover map, NaN
where nothing covers a pixel, any split into calls, the L2 normalisation), ViTSpatialSpectral.encode_scene against the CPU oracle
window by window and against predict_scene through the model's own head, its independence of repetition, mode, chunking and the
SimMIM wrapper, tools/embed_time.py and finetune.py --val-embed."""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT, load_golden, oracle_cfg_from, seed_all
from util import host_fold, record, rel_l2, relerr

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # unit roundoff of fp32
FP32_BAR = 1e-4         # every forward stage, fp32 mode, of the tensor maximum
BF16_BAR = 5e-3         # bf16 stages at depth <= 2, max-norm
CHUNK_BAR = 2e-6        # what predict_scene's chunk test records where a window's place in its chunk reaches the encoder's last bits


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a) if a.dtype == torch.float32 else a, bits(b) if b.dtype == torch.float32 else b)


def lib_and_helpers():
    from maskedsst_amd import _lib
    from maskedsst_amd.engine import _p, _stream
    return _lib.load(), _p, _stream


# ------------------------------------------------------------------------------------------------------------------ 1. pool kernel
@pytest.mark.parametrize("B,S,N", [(1, 1, 1), (2, 5, 64), (3, 20, 64), (2, 3, 36), (1, 64, 16), (5, 7, 49)])
def test_pool_spectral_against_float64(B, S, N):
    lib, _p, _stream = lib_and_helpers()
    g = torch.Generator().manual_seed(B * 10000 + S * 100 + N)
    y = torch.randn(B, S * N, 96, generator=g)
    y64 = y.double().view(B, S, N, 96)
    ref = (y64.sum(dim=1) / S).permute(0, 2, 1)                                    # [B, 96, N]
    bound = ((S + 1) * U * y64.abs().sum(dim=1) / S).permute(0, 2, 1)
    yd = y.cuda()
    outs = []
    for _ in range(2):
        out = torch.full((B, 96, N), float("nan"), device="cuda")
        assert lib.msst_pool_spectral_fwd(_p(yd), _p(out), B, S, N, _stream()) == 0
        outs.append(out)
    torch.cuda.synchronize()
    got = outs[0].cpu()
    assert not torch.isnan(got).any()
    err = (got.double() - ref).abs()
    print(f"pool ({B}, {S}, {N}): worst error / bound = {float((err / bound.clamp(min=1e-300)).max()):.3f}")
    assert (err <= bound).all(), float((err - bound).max())
    assert same_bits(outs[0], outs[1])


# -------------------------------------------------------------------------------------------------------------------- 2. assembler
def run_assemble(win_d, Bs, D, Hs, Ws, w, stride, splits, l2norm=0):
    """msst_scene_embed_assemble over the windows in calls of the given sizes -> (feat, cover), both prefilled (NaN, 12345) to show
    that nothing needs initialising"""
    lib, _p, _stream = lib_and_helpers()
    feat = torch.full((Bs, D, Hs, Ws), float("nan"), device="cuda")
    cover = torch.full((Bs, Hs, Ws), 12345, dtype=torch.int32, device="cuda")
    total = win_d.shape[0]
    win0 = 0
    for n in splits:
        part = win_d[win0:win0 + n].contiguous()
        rc = lib.msst_scene_embed_assemble(_p(part), win0, n, _p(feat), _p(cover), Bs, D, Hs, Ws, w, stride, int(win0 + n == total), l2norm,
                                           _stream())
        assert rc == 0, (rc, lib.msst_last_error())
        win0 += n
    assert win0 == total
    torch.cuda.synchronize()
    return feat, cover


def chunks_of(total, n):
    return [min(n, total - i) for i in range(0, total, n)]


@pytest.mark.parametrize("D", [96, 5])
@pytest.mark.parametrize("w,stride", [(8, 8), (8, 4), (8, 3), (8, 1), (7, 7), (7, 2), (6, 5)])
@pytest.mark.parametrize("Bs,Hs,Ws", [(2, 20, 22), (1, 8, 8)])
def test_scene_embed_assemble_against_the_host_fold(Bs, Hs, Ws, w, stride, D):
    nr, nq = (Hs - w) // stride + 1, (Ws - w) // stride + 1
    total = Bs * nr * nq
    g = torch.Generator().manual_seed(Hs * 1000 + w * 100 + stride * 10 + D)
    win = torch.randn(total, D, w * w, generator=g)
    acc, mag, cover_ref = host_fold(win, Bs, Hs, Ws, w, stride)
    win_d = win.cuda()
    feat_d, cover_d = run_assemble(win_d, Bs, D, Hs, Ws, w, stride, [total])
    feat, cover = feat_d.cpu(), cover_d.cpu()
    assert cover.dtype == torch.int32 and torch.equal(cover, cover_ref)                      # exact against the host count
    covered = (cover_ref > 0)[:, None].expand(Bs, D, Hs, Ws)
    assert torch.isnan(feat[~covered]).all() and not torch.isnan(feat[covered]).any()        # absent, in every channel; never elsewhere
    k = cover_ref.double().clamp(min=1)[:, None]
    mean = acc / k
    if stride == w:
        # one window per covered pixel: its value, bit for bit (0 + v, v / 1)
        assert torch.equal(bits(feat[covered]), bits(mean.float()[covered]))
    err = (feat.double() - mean).abs()[covered]
    bound = ((k + 1) * U * mag / k)[covered]
    print(f"assemble {Bs}x{Hs}x{Ws} w {w} stride {stride} D {D}: worst error / bound = {float((err / bound.clamp(min=1e-300)).max()):.3f}")
    assert (err <= bound).all(), float((err - bound).max())
    # any split into calls: the same bits
    for splits in (chunks_of(total, 1), chunks_of(total, 7), [total - 1, 1] if total > 1 else [1]):
        f2, c2 = run_assemble(win_d, Bs, D, Hs, Ws, w, stride, splits)
        assert same_bits(f2, feat_d) and torch.equal(c2, cover_d), (splits[:3], len(splits))
    # l2norm: against float64 on the un-normalised output
    fn_d, cn = run_assemble(win_d, Bs, D, Hs, Ws, w, stride, chunks_of(total, 7), l2norm=1)
    fn = fn_d.cpu()
    assert torch.equal(cn.cpu(), cover_ref) and torch.isnan(fn[~covered]).all() and not torch.isnan(fn[covered]).any()
    f64 = feat.double()
    norm = torch.where(covered[:, :1], f64, torch.zeros((), dtype=torch.float64)).pow(2).sum(dim=1, keepdim=True).sqrt()
    want = f64 / norm.clamp(min=1e-12)
    nerr = (fn.double() - want).abs()[covered]
    nbound = (64 * U * f64.abs() / norm.clamp(min=1e-300))[covered]
    print(f"  l2norm: worst error / bound = {float((nerr / nbound.clamp(min=1e-300)).max()):.3f}")
    assert (nerr <= nbound).all(), float((nerr - nbound).max())
    fn2, _ = run_assemble(win_d, Bs, D, Hs, Ws, w, stride, [total], l2norm=1)
    assert same_bits(fn2, fn_d)


def test_scene_embed_assemble_l2norm_keeps_a_zero_pixel_zero():
    Bs, D, Hs, Ws, w, stride = 1, 96, 10, 9, 8, 1
    total = 3 * 2
    g = torch.Generator().manual_seed(3)
    win = torch.randn(total, D, w, w, generator=g)
    # pixel (4, 4) lies at (4 - r, 4 - q) of window (r, q): every window's feature there is zero
    for r in range(3):
        for q in range(2):
            win[r * 2 + q, :, 4 - r, 4 - q] = 0.0
    feat, cover = run_assemble(win.view(total, D, w * w).cuda(), Bs, D, Hs, Ws, w, stride, [total], l2norm=1)
    feat = feat.cpu()
    assert int(cover[0, 4, 4]) == 6
    assert (feat[0, :, 4, 4] == 0).all()
    others = torch.ones(Hs, Ws, dtype=torch.bool)
    others[4, 4] = False
    others &= cover[0].cpu() > 0
    n = feat[0].double().pow(2).sum(dim=0).sqrt()[others]
    assert ((n - 1).abs() < 64 * U).all()


# --------------------------------------------------------------------------------------------------- 3. end to end against the oracle
def make_encoder(cfg, precision="fp32", draw_scene=None):
    """the encoder of tests/test_gpu_scene.py::make_encoder (same draw order), plus pixelwise"""
    from maskedsst_amd import ViTSpatialSpectral
    seed_all(5)
    enc = ViTSpatialSpectral(
        image_size=cfg.get("image_size", 8), spatial_patch_size=1, spectral_patch_size=10, num_classes=cfg["n_classes"], dim=96,
        depth=cfg["depth"], heads=cfg.get("heads", 8), mlp_dim=64, dropout=cfg.get("dropout", 0.0),
        emb_dropout=cfg.get("emb_dropout", 0.0), channels=cfg["bands"], spectral_pos_embed=cfg.get("spectral_pos_embed", False),
        spectral_pos=torch.arange(cfg["bands"] // 10), blockwise_patch_embed=True, pixelwise=cfg.get("pixelwise", False),
        precision=precision)
    scene = torch.randn(draw_scene) if draw_scene is not None else None
    return enc, scene


def frozen(cfg):
    return tuple(sorted(cfg.items()))


@functools.lru_cache(maxsize=None)
def oracle_map(cfg_items, shape, stride):
    """(reference features [Bs, 96, Hs, Ws] float64, cover [Bs, Hs, Ws] int32) of the seeded model and scene of cfg: per window
    oracle.transformer_forward(encoder_embed + pos_table), the mean over S, then the float64 mean over the covering windows.
    Computed once per (model, scene, stride), shared by the precisions, read-only."""
    from oracle import encoder_embed, transformer_forward
    from oracle.model import pos_table
    from maskedsst_amd.scene import scene_windows
    cfg = dict(cfg_items)
    enc, scene = make_encoder(cfg, "fp32", shape)
    params = {"encoder." + k: v.detach().clone() for k, v in enc.state_dict().items()}
    w = cfg.get("image_size", 8)
    Bs, _, Hs, Ws = shape
    org = scene_windows(Hs, Ws, w, stride)
    win = torch.stack([scene[s, :, y:y + w, x:x + w] for s in range(Bs) for (y, x) in org])
    ocfg = oracle_cfg_from(dict(cfg, B=len(win)))
    with torch.no_grad():
        _, tok = encoder_embed(params, win, ocfg)
        y = transformer_forward(params, tok + pos_table(params, ocfg), ocfg)
    S = cfg["bands"] // 10
    f = y.double().view(len(win), S, w * w, 96).mean(dim=1).permute(0, 2, 1)    # [nwin, 96, N]
    acc, _, cover = host_fold(f, Bs, Hs, Ws, w, stride)
    return acc / cover.double().clamp(min=1)[:, None], cover


def check_against_oracle(cfg, shape, stride, precision, bar, test):
    ref, cover_ref = oracle_map(frozen(cfg), shape, stride)
    enc, scene = make_encoder(cfg, precision, shape)
    emb = enc.cuda().encode_scene(scene.cuda(), stride=stride)
    assert type(emb).__name__ == "SceneEmbedding" and emb._fields == ("features", "cover")
    feat, cover = emb.features.cpu(), emb.cover.cpu()
    Bs, _, Hs, Ws = shape
    assert feat.shape == (Bs, 96, Hs, Ws) and feat.dtype == torch.float32 and not emb.features.requires_grad
    assert cover.dtype == torch.int32 and torch.equal(cover, cover_ref)
    covered = (cover_ref > 0)[:, None].expand_as(feat)
    assert torch.isnan(feat[~covered]).all() and not torch.isnan(feat[covered]).any()
    err = relerr(feat[covered], ref[covered])
    print(f"{test} {precision} stride {stride}: max-norm error {err:.3e} (bar {bar:.0e})")
    assert err < bar, (test, precision, stride, err, bar)
    record(test, err=err, precision=precision, stride=stride)


def golden_cfg():
    cfg = load_golden("scene_50b_L2_Bs2_40x44.npz")["cfg"]
    shape = (cfg["Bs"], cfg["bands"], cfg["Hs"], cfg["Ws"])
    return dict(bands=cfg["bands"], depth=cfg["depth"], n_classes=cfg["n_classes"]), shape


@pytest.mark.parametrize("stride", [8, 4, 3])
@pytest.mark.parametrize("precision,bar", [("fp32", FP32_BAR), ("bf16", BF16_BAR)])
def test_encode_scene_vs_oracle(precision, bar, stride):
    cfg, shape = golden_cfg()
    assert shape == (2, 50, 40, 44) and cfg["depth"] == 2
    check_against_oracle(cfg, shape, stride, precision, bar, "test_encode_scene_vs_oracle")


PIX_CFG = dict(bands=30, depth=1, n_classes=5, image_size=7, pixelwise=True)
SIX_CFG = dict(bands=30, depth=1, n_classes=5, image_size=6, heads=2)


@pytest.mark.parametrize("cfg,shape,stride", [(PIX_CFG, (1, 30, 16, 17), None), (PIX_CFG, (1, 30, 16, 17), 3), (SIX_CFG, (2, 30, 17, 20), 4)])
def test_encode_scene_other_models_vs_oracle(cfg, shape, stride):
    """a 7 x 7 pixelwise model (its head is never run; stride None still means image_size) and a 6 x 6, S = 3, 2-head model
    (generic tokenizer, 4-wave block kernel), fp32"""
    w = cfg["image_size"]
    ref_stride = w if stride is None else stride
    ref, cover_ref = oracle_map(frozen(cfg), shape, ref_stride)
    enc, scene = make_encoder(cfg, "fp32", shape)
    emb = enc.cuda().encode_scene(scene.cuda(), stride=stride)
    feat, cover = emb.features.cpu(), emb.cover.cpu()
    assert torch.equal(cover, cover_ref) and not bool((cover_ref > 0).all())
    covered = (cover_ref > 0)[:, None].expand_as(feat)
    assert torch.isnan(feat[~covered]).all() and not torch.isnan(feat[covered]).any()
    err = relerr(feat[covered], ref[covered])
    print(f"other models w {w} stride {stride}: max-norm error {err:.3e}")
    assert err < FP32_BAR, err
    record("test_encode_scene_other_models_vs_oracle", err=err, image_size=w, stride=ref_stride)


# ---------------------------------------------------------------------------------------------- 4. consistency with predict_scene
def test_encode_scene_feeds_the_models_own_head():
    """default head, stride = image_size: LayerNorm + Linear of mlp_head in float64 on the feature map = predict_scene's logit map"""
    cfg = dict(bands=50, depth=2, n_classes=8)
    enc, scene = make_encoder(cfg, "fp32", (2, 50, 21, 19))
    enc, scene = enc.cuda(), scene.cuda()
    emb = enc.encode_scene(scene)
    classes, logits = enc.predict_scene(scene, return_logits=True)
    cover = emb.cover.cpu()
    assert torch.equal(classes.cpu() == -1, cover == 0) and not bool((cover > 0).all())
    ln, lin = enc.mlp_head[0], enc.mlp_head[1]
    f = emb.features.cpu().double().permute(0, 2, 3, 1)[cover > 0]                     # [pixels, 96]
    x = torch.nn.functional.layer_norm(f, (96,), ln.weight.detach().cpu().double(), ln.bias.detach().cpu().double(), ln.eps)
    want = x @ lin.weight.detach().cpu().double().t() + lin.bias.detach().cpu().double()
    got = logits.cpu().double().permute(0, 2, 3, 1)[cover > 0]
    err = float((got - want).abs().max() / want.abs().max())
    print(f"head on features vs predict_scene: {err:.3e} of the logit maximum")
    assert err < 1e-4, err


# ------------------------------------------------------------------------------------------------------------------ 5. properties
def test_encode_scene_repetition_and_mode_leave_every_bit():
    cfg = dict(bands=50, depth=2, n_classes=8, dropout=0.3, emb_dropout=0.3)
    enc, scene = make_encoder(cfg, "bf16", (2, 50, 19, 21))
    enc, scene = enc.cuda(), scene.cuda()
    enc.eval()
    a = enc.encode_scene(scene, stride=3, normalize=True)
    b = enc.encode_scene(scene, stride=3, normalize=True)
    assert not enc.training
    assert same_bits(a.features, b.features) and torch.equal(a.cover, b.cover)
    enc.train()
    c = enc.encode_scene(scene, stride=3, normalize=True)
    assert enc.training                                                   # the mode is left as it was
    assert same_bits(a.features, c.features) and torch.equal(a.cover, c.cover)   # no dropout in the train-mode call
    assert not c.features.requires_grad
    # normalize: unit vectors on covered pixels, the direction of the plain map
    plain = enc.encode_scene(scene, stride=3)
    ok = plain.cover > 0
    f = plain.features.double().permute(0, 2, 3, 1)[ok]
    want = torch.nn.functional.normalize(f, dim=1)
    got = c.features.double().permute(0, 2, 3, 1)[ok]
    assert float((got - want).abs().max()) < 64 * U
    assert torch.isnan(c.features.permute(0, 2, 3, 1)[~ok]).all()


def test_encode_scene_chunking_leaves_every_bit_for_8x8_windows():
    """S = 4: 16 spectral sequences fill a 64-row tile and 64 of them a window, so a window's place in its chunk reaches no sum"""
    cfg = dict(bands=40, depth=2, n_classes=8)
    enc, scene = make_encoder(cfg, "bf16", (3, 40, 30, 29))
    enc, scene = enc.cuda(), scene.cuda()
    a = enc.encode_scene(scene, stride=5)
    for mw in (1, 7, 64):
        b = enc.encode_scene(scene, stride=5, max_windows=mw)
        assert same_bits(a.features, b.features) and torch.equal(a.cover, b.cover), mw


def test_encode_scene_chunking_6x6_within_the_recorded_bound():
    """6 x 6, S = 3: 21 spectral sequences per tile do not split window by window, so the encoder's last bits depend on the chunk"""
    enc, scene = make_encoder(SIX_CFG, "fp32", (2, 30, 17, 20))
    enc, scene = enc.cuda(), scene.cuda()
    a = enc.encode_scene(scene, stride=4)
    ok = (a.cover > 0)[:, None].expand_as(a.features)
    worst = 0.0
    for mw in (1, 7):
        b = enc.encode_scene(scene, stride=4, max_windows=mw)
        assert torch.equal(a.cover, b.cover) and torch.equal(torch.isnan(a.features), torch.isnan(b.features))
        worst = max(worst, rel_l2(b.features[ok], a.features[ok]))
    print(f"6 x 6 chunking: rel-L2 {worst:.3e}")
    assert worst < CHUNK_BAR, worst


def test_encode_scene_through_simmim_wrapper_gives_the_bare_encoders_bits():
    from maskedsst_amd import SimMIMSpatialSpectral
    cfg = dict(bands=40, depth=2, n_classes=8)
    enc, scene = make_encoder(cfg, "bf16", (2, 40, 24, 24))
    enc2, _ = make_encoder(cfg, "bf16")
    model = SimMIMSpatialSpectral(encoder=enc2, masking_ratio=0.7, mask_patch_size=4, tube_masking=True,
                                  to_pixels_per_spectral_block=True).cuda()
    for (n1, p1), (n2, p2) in zip(enc.named_parameters(), model.encoder.named_parameters()):
        assert n1 == n2 and torch.equal(p1.detach().cpu(), p2.detach().cpu())
    scene = scene.cuda()
    a = enc.cuda().encode_scene(scene, stride=4)
    b = model.encoder.encode_scene(scene, stride=4)
    assert model.encoder.engine() is model.engine()
    assert same_bits(a.features, b.features) and torch.equal(a.cover, b.cover)


def test_encode_scene_bad_input_on_the_device():
    enc, _ = make_encoder(dict(bands=50, depth=1, n_classes=4), "bf16")
    enc = enc.cuda()
    for shape, kw in (((2, 40, 16, 16), {}), ((2, 50, 7, 16), {}), ((50, 16, 16), {}), ((2, 50, 16, 16), {"stride": 9}),
                      ((2, 50, 16, 16), {"stride": 0})):
        with pytest.raises(ValueError):
            enc.encode_scene(torch.zeros(shape, device="cuda"), **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc.encode_scene(torch.zeros(2, 50, 16, 16))


# ------------------------------------------------------------------------------------------------------------------------ 6. tools
def child(cmd, timeout):
    """a script in a fresh child process under its own time limit.  A child that timed out or died of a signal (a GPU fault, an abort)
    ends the session: nothing more is started on the device after it."""
    e = dict(os.environ)
    e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
    try:
        r = subprocess.run(cmd, cwd=ROOT, env=e, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as t:
        pytest.exit(f"{' '.join(cmd)} timed out after {timeout} s: no further GPU work\n{(t.stderr or '')[-2000:]}", returncode=1)
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        pytest.exit(f"{' '.join(cmd)} ended with {r.returncode}: no further GPU work\n{r.stderr[-3000:]}", returncode=1)
    assert r.returncode == 0, f"--- stdout\n{r.stdout[-3000:]}\n--- stderr\n{r.stderr[-3000:]}"
    return r.stdout


def test_embed_time_script(tmp_path):
    """tools/embed_time.py --quick: exit 0, ONE JSON line with both legs' times at both strides, the same line appended to --append"""
    log = str(tmp_path / "t.jsonl")
    out = child([sys.executable, os.path.join("tools", "embed_time.py"), "--quick", "--append", log], 300)
    lines = [l for l in out.splitlines() if l.strip()]
    assert len(lines) == 1, out
    row = json.loads(lines[0])
    assert [json.loads(l) for l in open(log)] == [row]
    assert row["tool"] == "encode_scene_time" and row["scenes"] == 2 and row["scene_size"] == 24 and row["bands"] == 50
    assert [r["stride"] for r in row["results"]] == [8, 4] and [r["windows"] for r in row["results"]] == [2 * 9, 2 * 25]
    for r in row["results"]:
        assert len(r["encode_scene_ms"]) == len(r["eager_ms"]) == 2
        assert all(v > 0 for v in r["encode_scene_ms"] + r["eager_ms"]) and r["pool_kernel_ms"] > 0 and r["assemble_kernels_ms"] > 0
        assert r["cover_equal"] and r["nan_equal"] and r["max_abs_diff"] < 1e-4, r


def test_finetune_val_embed_script():
    """finetune.py --val-embed: one more line per validation pass, after the 'val step' line"""
    out = child([sys.executable, "finetune.py", "--steps", "2", "--val-scenes", "2", "--val-every", "1", "--val-embed"], 600)
    lines = out.splitlines()
    emb = [l.split() for l in lines if l.startswith("val-embed step ")]
    assert [e[2] for e in emb] == ["1", "2"], out
    assert len([l for l in lines if l.startswith("val step ")]) == 2
    for e in emb:
        assert e[3] == "ncm_acc" and 0.0 <= float(e[4]) <= 1.0
        assert e[9] == "test_pixels" and int(e[10]) > 0 and int(e[8]) > 0 and e[11:] == ["scenes", "2"]
