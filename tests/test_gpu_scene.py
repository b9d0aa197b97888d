"""Scene inference on the MI355X: ViTSpatialSpectral.predict_scene (windowed tokenizer -> blocks -> head -> scene assembly)
against the CPU oracle window by window, the reference fixtures of tools/make_golden_scene.py and the notebook's per-window
loop over the product model."""
import numpy as np
import pytest
import torch

from conftest import load_golden, oracle_cfg_from, seed_all
from util import record, rel_l2

pytestmark = pytest.mark.gpu

FP32_BAR = 1e-4            # fp32 mode against the oracle (the bar of test_finetune_step_fp32)
FP32_LOOP_BAR = 1e-5       # fp32 mode against the same kernels run window by window
# bf16 mode against model(window) with the same precision decisions: the bf16 block kernels' last bits depend on the batch a row
# runs in (measured on an MI355X: rel-L2 1.6e-6 at 50 bands / depth 2, 2.7e-5 at 200 bands / depth 4); bars ~4x the measurement
BF16_LOOP_BAR = {(50, 2): 6e-6, (200, 4): 1e-4}


def make_encoder(cfg, precision="fp32", draw_scene=None):
    """the encoder of tests/test_gpu_finetune.py::build_encoder (same draw order), then the scenes from the same stream"""
    from maskedsst_amd import ViTSpatialSpectral
    seed_all(5)
    w = cfg.get("image_size", 8)
    enc = ViTSpatialSpectral(
        image_size=w, spatial_patch_size=1, spectral_patch_size=10, num_classes=cfg["n_classes"], dim=96,
        depth=cfg["depth"], heads=cfg.get("heads", 8), mlp_dim=64, dropout=cfg.get("dropout", 0.0),
        emb_dropout=cfg.get("emb_dropout", 0.0), channels=cfg["bands"], spectral_pos_embed=cfg.get("spectral_pos_embed", False),
        spectral_pos=torch.arange(cfg["bands"] // 10), blockwise_patch_embed=True, precision=precision)
    scene = torch.randn(draw_scene) if draw_scene is not None else None
    return enc, scene


def windows_of(scene, w, stride):
    from maskedsst_amd.scene import scene_windows
    Bs, _, Hs, Ws = scene.shape
    org = scene_windows(Hs, Ws, w, stride)
    win = torch.stack([scene[s, :, y:y + w, x:x + w] for s in range(Bs) for (y, x) in org])
    return win, org


def assemble(win_logits, Bs, Hs, Ws, w, org):
    """host restatement of the assembly: float64 mean of the logits of the windows covering a pixel (window order), 0 elsewhere"""
    nc = win_logits.shape[1]
    acc = torch.zeros(Bs, nc, Hs, Ws, dtype=torch.float64)
    cnt = torch.zeros(Bs, 1, Hs, Ws, dtype=torch.float64)
    i = 0
    for s in range(Bs):
        for (y, x) in org:
            acc[s, :, y:y + w, x:x + w] += win_logits[i].double().cpu()
            cnt[s, :, y:y + w, x:x + w] += 1
            i += 1
    covered = cnt[:, 0] > 0
    return acc / cnt.clamp(min=1), covered


def margin(logits):
    top = logits.topk(2, dim=1).values
    return top[:, 0] - top[:, 1]


def check_maps(classes, logits, ref, covered, bar, test, **kv):
    classes, logits = classes.cpu(), logits.cpu()
    assert classes.dtype == torch.int64
    # uncovered pixels: class -1, logits 0
    assert bool((classes[~covered] == -1).all())
    assert float(logits.permute(0, 2, 3, 1)[~covered].abs().sum()) == 0.0
    # the class map is the argmax of the returned logit map, bit for bit
    assert torch.equal(classes[covered], logits.argmax(dim=1)[covered])
    err = rel_l2(logits.permute(0, 2, 3, 1)[covered], ref.permute(0, 2, 3, 1)[covered])
    assert err < bar, (test, err, bar)
    sure = covered & (margin(ref) > 1e-3)
    assert torch.equal(classes[sure], ref.argmax(dim=1)[sure])
    record(test, err=err, **kv)
    return err


CFG = dict(bands=50, depth=2, n_classes=8)


@pytest.mark.parametrize("stride", [8, 3])
def test_predict_scene_fp32_vs_oracle(stride):
    """logit map = mean of oracle.classify_forward over the windows covering each pixel; 40 x 45 scenes leave a border uncovered"""
    from oracle import classify_forward
    enc, scene = make_encoder(CFG, "fp32", (2, 50, 40, 45))
    params = {"encoder." + k: v.detach().clone() for k, v in enc.state_dict().items()}
    win, org = windows_of(scene, 8, stride)
    with torch.no_grad():
        ref_win = classify_forward(params, win, oracle_cfg_from(dict(CFG, B=len(win))))
    ref, covered = assemble(ref_win, 2, 40, 45, 8, org)
    if stride == 8:
        assert not bool(covered.all())
    enc = enc.cuda()
    classes, logits = enc.predict_scene(scene.cuda(), stride=stride, return_logits=True)
    assert classes.shape == (2, 40, 45) and logits.shape == (2, 8, 40, 45)
    check_maps(classes, logits, ref, covered, FP32_BAR, "test_predict_scene_fp32_vs_oracle", stride=stride)


@pytest.mark.parametrize("name", ["scene_50b_L2_Bs2_64x64.npz", "scene_50b_L2_Bs2_40x44.npz"])
def test_predict_scene_vs_reference_fixture(name):
    g = load_golden(name)
    cfg = g["cfg"]
    enc, scene = make_encoder(cfg, "fp32", (cfg["Bs"], cfg["bands"], cfg["Hs"], cfg["Ws"]))
    s = scene.double()
    np.testing.assert_allclose([s.sum().item(), s.abs().sum().item()], g["scene_fp"], rtol=1e-12)
    ref_classes = torch.from_numpy(g["classes"].astype(np.int64))
    ref_logits = torch.from_numpy(g["logits"])
    covered = ref_classes >= 0
    classes, logits = enc.cuda().predict_scene(scene.cuda(), return_logits=True)
    classes, logits = classes.cpu(), logits.cpu()
    assert torch.equal(classes < 0, ~covered)
    sure = covered & (margin(ref_logits) > 1e-3)
    assert torch.equal(classes[sure], ref_classes[sure])
    err = rel_l2(logits.permute(0, 2, 3, 1)[covered], ref_logits.permute(0, 2, 3, 1)[covered])
    assert err < FP32_BAR, err
    assert float(logits.permute(0, 2, 3, 1)[~covered].abs().sum()) == 0.0
    record("test_predict_scene_vs_reference_fixture", err=err, name=name)


def notebook_loop(enc, scene, w):
    """the notebook's loop over the product model: model(window) per window (stride = w), logits placed into the scene"""
    Bs, _, Hs, Ws = scene.shape
    out = torch.zeros(Bs, enc.num_classes, Hs, Ws, device=scene.device)
    with torch.no_grad():
        for x in range(0, Hs, w):
            for y in range(0, Ws, w):
                if x + w > Hs or y + w > Ws:
                    continue
                out[:, :, x:x + w, y:y + w] = enc(scene.narrow(2, x, w).narrow(3, y, w))
    return out


@pytest.mark.parametrize("precision,bands,depth", [("fp32", 50, 2), ("bf16", 50, 2), ("bf16", 200, 4)])
def test_predict_scene_vs_notebook_loop(precision, bands, depth):
    enc, scene = make_encoder(dict(bands=bands, depth=depth, n_classes=11), precision, (2, bands, 32, 36))
    enc = enc.cuda().eval()
    scene = scene.cuda()
    ref = notebook_loop(enc, scene, 8).cpu()
    classes, logits = enc.predict_scene(scene, return_logits=True)
    covered = torch.zeros(2, 32, 36, dtype=torch.bool)
    covered[:, :32, :32] = True
    bar = FP32_LOOP_BAR if precision == "fp32" else BF16_LOOP_BAR[(bands, depth)]
    check_maps(classes, logits, ref, covered, bar, "test_predict_scene_vs_notebook_loop", precision=precision, bands=bands, depth=depth)


def test_predict_scene_deterministic_and_chunk_independent():
    enc, scene = make_encoder(dict(bands=50, depth=2, n_classes=8), "bf16", (3, 50, 30, 29))
    enc, scene = enc.cuda(), scene.cuda()
    c0, l0 = enc.predict_scene(scene, stride=5, return_logits=True)
    c1, l1 = enc.predict_scene(scene, stride=5, return_logits=True)
    assert torch.equal(c0, c1) and torch.equal(l0, l1)   # bitwise, run to run
    worst = 0.0   # measured 2.2e-6 (bf16, see BF16_LOOP_BAR): under the fp32 loop bar
    for mw in (7, 64):
        c, l = enc.predict_scene(scene, stride=5, return_logits=True, max_windows=mw)
        err = rel_l2(l, l0)
        worst = max(worst, err)
        assert err < FP32_LOOP_BAR, (mw, err)
        sure = (c0 >= 0) & (margin(l0) > 1e-4)
        assert torch.equal(c[sure], c0[sure])
        assert torch.equal(c < 0, c0 < 0)
    record("test_predict_scene_deterministic_and_chunk_independent", err=worst)


def test_predict_scene_generic_tokenizer_path():
    """image_size 6 (36 spatial tokens): the generic tokenizer template reads the windows"""
    from oracle import classify_forward
    cfg = dict(bands=30, depth=1, n_classes=5, image_size=6)
    enc, scene = make_encoder(cfg, "fp32", (2, 30, 17, 20))
    params = {"encoder." + k: v.detach().clone() for k, v in enc.state_dict().items()}
    win, org = windows_of(scene, 6, 4)
    with torch.no_grad():
        ref_win = classify_forward(params, win, oracle_cfg_from(dict(cfg, B=len(win))))
    ref, covered = assemble(ref_win, 2, 17, 20, 6, org)
    assert not bool(covered.all())
    classes, logits = enc.cuda().predict_scene(scene.cuda(), stride=4, return_logits=True)
    check_maps(classes, logits, ref, covered, FP32_BAR, "test_predict_scene_generic_tokenizer_path")


def test_predict_scene_uncovered_border():
    enc, scene = make_encoder(dict(bands=50, depth=1, n_classes=6), "bf16", (2, 50, 21, 19))
    classes, logits = enc.cuda().predict_scene(scene.cuda(), return_logits=True)
    classes, logits = classes.cpu(), logits.cpu()
    covered = torch.zeros(2, 21, 19, dtype=torch.bool)
    covered[:, :16, :16] = True
    assert bool((classes[~covered] == -1).all()) and bool((classes[covered] >= 0).all())
    assert bool((logits.permute(0, 2, 3, 1)[~covered] == 0).all())
    assert bool((logits.permute(0, 2, 3, 1)[covered] != 0).any(dim=-1).all())


def test_predict_scene_memory_bound():
    """inside a chunk only two token buffers live: the call's allocation peak stays under four token buffers of one chunk plus
    the outputs and the per-window logits"""
    enc, scene = make_encoder(dict(bands=200, depth=4, n_classes=11), "bf16", (4, 200, 64, 64))
    enc, scene = enc.cuda(), scene.cuda()
    mw = 16
    enc.predict_scene(scene, max_windows=mw)   # warm: weight copies, guards
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    classes, logits = enc.predict_scene(scene, return_logits=True, max_windows=mw)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - base
    token_buf = mw * 20 * 64 * 96 * 4
    outputs = logits.numel() * 4 + classes.numel() * 8 + mw * 11 * 64 * 4
    assert growth <= 4 * token_buf + outputs, (growth, token_buf, outputs)
    record("test_predict_scene_memory_bound", growth=growth, token_buf=token_buf, outputs=outputs)


def test_predict_scene_through_simmim_wrapper():
    from maskedsst_amd import SimMIMSpatialSpectral
    cfg = dict(bands=50, depth=2, n_classes=8)
    enc, scene = make_encoder(cfg, "bf16", (2, 50, 24, 24))
    enc2, _ = make_encoder(cfg, "bf16")
    model = SimMIMSpatialSpectral(encoder=enc2, masking_ratio=0.7, mask_patch_size=4, tube_masking=True,
                                  to_pixels_per_spectral_block=True).cuda()
    scene = scene.cuda()
    c0, l0 = enc.cuda().predict_scene(scene, stride=4, return_logits=True)
    c1, l1 = model.encoder.predict_scene(scene, stride=4, return_logits=True)
    assert model.encoder.engine() is model.engine()
    assert rel_l2(l1, l0) < FP32_LOOP_BAR
    sure = margin(l0) > 1e-4
    assert torch.equal(c1[sure], c0[sure]) and torch.equal(c1 < 0, c0 < 0)


def test_predict_scene_keeps_training_mode_and_runs_eval_forward():
    cfg = dict(bands=50, depth=2, n_classes=8, dropout=0.3, emb_dropout=0.3)
    enc, scene = make_encoder(cfg, "bf16", (2, 50, 16, 16))
    enc, scene = enc.cuda(), scene.cuda()
    enc.eval()
    c_eval, l_eval = enc.predict_scene(scene, return_logits=True)
    enc.train()
    c_train, l_train = enc.predict_scene(scene, return_logits=True)
    assert enc.training
    assert torch.equal(l_train, l_eval) and torch.equal(c_train, c_eval)   # no dropout in the train-mode call
    enc.eval()
    enc.predict_scene(scene)
    assert not enc.training
    assert not l_train.requires_grad


@pytest.mark.parametrize("shape,kw", [
    ((2, 40, 16, 16), {}),          # wrong band count
    ((2, 50, 7, 16), {}),           # smaller than a window
    ((50, 16, 16), {}),             # not 4-D
    ((2, 50, 16, 16), {"stride": 9}),
])
def test_predict_scene_bad_input(shape, kw):
    enc, _ = make_encoder(dict(bands=50, depth=1, n_classes=4), "bf16")
    enc = enc.cuda()
    with pytest.raises(ValueError):
        enc.predict_scene(torch.zeros(shape, device="cuda"), **kw)


def test_finetune_scene_validation():
    """finetune.py --val-scenes N --val-every K prints one 'val step' line per validation; the training lines are those of
    the run without the options (the held-out scenes come from a generator of their own)"""
    import os
    import subprocess
    import sys
    from conftest import ROOT

    def run(extra):
        e = dict(os.environ)
        e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
        r = subprocess.run([sys.executable, "finetune.py", "enmap", "--steps", "10", "--batch-size", "2", "--precision", "fp32"] + extra,
                           cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        return r.stdout.splitlines()

    plain = run([])
    val = run(["--val-scenes", "2", "--val-every", "5"])
    train_lines = lambda lines: [l.split()[:6] for l in lines if l.startswith("step ")]   # noqa: E731  (samples/s varies)
    assert train_lines(plain) and train_lines(val) == train_lines(plain)
    vl = [l.split() for l in val if l.startswith("val step ")]
    assert [v[2] for v in vl] == ["5", "10"], val
    for v in vl:
        loss, acc, macro = float(v[4]), float(v[6]), float(v[8])
        assert np.isfinite(loss) and 0.0 <= acc <= 1.0 and 0.0 <= macro <= 1.0
    assert not any(l.startswith("val step ") for l in plain)
