"""GPU: the linear probe on cached features -- msst_probe_grad / msst_probe_update / msst_probe_fwd (maskedsst_amd/csrc/msst_probe.hip)
against the float64 restatement of tests/probe_util.py: one gradient launch against float64 autograd, whole trajectories against
float64 Adam, equal bits from equal inputs and in place in a model's flat buffer, the minibatch walk and the skipped step, the
forward in both layouts, the route through the model (probe_bank, load_into, probe_predict_scene) and the two scripts.  The bars
are 4 x the errors measured on the MI355X (profiles/probe_parity_measured.jsonl); tests/test_probe_host.py checks on
the CPU that they still tell the mutated references apart.  Every device output is prefilled with NaN or a sentinel."""
import json
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT
from util import record
import probe_util as pu

pytestmark = pytest.mark.gpu


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


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


def make_bank(x, labels, nc):
    from maskedsst_amd import KnnBank
    return KnnBank(x.clone().cuda(), labels.clone().cuda(), nc)


def make_probe(theta0, nc):
    from maskedsst_amd import LinearProbe
    return LinearProbe(theta0.clone().cuda(), nc)


# ------------------------------------------------------------------------------------- 1. one gradient launch against float64 autograd
def grad_figures(M, nc, variant):
    """-> (errors, correct of the launch, the float64 reference)"""
    from maskedsst_amd import probe_gradient
    c = pu.grad_case(M, nc, variant)
    grad, row = probe_gradient(make_bank(c["x"], c["labels"], nc), make_probe(c["theta0"], nc), c["row0"], c["rows"], c["class_w"])
    row = row.cpu()
    assert float(row[3]) == c["rows"]
    return pu.grad_errors(grad, row, c["ref"], nc), int(row[2]), c["ref"]


@pytest.mark.parametrize("variant", pu.GRAD_VARIANTS)
@pytest.mark.parametrize("M,nc", pu.GRAD_SHAPES)
def test_one_gradient_launch_against_float64_autograd(M, nc, variant):
    err, correct, ref = grad_figures(M, nc, variant)
    print(f"probe grad ({M}, {nc}, {variant}): {err}")
    assert correct == ref["correct"]                      # exact: every row's top-two gap exceeds 1e-4 (asserted by the fixture)
    bad = pu.within(err, pu.bars("test_gpu_probe.gradient"))
    assert not bad, bad
    record("test_gpu_probe.gradient", M=M, n_classes=nc, variant=variant, **{f"err_{k}": v for k, v in err.items()})


# ------------------------------------------------------------------------------------------- 2. trajectories against float64 Adam
def fit_case(c, nc, steps, batch, **kw):
    from maskedsst_amd import fit_linear_probe
    return fit_linear_probe(make_bank(c["x"], c["labels"], nc), steps=steps, lr=pu.LR, betas=pu.BETAS, eps=pu.EPS, weight_decay=pu.WD,
                            batch=batch, class_weights=c["class_w"], init=make_probe(c["theta0"], nc), **kw)


def traj_figures(M, nc, batch, weighted, steps, scale=1.0):
    c = pu.traj_case(M, nc, batch, weighted, steps, scale)
    probe = fit_case(c, nc, steps, batch)
    ref = c["ref"]
    h = probe.history.double()
    assert h.shape == (steps, 4) and probe.steps_applied == ref["steps_applied"]
    assert torch.equal(h[:, 3], ref["history"][:, 3]) and pu.relmax(h[:, 1], ref["history"][:, 1]) < 1e-6
    off = (h[:, 2] - ref["history"][:, 2]).abs()
    # `correct` is exact wherever every row's argmax is decided; a step holding undecided rows (probe_util.CLOSE_ALLOWED) may differ by them
    assert bool((off <= torch.tensor(ref["close"], dtype=torch.float64)).all()), (off.tolist(), ref["close"])
    return pu.traj_errors(h, probe.theta, probe.m, probe.v, ref, nc)


@pytest.mark.parametrize("steps", pu.TRAJ_STEPS)
@pytest.mark.parametrize("M,nc,batch,weighted", pu.TRAJ_CONFIGS)
def test_trajectory_against_float64_adam(M, nc, batch, weighted, steps):
    err = traj_figures(M, nc, batch, weighted, steps)
    print(f"probe trajectory ({M}, {nc}, {batch}, {weighted}) x {steps}: {err}")
    bad = pu.within(err, pu.bars(f"test_gpu_probe.trajectory_{steps}"))
    assert not bad, bad
    record("test_gpu_probe.trajectory", M=M, n_classes=nc, batch=batch, weighted=weighted, steps=steps,
           **{f"err_{k}": v for k, v in err.items()})


@pytest.mark.parametrize("steps", pu.TRAJ_STEPS)
def test_trajectory_on_the_small_variance_bank(steps):
    """the fixture of the LayerNorm-eps mutant: rows of variance about 1e-4, where eps 1e-5 is a tenth of the variance"""
    err = traj_figures(300, 5, None, False, steps, 0.01)
    print(f"probe trajectory (small variance) x {steps}: {err}")
    bad = pu.within(err, pu.bars(f"test_gpu_probe.trajectory_small_variance_{steps}"))
    assert not bad, bad
    record("test_gpu_probe.trajectory_small_variance", steps=steps, **{f"err_{k}": v for k, v in err.items()})


# ------------------------------------------------------------------------------------------------------------------------- 3. bits
def probe_bits_equal(a, b):
    return same_bits(a.theta, b.theta) and same_bits(a.m, b.m) and same_bits(a.v, b.v) and same_bits(a.history, b.history) \
        and torch.equal(a.step, b.step)


@pytest.mark.parametrize("M,nc,batch,weighted", [(1000, 17, 128, False), (67, 3, None, True), (2048, 128, None, False)])
def test_two_fits_give_the_same_bits(M, nc, batch, weighted):
    c = pu.traj_case(M, nc, batch, weighted, 8)
    a, b = fit_case(c, nc, 8, batch), fit_case(c, nc, 8, batch)
    assert probe_bits_equal(a, b)
    assert not torch.isnan(a.theta).any() and not same_bits(a.theta, c["theta0"].cuda())


def make_model(nc=5, **kw):
    from maskedsst_amd import ViTSpatialSpectral
    torch.manual_seed(5)
    return ViTSpatialSpectral(image_size=8, spatial_patch_size=1, spectral_patch_size=10, num_classes=nc, dim=96, depth=1, heads=8,
                              mlp_dim=64, channels=50, spectral_pos=torch.arange(5), blockwise_patch_embed=True, precision="fp32",
                              **kw).cuda()


def test_inplace_trains_the_flat_buffer_segment():
    from maskedsst_amd import LinearProbe, fit_linear_probe
    model = make_model(5)
    model.predict_scene(torch.zeros(1, 50, 8, 8, device="cuda"))          # a warm engine: the flat buffer exists
    c = pu.traj_case(300, 5, None, False, 8)
    bank = make_bank(c["x"], c["labels"], 5)
    kw = dict(steps=8, lr=pu.LR, weight_decay=pu.WD)
    copy = fit_linear_probe(bank, init=model, **kw)                            # a fit on a copy of the head
    fp = model.engine().fp
    before = fp.flat.clone()
    off = fp.segments["mlp_head.0.weight"][0]
    n = pu.n_params(5)
    assert same_bits(LinearProbe.from_model(model).theta, before[off:off + n])
    live = fit_linear_probe(bank, inplace=model, **kw)
    assert live.theta.data_ptr() == fp.flat.data_ptr() + 4 * off
    assert probe_bits_equal(live, copy)
    assert same_bits(fp.flat[:off], before[:off]) and same_bits(fp.flat[off + n:], before[off + n:])
    assert not same_bits(fp.flat[off:off + n], before[off:off + n])
    assert same_bits(model.mlp_head[1].weight.detach().reshape(-1), copy.weight.reshape(-1))   # the parameters are still the views


# ---------------------------------------------------------------------------------------------------- 4. minibatch and skipped step
def test_minibatch_walk_against_float64():
    M, nc, steps = 70, 4, 5
    x, labels, theta0 = pu.make_fixture(M, nc, 31)
    walk = pu.slice_walk(M, 32, steps)
    ref = pu.adam64(theta0, x, labels, None, nc, walk, check=True)
    probe = fit_case(dict(x=x, labels=labels, theta0=theta0, class_w=None), nc, steps, 32)
    assert probe.history[:, 3].tolist() == [32.0, 32.0, 6.0, 32.0, 32.0]
    assert torch.equal(probe.history[:, 2].double(), ref["history"][:, 2]) and probe.steps_applied == 5
    err = pu.traj_errors(probe.history, probe.theta, probe.m, probe.v, ref, nc)
    print(f"probe minibatch walk: {err}")
    bad = pu.within(err, pu.bars("test_gpu_probe.trajectory_8"))
    assert not bad, bad


def test_zero_weight_slice_is_skipped_whole():
    """a bank sorted by class, class 0 weighted 0, batch = class 0's size: step 1 sees no weight and changes nothing; step 2 is the
    float64 first Adam step"""
    from maskedsst_amd import fit_linear_probe
    M, nc = 96, 4
    x, labels, theta0 = pu.make_fixture(M, nc, 32)
    order = torch.sort(labels, stable=True).indices
    x, labels = x[order].contiguous(), labels[order].contiguous()
    n0 = int((labels == 0).sum())
    cw = [0.0, 1.0, 2.0, 0.5]
    c = dict(x=x, labels=labels, theta0=theta0, class_w=cw)
    one = fit_case(c, nc, 1, n0)
    assert torch.isnan(one.history[0, 0]) and one.history[0, 1:].tolist() == [0.0, float(one.history[0, 2]), float(n0)]
    assert same_bits(one.theta, theta0.cuda()) and not one.m.any() and not one.v.any() and not one.step.any()
    two = fit_case(c, nc, 2, n0)
    ref = pu.adam64(theta0, x, labels, cw, nc, pu.slice_walk(M, n0, 2))
    assert ref["steps_applied"] == 1 and two.steps_applied == 1 and torch.isnan(two.history[0, 0]) and not torch.isnan(two.history[1, 0])
    assert two.history[1, 3] == n0 and torch.equal(two.history[:, 2].double(), ref["history"][:, 2])
    err = pu.traj_errors(two.history, two.theta, two.m, two.v, ref, nc)
    print(f"probe skipped step: {err}")
    bad = pu.within(err, pu.bars("test_gpu_probe.trajectory_8"))
    assert not bad, bad


# --------------------------------------------------------------------------------------------------------------------- 5. forward
def fwd_run(probe, x, x_layout, Q, plane, out_layout):
    from maskedsst_amd.probe import probe_forward
    nc = probe.n_classes
    logits = torch.full((Q, nc) if out_layout == 0 else (Q // plane, nc, plane), 12345.0, device="cuda")
    classes = torch.full((Q,), -77, dtype=torch.int64, device="cuda")
    probe_forward(probe, x, x_layout, Q, plane, logits, out_layout, classes)
    torch.cuda.synchronize()
    return logits, classes


def forward_figures(nc, Q):
    c = pu.forward_case(nc, Q)      # 2 Q rows, NaN rows among them: a map of two scenes with Q pixels each
    x, theta0, ok, ref = c["x"], c["theta0"], c["ok"], c["ref"]
    probe = make_probe(theta0, nc)
    rows = x.cuda()
    fmap = rows.view(2, Q, 96).permute(0, 2, 1).contiguous()             # [2, 96, Q]
    la, ca = fwd_run(probe, rows, 0, 2 * Q, 1, 0)
    lm, cm = fwd_run(probe, fmap, 1, 2 * Q, Q, 1)
    assert same_bits(lm, la.view(2, Q, nc).permute(0, 2, 1).contiguous()) and torch.equal(ca, cm)
    lr, cr = fwd_run(probe, fmap, 1, 2 * Q, Q, 0)                         # the map read in place, rows written
    assert same_bits(lr, la) and torch.equal(cr, ca)
    la, ca = la.cpu(), ca.cpu()
    assert torch.isnan(la[~ok]).all() and (ca[~ok] == -1).all() and not torch.isnan(la[ok]).any()
    assert torch.equal(ca[ok], ref.argmax(dim=1))
    assert torch.equal(probe.classify(rows).cpu(), ca) and same_bits(probe.logits(rows).cpu(), la)
    return dict(logits=pu.relmax(la[ok], ref))


@pytest.mark.parametrize("Q", [1, 17, 65])
@pytest.mark.parametrize("nc", [2, 17, 128])
def test_forward_layouts_and_nan_rows(nc, Q):
    err = forward_figures(nc, Q)
    print(f"probe forward ({nc}, {Q}): {err}")
    bad = pu.within(err, pu.bars("test_gpu_probe.forward"))
    assert not bad, bad
    record("test_gpu_probe.forward", n_classes=nc, Q=Q, err_logits=err["logits"])


# ----------------------------------------------------------------------------------------------------------- 6. through the model
def model_figures():
    from maskedsst_amd import LinearProbe, fit_linear_probe, probe_bank
    model = make_model(5)
    g = torch.Generator().manual_seed(3)
    scene = torch.randn(2, 50, 16, 16, generator=g).cuda()
    labels = torch.randint(-1, 5, (2, 16, 16), generator=g).cuda()
    bank = probe_bank(model, scene, labels)
    emb = model.encode_scene(scene, normalize=False)
    ok = (emb.cover > 0) & (labels != -1)
    assert 0 < int(ok.sum()) < labels.numel() and len(bank) == int(ok.sum()) and bank.n_classes == 5
    assert same_bits(bank.features, emb.features.permute(0, 2, 3, 1)[ok].contiguous()) and torch.equal(bank.labels.long(), labels[ok])
    probe = fit_linear_probe(bank, steps=20, lr=1e-2)
    assert probe.history.shape == (20, 4) and float(probe.history[-1, 0]) < float(probe.history[0, 0])
    model.predict_scene(scene)                                              # warm the engine, then change the head under it
    probe.load_into(model)
    classes, logits = model.predict_scene(scene, return_logits=True)
    res = model.probe_predict_scene(scene, probe)
    assert res.logits.shape == (2, 5, 16, 16) and res.classes.dtype == torch.int64 and torch.equal(res.cover, emb.cover)
    back = LinearProbe.from_model(model)
    assert same_bits(back.theta, probe.theta) and not back.m.any()
    # float64 head on the cached features: where its top-two gap exceeds GAP both routes must give its class
    ref = pu.forward64(probe.theta.double().cpu(), emb.features.permute(0, 2, 3, 1).reshape(-1, 96).cpu(), 5)
    decided = (ref.topk(2, dim=1).values.diff(dim=1).abs().reshape(-1) > pu.GAP)
    share = float(decided.double().mean())
    assert share >= 0.99, share
    want = ref.argmax(dim=1)[decided]
    assert torch.equal(res.classes.reshape(-1).cpu()[decided], want) and torch.equal(classes.reshape(-1).cpu()[decided], want)
    return dict(logits=pu.relmax(res.logits, logits.double()), logits_vs_float64=pu.relmax(res.logits.permute(0, 2, 3, 1).reshape(-1, 5), ref))


def test_through_the_model():
    err = model_figures()
    print(f"probe through the model: {err}")
    bad = pu.within(err, pu.bars("test_gpu_probe.model"))
    assert not bad, bad
    record("test_gpu_probe.model", err_logits=err["logits"], err_logits_vs_float64=err["logits_vs_float64"])


def test_load_into_refuses_other_heads():
    from maskedsst_amd import LinearProbe, ViTSpatialSpectral
    probe = make_probe(pu.make_fixture(4, 5, 1)[2], 5)
    torch.manual_seed(5)
    kw = dict(spatial_patch_size=1, spectral_patch_size=10, num_classes=5, dim=96, depth=1, heads=8, mlp_dim=64, channels=50,
              spectral_pos=torch.arange(5), blockwise_patch_embed=True)
    for model in (ViTSpatialSpectral(image_size=8, spectral_mlp_head=True, **kw).cuda(), ViTSpatialSpectral(image_size=7, pixelwise=True, **kw).cuda(),
                  make_model(6)):
        with pytest.raises(ValueError):
            probe.load_into(model)
    for model in (ViTSpatialSpectral(image_size=8, spectral_mlp_head=True, **kw).cuda(), ViTSpatialSpectral(image_size=7, pixelwise=True, **kw).cuda()):
        with pytest.raises(ValueError):
            LinearProbe.from_model(model)


# ------------------------------------------------------------------------------------------------------------------------ 7. scripts
def test_finetune_val_probe_script():
    """finetune.py --val-probe: one more line per validation pass, beside --val-embed's, on the same split"""
    out = child([sys.executable, "finetune.py", "--steps", "2", "--val-scenes", "4", "--val-every", "1", "--val-embed", "--val-probe", "20"], 600)
    lines = out.splitlines()
    pr = [l.split() for l in lines if l.startswith("val-probe step ")]
    emb = [l.split() for l in lines if l.startswith("val-embed step ")]
    assert [e[2] for e in pr] == ["1", "2"] and [e[2] for e in emb] == ["1", "2"], out
    for e, m in zip(pr, emb):
        assert e[3:5] == ["steps", "20"] and e[5] == "probe_acc" and 0.0 <= float(e[6]) <= 1.0, e
        assert e[7] == "bank_pixels" and int(e[8]) > 0 and e[9] == "test_pixels" and int(e[10]) > 0, e
        assert (e[8], e[10]) == (m[8], m[10])          # the split of --val-embed


def test_probe_time_script():
    """tools/probe_time.py --smoke: exit 0 and ONE JSON line, nothing appended"""
    out = child([sys.executable, os.path.join("tools", "probe_time.py"), "--smoke"], 300)
    lines = [l for l in out.splitlines() if l.strip()]
    assert len(lines) == 1, out
    row = json.loads(lines[0])
    assert row["tool"] == "probe_time" and len(row["results"]) >= 1
    r = row["results"][0]
    assert r["fit_ms"] > 0 and r["eager_fit_ms"] > 0 and r["linear_eval_step_ms"] > 0 and r["linear_eval_steps_per_fit"] > 0
