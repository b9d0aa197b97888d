"""The linear probe, host side (no GPU needed): the C ABI of msst_probe_scratch_floats / msst_probe_grad / msst_probe_update /
msst_probe_fwd (additive under MSST_VERSION 109) and their argument checks (they run before any HIP call, so null pointers, host
buffers and no device are enough to see them), the ValueError / RuntimeError surface of maskedsst_amd/probe.py, the minibatch
bookkeeping, the flag of finetune.py, and the float64 restatement of tests/probe_util.py: its Adam against torch.optim.Adam, the
conditioning of every fixture it hands out, and the committed bars against the mutated references."""
import ctypes
import re
import subprocess

import pytest
import torch

import probe_util as pu

BADARG, UNSUPPORTED = -3, -2   # include/msst.h: MSST_ERR_BADARG, MSST_ERR_UNSUPPORTED


# --------------------------------------------------------------------------------------------------------------------- C ABI
def test_c_abi_declares_and_exports_the_entry_points():
    from ctypes import c_double, c_int, c_long, c_void_p
    from maskedsst_amd import _lib
    header = open(_lib.HEADER_PATH).read()
    assert _lib.header_version() == 109   # additive: the revision does not move
    lib = _lib.load()
    assert lib.msst_version() == 109
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    P = c_void_p
    sigs = {
        # long rows, int nc
        "msst_probe_scratch_floats": (c_long, [c_long, c_int]),
        # x, labels, class_w, theta, long M, int dim, long row0, long rows, int nc, slab, long slab_floats, stream
        "msst_probe_grad": (c_int, [P, P, P, P, c_long, c_int, c_long, c_long, c_int, P, c_long, P]),
        # slab, long slab_floats, long rows, int dim, int nc, theta, m, v, step, double lr, beta1, beta2, eps, weight_decay, history_row,
        # grad_out, int apply, stream
        "msst_probe_update": (c_int, [P, c_long, c_long, c_int, c_int, P, P, P, P] + [c_double] * 5 + [P, P, c_int, P]),
        # x, int x_layout, long Q, long plane, theta, int dim, int nc, logits, int out_layout, classes, stream
        "msst_probe_fwd": (c_int, [P, c_int, c_long, c_long, P, c_int, c_int, P, c_int, P, P]),
    }
    for name, sig in sigs.items():
        assert re.search(r"^(int|long) %s\(" % name, header, re.M), name
        assert name in _lib.declared_symbols() and _lib._SIGS[name] == sig, name
        assert re.search(r" T %s$" % name, out, re.M), name
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == sig, name
    assert re.search(r"^#define\s+MSST_PROBE_STEP_INTS\s+%d$" % _lib.PROBE_STEP_INTS, header, re.M)
    import maskedsst_amd
    for name in ("LinearProbe", "ProbeScene", "fit_linear_probe", "probe_bank", "probe_gradient", "probe_predict_scene"):
        assert name in maskedsst_amd.__all__ and hasattr(maskedsst_amd, name), name
    assert maskedsst_amd.ProbeScene._fields == ("classes", "logits", "cover")
    assert hasattr(maskedsst_amd.ViTSpatialSpectral, "probe_predict_scene")
    assert "differs" in maskedsst_amd.ViTSpatialSpectral.probe_predict_scene.__doc__      # overlapping windows: features, not logits, are averaged
    assert "msst_probe.hip" in __import__("maskedsst_amd.build", fromlist=["SOURCES"]).SOURCES


def _ptr():
    buf = (ctypes.c_char * 64)()
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)


def test_scratch_floats():
    from maskedsst_amd import _lib
    f = _lib.load().msst_probe_scratch_floats
    per = lambda nc: 192 + 97 * nc + 4   # noqa: E731
    assert f(1, 2) == per(2) and f(64, 16) == per(16) and f(65, 16) == 2 * per(16) and f(512 * 64, 5) == 512 * per(5)
    assert f(512 * 64 + 1, 5) == 257 * per(5)                   # two tiles per workgroup from here on
    assert f(262144, 16) == 512 * per(16) and f(262144, 128) == 512 * per(128)
    for bad in ((0, 5), (-1, 5), (10, 0), (10, 129)):
        assert f(*bad) == 0, bad


def test_probe_grad_refuses_bad_arguments_before_launch():
    from maskedsst_amd import _lib
    lib = _lib.load()
    buf, p = _ptr()
    names = ("x", "labels", "class_w", "theta", "slab")

    def call(M=100, dim=96, row0=0, rows=100, nc=5, slab_floats=None, **ptr):
        a = {n: ptr.get(n, p) for n in names}
        if slab_floats is None:
            slab_floats = lib.msst_probe_scratch_floats(rows, nc)
        return lib.msst_probe_grad(a["x"], a["labels"], a["class_w"], a["theta"], M, dim, row0, rows, nc, a["slab"], slab_floats, None)

    null = {n: None for n in names}
    for bad in (dict(rows=0), dict(rows=-3), dict(row0=-1), dict(row0=1), dict(row0=50, rows=51), dict(row0=101, rows=1), dict(nc=0),
                dict(nc=-2), dict(M=0, rows=1), dict(dim=0)):
        assert call(**bad) == BADARG and call(**bad, **null) == BADARG, bad
    assert b"msst_probe_grad" in lib.msst_last_error()
    for over in (dict(dim=95), dict(dim=97), dict(dim=128), dict(nc=129), dict(nc=1000)):
        assert call(slab_floats=1 << 40, **over) == UNSUPPORTED and call(slab_floats=0, **over, **null) == UNSUPPORTED, over
    assert b"msst_probe_grad" in lib.msst_last_error()
    # the limits themselves are inside: the next check (null pointers) answers
    assert call(nc=128, **null) == BADARG and call(nc=1, row0=99, rows=1, **null) == BADARG and b"null" in lib.msst_last_error()
    for n in ("x", "labels", "theta", "slab"):
        assert call(**{n: None}) == BADARG, n
    assert call(x=ctypes.c_void_p(p.value + 4)) == BADARG
    for n in ("labels", "class_w", "theta", "slab"):
        assert call(**{n: ctypes.c_void_p(p.value + 2)}) == BADARG, n
    need = lib.msst_probe_scratch_floats(100, 5)
    assert need > 0 and call(slab_floats=need - 1) == BADARG and call(slab_floats=0) == BADARG
    assert b"slab" in lib.msst_last_error()


def test_probe_update_refuses_bad_arguments_before_launch():
    from maskedsst_amd import _lib
    lib = _lib.load()
    buf, p = _ptr()
    names = ("slab", "theta", "m", "v", "step", "history_row", "grad_out")

    def call(rows=100, dim=96, nc=5, lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0, apply=1, slab_floats=None, **ptr):
        a = {n: ptr.get(n, p) for n in names}
        if slab_floats is None:
            slab_floats = lib.msst_probe_scratch_floats(rows, nc)
        return lib.msst_probe_update(a["slab"], slab_floats, rows, dim, nc, a["theta"], a["m"], a["v"], a["step"], lr, beta1, beta2, eps, wd,
                                     a["history_row"], a["grad_out"], apply, None)

    null = {n: None for n in names}
    for bad in (dict(rows=0), dict(rows=-1), dict(nc=0), dict(dim=0)):
        assert call(**bad) == BADARG and call(**bad, **null) == BADARG, bad
    for over in (dict(dim=95), dict(nc=129)):
        assert call(slab_floats=1 << 40, **over) == UNSUPPORTED and call(**over, **null) == UNSUPPORTED, over
    assert b"msst_probe_update" in lib.msst_last_error()
    for bad in (dict(lr=-1e-3), dict(lr=float("nan")), dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.5), dict(eps=-1e-8), dict(wd=-1e-4),
                dict(wd=float("nan"))):
        assert call(**bad) == BADARG, bad
    for n in ("slab", "theta", "m", "v", "step", "history_row"):
        assert call(**{n: None}) == BADARG, n
    for n in names:
        assert call(**{n: ctypes.c_void_p(p.value + 2)}) == BADARG, n
    assert call(slab_floats=lib.msst_probe_scratch_floats(100, 5) - 1) == BADARG and b"slab" in lib.msst_last_error()
    # apply = 0 only reduces: theta, m, v, step may be null -- the next refusal is then the slab's size
    assert call(apply=0, theta=None, m=None, v=None, step=None, slab_floats=0) == BADARG and b"slab" in lib.msst_last_error()
    assert call(apply=0, slab=None, theta=None, m=None, v=None, step=None) == BADARG and b"null" in lib.msst_last_error()


def test_probe_fwd_refuses_bad_arguments_before_launch():
    from maskedsst_amd import _lib
    lib = _lib.load()
    buf, p = _ptr()
    names = ("x", "theta", "logits", "classes")

    def call(x_layout=0, Q=64, plane=1, dim=96, nc=5, out_layout=0, **ptr):
        a = {n: ptr.get(n, p) for n in names}
        return lib.msst_probe_fwd(a["x"], x_layout, Q, plane, a["theta"], dim, nc, a["logits"], out_layout, a["classes"], None)

    null = {n: None for n in names}
    for bad in (dict(Q=0), dict(Q=-1), dict(nc=0), dict(dim=0)):
        assert call(**bad) == BADARG and call(**bad, **null) == BADARG, bad
    for over in (dict(dim=95), dict(dim=192), dict(nc=129), dict(Q=1 << 31)):
        assert call(**over) == UNSUPPORTED and call(x_layout=5, **over, **null) == UNSUPPORTED, over
    assert b"msst_probe_fwd" in lib.msst_last_error()
    for layout in (-1, 2):
        assert call(x_layout=layout) == BADARG and call(out_layout=layout) == BADARG, layout
    for plane in (0, -4, 5, 128):          # layout 1: plane must divide Q = 64
        assert call(x_layout=1, plane=plane) == BADARG and call(out_layout=1, plane=plane) == BADARG, plane
    assert call(plane=5, **null) == BADARG and b"null" in lib.msst_last_error()      # plane is not read in layout 0
    for n in names:
        assert call(**{n: None}) == BADARG, n
    assert call(x=ctypes.c_void_p(p.value + 4)) == BADARG                            # rows are read 16 bytes at a time
    assert call(classes=ctypes.c_void_p(p.value + 4)) == BADARG
    for n in ("theta", "logits"):
        assert call(**{n: ctypes.c_void_p(p.value + 2)}) == BADARG, n
    assert call(nc=128, Q=(1 << 31) - 1, **null) == BADARG                           # the limits themselves are inside


# --------------------------------------------------------------------------------------------------------- the Python surface
def make_encoder(**kw):
    from maskedsst_amd import ViTSpatialSpectral
    torch.manual_seed(5)
    args = dict(image_size=8, spatial_patch_size=1, spectral_patch_size=10, num_classes=4, dim=96, depth=1, heads=8, mlp_dim=64,
                channels=50, spectral_pos=torch.arange(5), blockwise_patch_embed=True)
    args.update(kw)
    return ViTSpatialSpectral(**args)


def fake_bank(M=10, nc=4):
    from maskedsst_amd import KnnBank
    bank = KnnBank.__new__(KnnBank)   # a bank whose tensors are never touched: every refusal below comes before device work
    bank.features, bank.labels, bank.n_classes = torch.zeros(M, 96), torch.zeros(M, dtype=torch.int32), nc
    return bank


def test_slice_walk():
    from maskedsst_amd.probe import slice_walk
    assert slice_walk(10, 4, 7) == [(0, 4), (4, 4), (8, 2), (0, 4), (4, 4), (8, 2), (0, 4)]     # remainder, then the wrap
    assert slice_walk(8, 8, 3) == [(0, 8), (0, 8), (0, 8)]
    assert slice_walk(8, None, 2) == [(0, 8), (0, 8)] and slice_walk(8, 100, 2) == [(0, 8), (0, 8)]
    assert slice_walk(8, 4, 5) == [(0, 4), (4, 4), (0, 4), (4, 4), (0, 4)]                      # no remainder: wrap at the end
    assert slice_walk(70, 32, 5) == [(0, 32), (32, 32), (64, 6), (0, 32), (32, 32)]
    assert slice_walk(3, 1, 4) == [(0, 1), (1, 1), (2, 1), (0, 1)]


def test_fit_refuses_bad_arguments_before_device_work():
    from maskedsst_amd import LinearProbe, fit_linear_probe, probe_gradient
    bank = fake_bank()
    good = LinearProbe(torch.zeros(pu.n_params(4)), 4)
    for kw in (dict(bank=None), dict(bank=object()), dict(steps=0), dict(steps=-1), dict(steps=2.0), dict(steps=True),
               dict(lr=-1e-2), dict(lr=float("nan")), dict(lr=float("inf")), dict(lr="1e-2"), dict(lr=None), dict(lr=[1e-2] * 2),
               dict(lr=[1e-2, -1.0, 1e-2]), dict(lr=[1e-2, None, 1e-2]), dict(betas=(0.9,)), dict(betas=(0.9, 1.0)), dict(betas=(-0.1, 0.9)),
               dict(betas=0.9), dict(eps=-1e-8), dict(eps=None), dict(weight_decay=-1e-4), dict(weight_decay=float("nan")),
               dict(batch=0), dict(batch=-4), dict(batch=2.0), dict(batch=True),
               dict(class_weights=[1.0] * 3), dict(class_weights=[1.0, -1.0, 1.0, 1.0]), dict(class_weights=[0.0] * 4),
               dict(class_weights=[1.0, float("nan"), 1.0, 1.0]), dict(class_weights=[1.0, float("inf"), 1.0, 1.0]),
               dict(class_weights=torch.ones(2, 2)), dict(class_weights="balanced"),
               dict(init=LinearProbe(torch.zeros(pu.n_params(5)), 5)), dict(init=make_encoder(num_classes=5)),
               dict(init=make_encoder(spectral_mlp_head=True)), dict(init=make_encoder(image_size=7, pixelwise=True)), dict(init="zeros"),
               dict(inplace=make_encoder(num_classes=5)), dict(inplace=make_encoder(spectral_mlp_head=True)), dict(inplace=good)):
        args = dict(bank=bank, steps=3)
        args.update(kw)
        with pytest.raises(ValueError):
            fit_linear_probe(**args)
    for args in (dict(), dict(lr=[1e-2, 5e-3, 1e-3]), dict(class_weights=[0.0, 1.0, 2.0, 0.5]), dict(init=good), dict(init=make_encoder()),
                 dict(inplace=make_encoder()), dict(batch=4)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):          # everything is in order but the device
            fit_linear_probe(bank, steps=3, **args)
    for kw in (dict(bank=None), dict(probe=None), dict(probe=LinearProbe(torch.zeros(pu.n_params(5)), 5)), dict(row0=-1), dict(row0=10),
               dict(rows=0), dict(row0=5, rows=6), dict(rows=2.0), dict(class_weights=[1.0] * 5)):
        args = dict(bank=bank, probe=good)
        args.update(kw)
        with pytest.raises(ValueError):
            probe_gradient(**args)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        probe_gradient(bank, good)


def test_linear_probe_and_scene_refuse_bad_arguments():
    from maskedsst_amd import LinearProbe, probe_bank, probe_predict_scene
    n = pu.n_params(4)
    for theta, nc in ((torch.zeros(n - 1), 4), (torch.zeros(n).double(), 4), (torch.zeros(1, n), 4), ([0.0] * n, 4), (torch.zeros(n), 0),
                      (torch.zeros(n), 129), (torch.zeros(n), 4.0), (torch.zeros(2 * n)[::2], 4)):
        with pytest.raises(ValueError):
            LinearProbe(theta, nc)
    with pytest.raises(ValueError):
        LinearProbe(torch.zeros(n), 4, m=torch.zeros(n - 1))
    probe = LinearProbe(torch.zeros(n), 4)
    assert probe.gamma.shape == (96,) and probe.beta.shape == (96,) and probe.weight.shape == (4, 96) and probe.bias.shape == (4,)
    assert probe.step.shape == (512,) and probe.step.dtype == torch.int32 and probe.steps_applied == 0 and probe.history is None
    for f in (torch.zeros(5, 95), torch.zeros(96), torch.zeros(0, 96), torch.zeros(5, 96).double(), torch.zeros(96, 5).t(), [[0.0] * 96]):
        with pytest.raises(ValueError):
            probe.logits(f)
        with pytest.raises(ValueError):
            probe.classify(f)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        probe.logits(torch.zeros(5, 96))
    enc = make_encoder()
    scene = torch.zeros(2, 50, 16, 16)
    for kw in (dict(probe=None), dict(probe=fake_bank()), dict(scene=torch.zeros(2, 40, 16, 16)), dict(scene=torch.zeros(50, 16, 16)),
               dict(scene=torch.zeros(2, 50, 4, 16)), dict(stride=9), dict(stride=0), dict(max_windows=0)):
        args = dict(scene=scene, probe=probe)
        args.update(kw)
        with pytest.raises(ValueError):
            enc.probe_predict_scene(**args)
        with pytest.raises(ValueError):
            probe_predict_scene(enc, **args)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc.probe_predict_scene(scene, probe)
    labels = torch.zeros(2, 16, 16, dtype=torch.int64)
    for kw in (dict(scenes=torch.zeros(50, 16, 16)), dict(labels=torch.zeros(2, 16, 15, dtype=torch.int64)), dict(labels=torch.zeros(2, 16, 16)),
               dict(per_class=0), dict(per_class=2.0)):
        args = dict(scenes=scene, labels=labels)
        args.update(kw)
        with pytest.raises(ValueError):
            probe_bank(enc, **args)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        probe_bank(enc, scene, labels)
    assert enc.training   # nothing above touched the module's mode


def test_load_into_and_from_model_take_the_patch_head_only():
    from maskedsst_amd import LinearProbe
    g = torch.Generator().manual_seed(1)
    probe = LinearProbe(torch.randn(pu.n_params(4), generator=g), 4)
    for model in (make_encoder(num_classes=5), make_encoder(num_classes=3), make_encoder(spectral_mlp_head=True),
                  make_encoder(image_size=7, pixelwise=True), torch.nn.Linear(96, 4), None):
        with pytest.raises(ValueError):
            probe.load_into(model)
    for model in (make_encoder(spectral_mlp_head=True), make_encoder(image_size=7, pixelwise=True), torch.nn.Linear(96, 4)):
        with pytest.raises(ValueError):
            LinearProbe.from_model(model)
    # the copy itself is plain tensor work: on a CPU model it is in place (the parameters stay the objects they were) and round-trips
    enc = make_encoder()
    params = [enc.mlp_head[0].weight, enc.mlp_head[0].bias, enc.mlp_head[1].weight, enc.mlp_head[1].bias]
    ptrs = [q.data_ptr() for q in params]
    assert probe.load_into(enc) is enc
    assert [q.data_ptr() for q in params] == ptrs and all(q.requires_grad for q in params)
    assert torch.equal(enc.mlp_head[1].weight.detach(), probe.weight) and torch.equal(enc.mlp_head[0].bias.detach(), probe.beta)
    back = LinearProbe.from_model(enc)
    assert torch.equal(back.theta, probe.theta) and back.n_classes == 4 and not back.m.any() and not back.v.any()
    assert back.theta.data_ptr() != enc.mlp_head[0].weight.data_ptr()       # a copy


def test_finetune_parser_takes_val_probe():
    import finetune
    ap = finetune.build_parser()
    assert ap.parse_args(["enmap"]).val_probe == 0
    a = ap.parse_args(["enmap", "--val-scenes", "4", "--val-every", "1", "--val-embed", "--val-probe", "20"])
    assert a.val_probe == 20 and a.val_embed is True
    with pytest.raises(SystemExit):
        finetune.check_val_probe(ap.parse_args(["enmap", "--val-probe", "20"]))                     # needs --val-scenes and --val-every
    with pytest.raises(SystemExit):
        finetune.check_val_probe(ap.parse_args(["enmap", "--val-scenes", "4", "--val-probe", "20"]))
    with pytest.raises(SystemExit):
        finetune.check_val_probe(ap.parse_args(["enmap", "--val-scenes", "4", "--val-every", "1", "--val-probe", "-3"]))
    finetune.check_val_probe(a)
    finetune.check_val_probe(ap.parse_args(["enmap"]))


# ------------------------------------------------------------------------------------------------- the float64 restatement itself
def test_restatement_is_torch_adam_in_float64():
    """adam64 (Adam written out, so that it can be mutated) against torch.optim.Adam and torch's weighted CrossEntropyLoss"""
    M, nc, steps = 67, 3, 6
    x, labels, theta0 = pu.make_fixture(M, nc, 77)
    cw = pu.traj_weights(nc)
    walk = pu.slice_walk(M, 32, steps)
    ref = pu.adam64(theta0, x, labels, cw, nc, walk)
    theta = theta0.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([theta], lr=pu.LR, betas=pu.BETAS, eps=pu.EPS, weight_decay=pu.WD)
    crit = torch.nn.CrossEntropyLoss(weight=torch.tensor(cw, dtype=torch.float64))
    for i, (row0, rows) in enumerate(walk):
        opt.zero_grad()
        loss = crit(pu.forward64(theta, x[row0:row0 + rows], nc), labels[row0:row0 + rows])
        assert abs(loss.item() - float(ref["history"][i, 0])) <= 1e-13 * abs(loss.item())
        loss.backward()
        opt.step()
    assert pu.relmax(theta.detach(), ref["theta"]) < 1e-13
    st = opt.state[theta]
    assert pu.relmax(st["exp_avg"], ref["m"]) < 1e-13 and pu.relmax(st["exp_avg_sq"], ref["v"]) < 1e-13
    assert ref["history"][:, 3].tolist() == [32.0, 32.0, 3.0, 32.0, 32.0, 3.0] and ref["steps_applied"] == steps


def test_restatement_skips_a_step_without_weight():
    x, labels, theta0 = pu.make_fixture(12, 3, 78)
    order = torch.sort(labels, stable=True).indices
    x, labels = x[order], labels[order]
    ref = pu.adam64(theta0, x, labels, [0.0, 1.0, 1.0], 3, [(0, 4), (4, 4)])
    one = pu.adam64(theta0, x, labels, [0.0, 1.0, 1.0], 3, [(4, 4)])
    assert torch.isnan(ref["history"][0, 0]) and ref["steps_applied"] == 1 and torch.equal(ref["theta"], one["theta"])


def test_every_fixture_is_well_conditioned():
    """building a fixture runs its asserts: top-two logit gaps above 1e-4, gradient components above 1e-7 of the largest"""
    for M, nc in pu.GRAD_SHAPES:
        for variant in pu.GRAD_VARIANTS:
            c = pu.grad_case(M, nc, variant)
            assert c["ref"]["gap"] > pu.GAP and c["row0"] + c["rows"] <= M
    c = pu.grad_case(300, 5, "weights")
    assert c["class_w"][0] == 0.0 and not bool((c["labels"] == 4).any())            # one zero weight, one class absent
    c = pu.grad_case(300, 5, "slice")
    assert c["row0"] != 0 and (c["row0"] + c["rows"]) % 16 != 0 and c["rows"] % 16 != 0
    c = pu.grad_case(300, 5, "constant_row")
    assert float(c["x"][150].var()) == 0.0
    for nc in (2, 17, 128):
        for Q in (1, 17, 65):
            pu.forward_case(nc, Q)
    for steps in pu.TRAJ_STEPS:
        for cfg in pu.TRAJ_CONFIGS:
            ref = pu.traj_case(*cfg, steps)["ref"]
            assert sum(ref["close"]) <= pu.CLOSE_ALLOWED.get(cfg[:2], 0) and ref["min_grad_ratio"] > pu.MIN_GRAD_RATIO
        c = pu.ln_eps_case(steps)
        assert 5e-5 < float(c["x"].double().var(dim=1, unbiased=False).mean()) < 5e-4      # row variance about 1e-4


def test_committed_bars_tell_the_mutants_apart():
    """every bar is 4 x a committed measurement, and at least one compared quantity of every mutated reference lies beyond its bar"""
    def distance(c, nc, mutant):
        r = pu.adam64(c["theta0"], c["x"], c["labels"], c["class_w"], nc, c["walk"], mutant=mutant)
        return pu.traj_errors(r["history"], r["theta"], r["m"], r["v"], c["ref"], nc)

    for test in ("test_gpu_probe.gradient", "test_gpu_probe.forward", "test_gpu_probe.model"):
        assert all(0.0 <= v < 1e-5 for v in pu.bars(test).values()), test            # fp32 kernels: nothing here is looser than 1e-5
    for steps in pu.TRAJ_STEPS:
        bar = pu.bars(f"test_gpu_probe.trajectory_{steps}")
        assert set(bar) == {"loss"} | {f"{w}.{s}" for w in ("theta", "m", "v") for s in pu.SEGMENTS} and all(0 < v < 1e-4 for v in bar.values())
        for cfg in pu.TRAJ_CONFIGS:                                                  # every run has weight decay 1e-4
            c = pu.traj_case(*cfg, steps)
            for mutant in ["no_weight_decay", "eps_x10", "no_bias_correction"] + (["mean_over_rows"] if cfg[3] else []):
                d = distance(c, cfg[1], mutant)
                assert any(d[k] > bar[k] for k in d), (steps, cfg, mutant, d)
        assert any(cfg[3] for cfg in pu.TRAJ_CONFIGS)
        c = pu.ln_eps_case(steps)
        bar = pu.bars(f"test_gpu_probe.trajectory_small_variance_{steps}")
        d = distance(c, 5, "ln_eps_1e-6")
        assert any(d[k] > bar[k] for k in d), (steps, d)
