"""Cross entropy with class weights, label smoothing and a confusion matrix, host side (no GPU needed): the C ABI of msst_ce_ext_fwd /
msst_ce_ext_bwd / msst_ce_ext_scratch_bytes (additive under MSST_VERSION 109), their argument checks (they run before any HIP call, so
null buffers and no device are enough to see them), ``confusion_report`` against a float64 numpy restatement written here, and the
Python surface: the weight buffer of FusedCrossEntropy, no CPU fallback, finetune.py's new flags."""
import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch

BADARG, UNSUPPORTED = -3, -2   # include/msst.h: MSST_ERR_BADARG, MSST_ERR_UNSUPPORTED
CALLS = {"msst_ce_ext_scratch_bytes": 4, "msst_ce_ext_fwd": 16, "msst_ce_ext_bwd": 8}   # arguments in include/msst.h


def declared_arguments(header, name):
    """the number of arguments of `name`'s declaration in the header (comments removed)"""
    m = re.search(r"^(?:int|long) %s\(([^;]*)\);" % name, header, re.M)
    assert m, name
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return len([a for a in args.split(",") if a.strip()])


def test_c_abi_declares_and_exports_the_extended_calls():
    from maskedsst_amd import _lib
    header = open(_lib.HEADER_PATH).read()
    assert _lib.header_version() == 109   # additive: the revision does not move
    lib = _lib.load()
    assert lib.msst_version() == 109 and set(CALLS) <= set(_lib.declared_symbols())
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name, n in CALLS.items():
        assert re.search(r" T %s$" % name, out, re.M), name
        assert declared_arguments(header, name) == n == len(_lib._SIGS[name][1]) == len(getattr(lib, name).argtypes), name
    # label_smoothing travels as a C float, the sums as a pointer
    assert _lib._SIGS["msst_ce_ext_fwd"][1][5] is ctypes.c_float and _lib._SIGS["msst_ce_ext_fwd"][1][3] is ctypes.c_long
    for name, want in (("EXT_LOSS_SUM", _lib.CE_EXT_LOSS_SUM), ("EXT_WEIGHT_SUM", _lib.CE_EXT_WEIGHT_SUM),
                       ("CONFUSION_MAX_CLASSES", _lib.CE_CONFUSION_MAX_CLASSES)):
        m = re.search(r"#define\s+MSST_CE_%s\s+(\d+)" % name, header)
        assert m and int(m.group(1)) == want, name
    assert _lib.CE_CONFUSION_MAX_CLASSES >= 128
    # the record keeps its layout
    assert re.search(r"#define\s+MSST_CE_RECORD_SLOTS\(n_classes\)\s+\(5 \+ 2 \* \(n_classes\)\)", header)


def test_extended_calls_refuse_bad_arguments_before_launch():
    from maskedsst_amd import _lib
    lib = _lib.load()
    limit = _lib.CE_CONFUSION_MAX_CLASSES
    anchor = ctypes.create_string_buffer(8)   # a non-null address that nothing dereferences: every call below is refused first
    some = ctypes.c_void_p(ctypes.addressof(anchor))

    def fwd(R0, nc, M, eps=0.0, confusion=None, rest=None):
        return lib.msst_ce_ext_fwd(rest, rest, None, -1, None, eps, None, rest, rest, rest, confusion, rest, R0, nc, M, None)

    def bwd(R0, nc, M):
        return lib.msst_ce_ext_bwd(None, None, None, None, R0, nc, M, None)

    for shape in [(0, 8, 64), (4, 0, 64), (4, 8, 0), (-1, 8, 64), (4, -3, 1), (0, 0, 0)]:
        assert fwd(*shape) == BADARG and bwd(*shape) == BADARG, shape
        assert lib.msst_ce_ext_scratch_bytes(*shape, 0) == 0 and lib.msst_ce_ext_scratch_bytes(*shape, 1) == 0, shape
    assert b"msst_ce_ext_bwd" in lib.msst_last_error()
    for shape in [(1 << 16, 8, 1 << 15), (1 << 20, 4096, 1), (3, 1 << 30, 1), (1 << 30, 1, 2)]:
        assert fwd(*shape) == UNSUPPORTED and bwd(*shape) == UNSUPPORTED, shape
        assert lib.msst_ce_ext_scratch_bytes(*shape, 0) == 0, shape
    # shapes the kernels take, with null pointers: bad arguments, nothing launched
    for shape in [(256, 8, 64), (1, 1, 1), (2, 33, 5), (1, 128, 3), (1, 5000, 1)]:
        assert fwd(*shape) == BADARG and bwd(*shape) == BADARG, shape
        assert fwd(*shape, eps=0.1) == BADARG, shape
    assert b"msst_ce_ext_fwd" in lib.msst_last_error()
    # label smoothing outside [0, 1): a bad argument even with every required pointer given
    for eps in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
        assert fwd(2, 8, 64, eps=eps, rest=some) == BADARG, eps
        assert b"label_smoothing" in lib.msst_last_error(), eps
    # a confusion matrix past the class limit: unsupported, whatever else is given; at the limit the null pointers are what is wrong
    assert fwd(1, limit + 1, 2, confusion=some, rest=some) == UNSUPPORTED
    assert b"MSST_CE_CONFUSION_MAX_CLASSES" in lib.msst_last_error()
    assert fwd(1, limit + 1, 2, confusion=some) == UNSUPPORTED and fwd(1, 5000, 1, confusion=some) == UNSUPPORTED
    assert fwd(1, limit, 3, confusion=some) == BADARG and fwd(1, limit + 1, 2) == BADARG
    assert fwd(0, limit + 1, 2, confusion=some) == BADARG               # a size below 1 wins
    assert fwd(1, limit + 1, 2, eps=2.0, confusion=some) == BADARG      # ... and so does the smoothing, in the header's order
    # scratch: two fp32 partials and an int32 row [4 + 2 nc] per 256 rows; with a confusion matrix an int32 [nc][nc] more
    assert lib.msst_ce_ext_scratch_bytes(256, 8, 64, 0) == 64 * (6 + 16) * 4
    assert lib.msst_ce_ext_scratch_bytes(256, 8, 64, 1) == 64 * (6 + 16 + 64) * 4
    assert lib.msst_ce_ext_scratch_bytes(1, 1, 1, 1) == (6 + 2 + 1) * 4
    assert lib.msst_ce_ext_scratch_bytes(3, 97, 100, 1) == 2 * (6 + 194 + 97 * 97) * 4
    assert lib.msst_ce_ext_scratch_bytes(1, limit, 3, 1) == (6 + 2 * limit + limit * limit) * 4
    assert lib.msst_ce_ext_scratch_bytes(1, limit + 1, 2, 1) == 0 and lib.msst_ce_ext_scratch_bytes(1, limit + 1, 2, 0) > 0
    # the existing call keeps its size
    assert lib.msst_ce_scratch_bytes(256, 8, 64) == 64 * (5 + 16) * 4


# ------------------------------------------------------------------------------------------------ confusion_report
def report_reference(cm):
    """float64 numpy restatement of the protocol: overall / average accuracy, precision, recall, F1, IoU by class (0 where the
    denominator is 0), their means over the classes with support, Cohen's kappa (nan when 1 - pe is 0)"""
    cm = np.asarray(cm, dtype=np.float64)
    nc = cm.shape[0]
    n = cm.sum()
    prec, rec, f1, iou = (np.zeros(nc) for _ in range(4))
    for c in range(nc):
        tp, row, col = cm[c, c], cm[c, :].sum(), cm[:, c].sum()
        rec[c] = tp / row if row else 0.0
        prec[c] = tp / col if col else 0.0
        f1[c] = 2.0 * tp / (row + col) if row + col else 0.0
        iou[c] = tp / (row + col - tp) if row + col - tp else 0.0
    has = [c for c in range(nc) if cm[c, :].sum() > 0]
    nan = float("nan")
    oa = np.trace(cm) / n if n else nan
    pe = (cm.sum(axis=0) * cm.sum(axis=1)).sum() / (n * n) if n else nan
    kappa = (oa - pe) / (1.0 - pe) if n and 1.0 - pe != 0.0 else nan
    return dict(oa=oa, aa=np.mean(rec[has]) if has else nan, kappa=kappa, mean_f1=np.mean(f1[has]) if has else nan,
                mean_iou=np.mean(iou[has]) if has else nan, precision=prec, recall=rec, f1=f1, iou=iou)


MATRICES = {
    "mixed": [[5, 1, 0], [2, 3, 1], [0, 0, 7]],
    "class_without_support": [[4, 1, 2], [0, 0, 0], [1, 3, 6]],          # label 1 never occurs, but is predicted
    "class_never_predicted": [[4, 0, 2], [3, 0, 1], [1, 0, 6]],          # class 1 occurs, no pixel is given to it
    "perfect": [[3, 0, 0, 0], [0, 9, 0, 0], [0, 0, 1, 0], [0, 0, 0, 4]],
    "pe_is_one": [[0, 0], [0, 11]],                                       # everything in one cell: 1 - pe = 0
    "one_class": [[6]],
    "empty": [[0, 0], [0, 0]],
    "all_wrong": [[0, 5], [5, 0]],
}


def same(a, b):
    return (a != a and b != b) or abs(a - b) <= 1e-15


@pytest.mark.parametrize("name", sorted(MATRICES))
def test_confusion_report_matches_the_numpy_restatement(name):
    from maskedsst_amd.ops import confusion_report
    cm = np.array(MATRICES[name], dtype=np.int64)
    ref = report_reference(cm)
    for given in (cm, torch.from_numpy(cm), cm.tolist()):
        got = confusion_report(given)
        for key in ("oa", "aa", "kappa", "mean_f1", "mean_iou"):
            assert same(getattr(got, key), ref[key]), (name, key, getattr(got, key), ref[key])
        for key in ("precision", "recall", "f1", "iou"):
            v = getattr(got, key)
            assert v.dtype == np.float64 and np.array_equal(v, ref[key]), (name, key, v, ref[key])
        assert got.total == int(cm.sum()) and got.support.tolist() == cm.sum(axis=1).tolist()
    got = confusion_report(cm)
    if name == "perfect":
        assert got.oa == 1.0 and got.aa == 1.0 and got.kappa == 1.0 and got.mean_iou == 1.0 and got.mean_f1 == 1.0
    if name in ("pe_is_one", "one_class", "empty"):
        assert got.kappa != got.kappa
    if name == "pe_is_one":
        assert got.oa == 1.0 and got.aa == 1.0 and got.recall.tolist() == [0.0, 1.0]
    if name == "class_without_support":
        assert got.recall[1] == 0.0 and got.f1[1] == 0.0 and abs(got.aa - (4 / 7 + 6 / 10) / 2) <= 1e-15   # the mean of two classes
    if name == "class_never_predicted":
        assert got.precision[1] == 0.0 and got.iou[1] == 0.0 and abs(got.aa - (4 / 6 + 0 + 6 / 7) / 3) <= 1e-15
    if name == "all_wrong":
        assert got.oa == 0.0 and got.kappa == -1.0
    if name == "empty":
        assert all(getattr(got, k) != getattr(got, k) for k in ("oa", "aa", "mean_f1", "mean_iou"))


def test_confusion_report_refuses_what_is_no_matrix():
    from maskedsst_amd.ops import confusion_report
    with pytest.raises(ValueError, match="square"):
        confusion_report(np.zeros((2, 3)))
    with pytest.raises(ValueError, match="square"):
        confusion_report(np.zeros(4))


# ------------------------------------------------------------------------------------------------ the Python surface
def test_fused_criterion_keeps_its_weight_as_a_buffer():
    from maskedsst_amd.ops import FusedCrossEntropy
    w = torch.tensor([0.5, 2.0, 0.0, 1.25])
    crit = FusedCrossEntropy(ignore_index=-1, weight=w, label_smoothing=0.1)
    assert list(crit.state_dict()) == ["weight"] and torch.equal(crit.state_dict()["weight"], w)
    assert dict(crit.named_buffers())["weight"] is crit.weight and crit.weight is not w and not list(crit.parameters())
    assert crit.weight.dtype == torch.float32 and crit.label_smoothing == 0.1 and crit.ignore_index == -1 and crit.fused_stats
    r = repr(crit)
    assert "ignore_index=-1" in r and "weight=[0.5, 2, 0, 1.25]" in r and "label_smoothing=0.1" in r, r
    # .to() moves it with the module (a dtype here: no device needed); a state_dict round trip restores it
    assert crit.double().weight.dtype == torch.float64
    other = FusedCrossEntropy(weight=torch.ones(4))
    other.load_state_dict(FusedCrossEntropy(weight=w).state_dict())
    assert torch.equal(other.weight, w)
    # without a weight: no buffer in the state, the defaults in the repr
    plain = FusedCrossEntropy()
    assert plain.weight is None and not plain.state_dict() and plain.label_smoothing == 0.0
    assert "weight=None" in repr(plain) and "label_smoothing=0" in repr(plain) and "ignore_index=-1" in repr(plain)
    assert FusedCrossEntropy(-3, [1.0, 2.0]).weight.tolist() == [1.0, 2.0]   # a list is taken too
    for bad in (-0.1, 1.0):
        with pytest.raises(ValueError, match="label_smoothing"):
            FusedCrossEntropy(label_smoothing=bad)
    with pytest.raises(ValueError, match="weight"):
        FusedCrossEntropy(weight=torch.ones(2, 2))


def test_extended_cross_entropy_has_no_cpu_fallback():
    from maskedsst_amd.ops import cross_entropy_stats, FusedCrossEntropy
    from maskedsst_amd.scene import scene_report, SceneMetrics, SceneReport
    logits, labels = torch.randn(2, 8, 4, 4), torch.randint(-1, 8, (2, 4, 4))
    w = torch.rand(8) + 0.1
    for kw in (dict(weight=w), dict(label_smoothing=0.1), dict(confusion=True), dict(weight=w, label_smoothing=0.1, confusion=True)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            cross_entropy_stats(logits, labels, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FusedCrossEntropy(-1, w, 0.1)(logits, labels)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FusedCrossEntropy(-1)(logits, labels, return_stats=True, confusion=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scene_report(logits, torch.zeros(2, 4, 4, dtype=torch.int64), labels)
    assert SceneMetrics._fields == ("loss", "acc", "macro_acc") and SceneReport._fields == SceneMetrics._fields + ("report",)


def test_finetune_parser_takes_the_new_flags_and_the_defaults_change_nothing():
    import finetune
    from maskedsst_amd.ops import FusedCrossEntropy
    ap = finetune.build_parser()
    d = ap.parse_args([])
    assert d.class_weights == "none" and d.label_smoothing == 0.0 and d.val_report is False
    a = ap.parse_args(["--loss", "fused", "--class-weights", "inverse", "--label-smoothing", "0.1", "--val-scenes", "4", "--val-every", "10",
                       "--val-report"])
    assert a.class_weights == "inverse" and a.label_smoothing == 0.1 and a.val_report is True and a.loss == "fused"
    with pytest.raises(SystemExit):
        ap.parse_args(["--class-weights", "sqrt"])
    # the defaults: the criteria of before
    crit = finetune.make_criterion("torch", -1)
    assert type(crit) is torch.nn.CrossEntropyLoss and crit.ignore_index == -1 and crit.weight is None and crit.label_smoothing == 0.0
    assert not crit.state_dict()
    crit = finetune.make_criterion("fused", -1)
    assert type(crit) is FusedCrossEntropy and crit.ignore_index == -1 and crit.weight is None and crit.label_smoothing == 0.0
    # with the flags: the same arguments on both kinds
    w = torch.tensor([1.0, 0.0, 3.0])
    for kind, cls in (("torch", torch.nn.CrossEntropyLoss), ("fused", FusedCrossEntropy)):
        crit = finetune.make_criterion(kind, -1, w, 0.1)
        assert type(crit) is cls and torch.equal(crit.weight, w) and crit.label_smoothing == 0.1 and crit.ignore_index == -1
    # --class-weights inverse: 1 / frequency, mean 1 over the classes present, 0 for an absent class; ignored labels do not count
    label = torch.tensor([[0, 0, 0, 0, 2, 2, -1, -1], [0, 0, 3, 3, 3, 3, -1, 0]])
    got = finetune.inverse_frequency_weights(label, 5, -1)
    inv = np.array([13 / 7, 0.0, 13 / 2, 13 / 4, 0.0])
    want = inv / inv[[0, 2, 3]].mean()
    assert got.dtype == torch.float32 and got.shape == (5,) and np.allclose(got.numpy(), want, rtol=1e-6, atol=0)
    assert abs(float(got[[0, 2, 3]].mean()) - 1.0) <= 1e-6 and got[1] == 0 and got[4] == 0
    assert finetune.inverse_frequency_weights(torch.full((2, 3), -1), 4, -1).tolist() == [0.0] * 4
