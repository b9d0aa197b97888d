"""Gaussian (QDA / LDA) classification of frozen features, host side (no GPU needed): the C ABI of msst_gauss_score (additive under
MSST_VERSION 109) and its argument checks (they run before any HIP call, so null pointers, host buffers and no device are enough to
see them), the ValueError / RuntimeError surface of maskedsst_amd/gaussian.py, the flag of finetune.py, and the float64 restatement of
tests/gauss_util.py: it agrees with scikit-learn where that is importable, it tells itself apart from its mutations at the committed
bars, and its real-valued cases leave at most 1 % of their rows under the margin gap."""
import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch

import gauss_util as gu
import pca_util as pu

BADARG, UNSUPPORTED = -3, -2   # include/msst.h: MSST_ERR_BADARG, MSST_ERR_UNSUPPORTED


# --------------------------------------------------------------------------------------------------------------------- C ABI
def test_c_abi_declares_and_exports_the_entry_point():
    from ctypes import c_float, c_int, c_long, c_void_p
    from maskedsst_amd import _lib
    header = open(_lib.HEADER_PATH).read()
    assert _lib.header_version() == 109   # additive: the revision does not move
    lib = _lib.load()
    assert lib.msst_version() == 109
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    P = c_void_p
    # x, int x_layout, long rows, long plane, int dim, centres, tables, int n_tables, class_table (host), offsets, consts, int nc,
    # float max_d2, classes, distance, scores, int out_layout, stream
    sig = (c_int, [P, c_int, c_long, c_long, c_int, P, P, c_int, P, P, P, c_int, c_float, P, P, P, c_int, P])
    name = "msst_gauss_score"
    m = re.search(r"^int %s\(([^;]*)\);" % name, header, re.M)
    assert m and len(m.group(1).split(",")) == len(sig[1])
    assert name in _lib.declared_symbols() and _lib._SIGS[name] == sig
    assert re.search(r" T %s$" % name, out, re.M)
    fn = getattr(lib, name)
    assert (fn.restype, list(fn.argtypes)) == sig
    import maskedsst_amd
    for n in ("GaussianClassifier", "GaussianResult", "GaussianScene", "fit_gaussian", "gaussian_predict_scene"):
        assert n in maskedsst_amd.__all__ and hasattr(maskedsst_amd, n), n
    assert maskedsst_amd.GaussianResult._fields == ("classes", "scores", "distance")
    assert maskedsst_amd.GaussianScene._fields == ("classes", "scores", "distance", "cover")
    assert hasattr(maskedsst_amd.ViTSpatialSpectral, "gaussian_predict_scene")
    assert "msst_gauss.hip" in __import__("maskedsst_amd.build", fromlist=["SOURCES"]).SOURCES


def _ptr():
    buf = (ctypes.c_char * 1024)()
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)


def test_gauss_score_refuses_bad_arguments_before_launch():
    from maskedsst_amd import _lib
    lib = _lib.load()
    buf, p = _ptr()                                     # zeros: as a class_table, every id is 0
    names = ("x", "centres", "tables", "class_table", "offsets", "consts", "classes", "distance", "scores")

    def call(x_layout=0, rows=128, plane=1, dim=96, n_tables=1, nc=3, max_d2=float("inf"), out_layout=0, **ptr):
        a = {n: ptr.get(n, p) for n in names}
        return lib.msst_gauss_score(a["x"], x_layout, rows, plane, dim, a["centres"], a["tables"], n_tables, a["class_table"], a["offsets"],
                                    a["consts"], nc, max_d2, a["classes"], a["distance"], a["scores"], out_layout, None)

    null = {n: None for n in names}
    for bad in (dict(rows=-1), dict(dim=0), dict(dim=-96), dict(nc=0), dict(nc=-2), dict(n_tables=0), dict(n_tables=-1), dict(n_tables=4),
                dict(nc=128, n_tables=129)):
        assert call(**bad) == BADARG and call(**bad, **null) == BADARG, bad
        assert b"msst_gauss_score" in lib.msst_last_error(), bad
    for over in (dict(dim=95), dict(dim=128), dict(nc=129), dict(nc=200, n_tables=130), dict(rows=1 << 31)):
        assert call(**over) == UNSUPPORTED and call(**over, **null) == UNSUPPORTED, over
        assert b"msst_gauss_score" in lib.msst_last_error(), over
    for kw in (dict(x_layout=-1), dict(x_layout=2), dict(out_layout=-1), dict(out_layout=2)):
        assert call(**kw) == BADARG and b"msst_gauss_score" in lib.msst_last_error(), kw
    for plane in (0, -4, 5, 256):          # a map on either side: plane must divide rows = 128
        assert call(x_layout=1, plane=plane) == BADARG and call(out_layout=1, plane=plane) == BADARG, plane
        assert b"plane" in lib.msst_last_error()
    for bad in (-1.0, float("nan"), float("-inf")):
        assert call(max_d2=bad) == BADARG and b"max_d2" in lib.msst_last_error(), bad
    # rows == 0 is a no-op: nothing is read, nothing is launched -- but the sizes are still checked
    assert call(rows=0) == 0 and call(rows=0, **null) == 0 and call(rows=0, x_layout=1, plane=7, **null) == 0
    assert call(rows=0, nc=129) == UNSUPPORTED and call(rows=0, x_layout=3) == BADARG
    assert call(plane=5, **null) == BADARG and b"null" in lib.msst_last_error()      # plane is not read with rows on both sides
    for nc, T in ((1, 1), (128, 128), (128, 1)):                                      # the limits themselves are inside
        assert call(nc=nc, n_tables=T, rows=(1 << 31) - 1, **null) == BADARG and b"null" in lib.msst_last_error()
    for n in names[:-1]:
        assert call(**{n: None}) == BADARG and b"null" in lib.msst_last_error(), n
    assert call(x=ctypes.c_void_p(p.value + 4)) == BADARG                            # rows are read 16 bytes at a time
    assert call(tables=ctypes.c_void_p(p.value + 4)) == BADARG                       # ... and so are the tables
    for n in names:
        assert call(**{n: ctypes.c_void_p(p.value + 2)}) == BADARG and b"misaligned" in lib.msst_last_error(), n
    # a table id outside [0, n_tables), on the host copy the call is given: the last check, so everything else is in order here
    for ids, T in (([0, 1, 2], 2), ([0, -1, 0], 1), ([3, 0, 0], 3)):
        arr = (ctypes.c_int32 * 3)(*ids)
        assert call(n_tables=T, class_table=ctypes.cast(arr, ctypes.c_void_p)) == BADARG, ids
        assert b"msst_gauss_score" in lib.msst_last_error() and b"table id" in lib.msst_last_error()


# --------------------------------------------------------------------------------------------------------- the Python surface
def cpu_bank(n=60, nc=3):
    from maskedsst_amd import KnnBank
    bank = KnnBank.__new__(KnnBank)
    bank.features, bank.labels, bank.n_classes = torch.randn(n, 96), (torch.arange(n) % nc).to(torch.int32), nc
    return bank


def given_clf(nc=3, tied=False, **kw):
    from maskedsst_amd import GaussianClassifier
    cov = np.eye(96) if tied else np.stack([np.eye(96) * (c + 1) for c in range(nc)])
    args = dict(means=np.zeros((nc, 96)), covariances=cov, priors=np.ones(nc), tied=tied)
    args.update(kw)
    return GaussianClassifier(**args)


def test_fit_refuses_bad_arguments_before_device_work():
    from maskedsst_amd import fit_gaussian
    bank = cpu_bank()
    for kw in (dict(bank=None), dict(bank=torch.zeros(40, 96)), dict(covariance="diag"), dict(covariance=None), dict(shrinkage=-0.1),
               dict(shrinkage=1.5), dict(shrinkage="a"), dict(shrinkage=True), dict(priors="flat"), dict(priors=[1.0, 2.0]),
               dict(priors=[1.0, -1.0, 1.0]), dict(priors=[0.0, 0.0, 0.0]), dict(priors=[1.0, float("nan"), 1.0]), dict(ddof=-1), dict(ddof=1.0),
               dict(ddof=None), dict(rcond=-1e-3), dict(rcond=1.0), dict(rcond="small"), dict(rcond=None)):
        args = dict(bank=bank)
        args.update(kw)
        with pytest.raises(ValueError):
            fit_gaussian(**args)
    for kw in (dict(), dict(covariance="tied", shrinkage=0.5, priors="uniform", ddof=0, rcond=0), dict(priors=[1, 2, 3]),
               dict(priors=torch.tensor([0.2, 0.3, 0.5]))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):           # everything is in order but the device
            fit_gaussian(bank, **kw)


def test_classifier_checks_given_arrays_once():
    from maskedsst_amd import GaussianClassifier
    eye3 = np.stack([np.eye(96)] * 3)
    nan_mean = np.zeros((3, 96))
    nan_mean[1, 4] = np.nan
    dead = eye3.copy()
    dead[2] = 0.0
    for kw in (dict(means=np.zeros((3, 95))), dict(means=np.zeros(96)), dict(means=np.zeros((0, 96))), dict(means=np.zeros((129, 96)), priors=np.ones(129)),
               dict(means=np.zeros((3, 96), dtype=np.int64)), dict(means=nan_mean), dict(covariances=np.eye(96)), dict(covariances=eye3[:2]),
               dict(covariances=eye3, tied=True), dict(covariances=eye3.astype(np.int64)), dict(covariances=dead),
               dict(covariances=np.full((3, 96, 96), np.inf)), dict(priors=np.ones(2)), dict(priors=[1.0, -1.0, 1.0]), dict(priors=np.zeros(3)),
               dict(priors=[1.0, np.nan, 1.0]), dict(counts=[1, 2]), dict(counts=[1.0, 2.0, 3.0]), dict(counts=[1, -1, 1]), dict(counts=[0, 0, 0]),
               dict(rcond=1.0), dict(rcond=-0.1), dict(rcond=None)):
        args = dict(means=np.zeros((3, 96)), covariances=eye3, priors=np.ones(3))
        args.update(kw)
        with pytest.raises(ValueError):
            GaussianClassifier(**args)
    with pytest.raises(ValueError, match="class 2"):
        GaussianClassifier(np.zeros((3, 96)), dead, np.ones(3))
    clf = GaussianClassifier(torch.zeros(3, 96), dead, [2.0, 2.0, 0.0])        # a class with prior 0 needs no covariance
    assert clf.n_classes == 3 and not clf.tied and np.array_equal(clf.priors, [0.5, 0.5, 0.0]) and clf.counts is None
    assert clf.means.shape == (3, 96) and clf.means.dtype == torch.float32 and clf.covariances.dtype == np.float64
    assert np.array_equal(clf.logdet[:2], [0.0, 0.0]) and np.isnan(clf.logdet[2]) and clf.pooled_covariance is None
    assert clf._host["tables"].shape == (2, 96, 96) and list(clf._class_table) == [0, 1, 0]
    assert np.array_equal(clf._host["consts"], np.array([np.log(0.5) - gu.LOG_2PI_HALF_D] * 2 + [-np.inf]).astype(np.float32))
    tied = given_clf(4, tied=True, counts=[5, 0, 3, 2], priors=[5, 9, 3, 2], means=np.arange(4)[:, None] * np.ones((4, 96)))
    assert tied.tied and tied.covariances is None and tied.pooled_covariance.shape == (96, 96) and tied.logdet.shape == (1,)
    assert np.allclose(tied.priors, [0.5, 0.0, 0.3, 0.2], rtol=1e-15) and tied.priors[1] == 0 and tied._host["tables"].shape == (1, 96, 96)
    centre = tied._host["centres"][0]                                            # the count-weighted mean of the present classes
    assert np.allclose(centre, (0 * 5 + 2 * 3 + 3 * 2) / 10.0)
    assert np.allclose((tied._host["offsets"] ** 2).sum(axis=1), [96 * 1.2 ** 2, 0.0, 96 * 0.8 ** 2, 96 * 1.8 ** 2], rtol=1e-6)
    # the floor: eigenvalues below rcond x the largest are raised to it, not dropped
    lam = np.ones(96)
    lam[90:] = 1e-9
    low = GaussianClassifier(np.zeros((1, 96)), np.diag(lam)[None], [1.0], rcond=1e-4)
    assert abs(low.logdet[0] - 6 * np.log(1e-4)) < 1e-9
    assert np.allclose(np.sort((low._host["tables"][0] ** 2).sum(axis=1)), np.concatenate([np.ones(90), np.full(6, 1e4)]), rtol=1e-6)
    with pytest.raises(ValueError, match="singular"):
        lam0 = lam.copy()
        lam0[95] = 0.0
        GaussianClassifier(np.zeros((1, 96)), np.diag(lam0)[None], [1.0], rcond=0)


def test_classify_and_scene_calls_refuse_bad_arguments():
    from maskedsst_amd import ViTSpatialSpectral, gaussian_predict_scene
    clf = given_clf()
    for f in (torch.zeros(5, 95), torch.zeros(96), torch.zeros(0, 96), torch.zeros(5, 96).double(), torch.zeros(96, 5).t(), [[0.0] * 96], None,
              torch.zeros(2, 95, 4, 4)):
        with pytest.raises(ValueError):
            clf.classify(f)
    for md in (-1.0, float("nan"), "far", True):
        with pytest.raises(ValueError, match="max_distance"):
            clf.classify(torch.zeros(5, 96), max_distance=md)
    for q in (-0.1, 1.5, None, True):
        with pytest.raises(ValueError, match="quantile"):
            clf.threshold(cpu_bank(), quantile=q)
    with pytest.raises(ValueError, match="KnnBank"):
        clf.threshold(torch.zeros(5, 96))
    for call in (lambda: clf.classify(torch.zeros(5, 96)), lambda: clf.classify(torch.zeros(5, 96), scores=False, max_distance=3.0),
                 lambda: clf.classify(torch.zeros(2, 96, 4, 4)), lambda: clf.classify(cpu_bank()), lambda: clf.threshold(cpu_bank()),
                 lambda: given_clf(tied=True).classify(torch.zeros(5, 96))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    torch.manual_seed(5)
    enc = ViTSpatialSpectral(image_size=8, spatial_patch_size=1, spectral_patch_size=10, num_classes=4, dim=96, depth=1, heads=8, mlp_dim=64,
                             channels=50, spectral_pos=torch.arange(5), blockwise_patch_embed=True)
    scene = torch.zeros(2, 50, 16, 16)
    for kw in (dict(clf=None), dict(clf=torch.eye(96)), dict(max_distance=-2.0), dict(scene=torch.zeros(2, 40, 16, 16)), dict(scene=torch.zeros(50, 16, 16)),
               dict(stride=9), dict(stride=0), dict(max_windows=0)):
        args = dict(scene=scene, clf=clf)
        args.update(kw)
        with pytest.raises(ValueError):
            enc.gaussian_predict_scene(**args)
        with pytest.raises(ValueError):
            gaussian_predict_scene(enc, **args)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc.gaussian_predict_scene(scene, clf)
    assert enc.training   # nothing above touched the module's mode


def test_finetune_parser_takes_val_gauss():
    import finetune
    ap = finetune.build_parser()
    assert ap.parse_args(["enmap"]).val_gauss is None
    a = ap.parse_args(["enmap", "--val-scenes", "4", "--val-every", "1", "--val-gauss", "tied"])
    assert a.val_gauss == "tied"
    with pytest.raises(SystemExit):
        ap.parse_args(["enmap", "--val-gauss", "diag"])
    with pytest.raises(SystemExit):
        finetune.check_val_gauss(ap.parse_args(["enmap", "--val-gauss", "full"]))                 # needs --val-scenes and --val-every
    with pytest.raises(SystemExit):
        finetune.check_val_gauss(ap.parse_args(["enmap", "--val-scenes", "4", "--val-gauss", "full"]))
    finetune.check_val_gauss(a)
    finetune.check_val_gauss(ap.parse_args(["enmap"]))


# ------------------------------------------------------------------------------------------------ the float64 restatement itself
def test_exact_reference_rules():
    """the whole-number reference: NaN rows, ties to the lowest index, a class with the constant -inf, rejection at the distance"""
    x = gu.int_rows(321, "ends")
    for nc in gu.INT_NC:
        for form in gu.INT_FORMS:
            tab = gu.int_tables(nc, form, duplicate=True, zero_prior=True)
            classes, distance, scores = gu.int_reference(x, tab)
            assert classes[0] == classes[-1] == -1 and np.isnan(distance[[0, -1]]).all() and np.isnan(scores[[0, -1]]).all()
            inner = classes[1:-1]
            assert (inner >= 0).all() and (inner < nc).all() and not np.isnan(scores[1:-1]).any()
            if nc > 1:
                assert (inner != 0).all() and (inner != nc - 1).all() or nc == 2      # class 0 is -inf; its copy, the last, ties with it
                assert np.isneginf(scores[1:-1, 0]).all() and np.isneginf(scores[1:-1, nc - 1]).all()
                if nc > 2:                                                           # (two classes: both -inf, class 0 by the order)
                    assert np.array_equal(distance[1:-1], 2 * (tab["consts"][inner] - scores[np.arange(1, 320), inner]))
    tab = gu.int_tables(17, "tied", duplicate=True)
    classes, distance, scores = gu.int_reference(gu.int_rows(321), tab)
    assert np.array_equal(scores[:, 0], scores[:, 16]) and (classes != 16).all() and (classes == 0).any()
    k = int(np.argmax(classes == 0))
    at = gu.int_reference(gu.int_rows(321), tab, max_d2=float(distance[k]))[0]
    below = gu.int_reference(gu.int_rows(321), tab, max_d2=float(np.nextafter(distance[k], np.float32(0))))[0]
    assert at[k] == 0 and below[k] == -2


def test_restatement_against_scikit_learn():
    """fit64 + score64 are scikit-learn's QDA (full covariances) and LDA (a tied one) where the two define the same thing: store_covariance
    QDA divides by n_c - 1; LDA's lsqr solver pools with the PRIORS as weights and ddof 0 -- restated here from the class moments"""
    pytest.importorskip("sklearn")
    from sklearn.discriminant_analysis import LinearDiscriminantAnalysis, QuadraticDiscriminantAnalysis
    x, labels, nc = gu.fit_bank()
    keep = labels != 5
    x64, y = x[keep].astype(np.float64), labels[keep]
    test = gu.real_rows(3000, 16, "full")[0][:400]
    test = test[np.isfinite(test).all(axis=1)].astype(np.float64)
    ref = gu.fit64(x[keep], y, nc, rcond=0.0)
    qda = QuadraticDiscriminantAnalysis(store_covariance=True).fit(x64, y)
    present = [0, 1, 3, 4]
    assert list(qda.classes_) == present
    for k, c in enumerate(present):
        assert pu.relmax(qda.covariance_[k], ref["covariances"][c]) < 1e-9 and pu.relmax(qda.means_[k], ref["means"][c]) < 1e-12
    assert pu.relmax(qda.priors_, ref["priors"][present]) < 1e-12
    classes, scores, _ = gu.score64(test.astype(np.float32), ref)
    # sklearn's decision function is the log joint density without the 48 log(2 pi)
    assert pu.relmax(qda.decision_function(test), scores[:, present] + gu.LOG_2PI_HALF_D) < 1e-7
    assert np.array_equal(qda.predict(test), classes)
    # LDA: one covariance.  sklearn (lsqr) pools sum_c prior_c cov_c(ddof 0); ours sum_c (n_c - 1) cov_c(ddof 1) / sum_c (n_c - 1) --
    # the same matrix up to the factor n / (n - classes): give the restatement sklearn's matrix and compare the decisions
    lda = LinearDiscriminantAnalysis(solver="lsqr", store_covariance=True).fit(x64, y)
    tied = gu.fit64(x[keep], y, nc, covariance="tied", rcond=0.0)
    n = len(y)
    assert pu.relmax(lda.covariance_ * n / (n - len(present)), tied["pooled"]) < 1e-9
    model = dict(means=tied["means"], covariances=lda.covariance_, priors=tied["priors"], tied=True, rcond=0.0)
    classes_t, scores_t, _ = gu.score64(test.astype(np.float32), model)
    assert np.array_equal(lda.predict(test), classes_t)
    # (LDA's decision function drops the terms common to all classes: compare the differences between classes)
    dec = lda.decision_function(test)
    ours = scores_t[:, present]
    assert pu.relmax(dec - dec[:, :1], ours - ours[:, :1]) < 1e-7


def test_fit_restatement_rules():
    x, labels, nc = gu.fit_bank()
    f = gu.fit64(x, labels, nc)
    assert list(f["counts"]) == [700, 450, 0, 230, 520, 300] and f["priors"][2] == 0 and abs(f["priors"].sum() - 1) < 1e-15
    for c in (0, 1, 3, 4, 5):
        rows = x[labels == c].astype(np.float64)
        assert pu.relmax(f["class_cov"][c], np.cov(rows, rowvar=False)) < 1e-11 and pu.relmax(f["means"][c], rows.mean(axis=0)) < 1e-13
    w = np.array([699, 449, 0, 229, 519, 299.0])
    assert pu.relmax(f["pooled"], sum(w[c] * f["class_cov"][c] for c in range(nc)) / w.sum()) < 1e-14
    assert np.isnan(f["logdet"][2]) and np.isfinite(np.delete(f["logdet"], 2)).all()
    s = gu.fit64(x, labels, nc, shrinkage=0.3)
    assert pu.relmax(s["covariances"][3], 0.7 * f["class_cov"][3] + 0.3 * f["pooled"]) < 1e-15
    one = gu.fit64(x, labels, nc, shrinkage=1.0)
    t = gu.fit64(x, labels, nc, covariance="tied")
    assert np.array_equal(one["covariances"][4], t["covariances"]) and t["logdet"].shape == (1,) and abs(one["logdet"][0] - t["logdet"][0]) < 1e-12
    u = gu.fit64(x, labels, nc, priors="uniform")
    assert np.array_equal(u["priors"], [0.2, 0.2, 0.0, 0.2, 0.2, 0.2])
    xs, ls, _ = gu.fit_bank(single=True)
    single = gu.fit64(xs, ls, nc, covariance="tied")
    assert single["counts"][5] == 1 and np.isnan(single["class_cov"][5]).all() and np.isfinite(single["pooled"]).all()
    assert np.array_equal(single["means"][5], xs[ls == 5][0].astype(np.float64))
    # the trace identity: under full covariances with nothing floored the own-class distances sum to sum_c (n_c - ddof) x 96
    _, _, cov = gu.class_moments64(x, labels, nc)
    total = 0.0
    for c in (0, 1, 3, 4, 5):
        lam = np.linalg.eigvalsh(cov[c])
        assert lam[0] > 1e-6 * lam[-1]
        a, _ = gu.whitening64(cov[c])
        z = (x[labels == c].astype(np.float64) - f["means"][c]) @ a.T
        total += (z * z).sum()
    assert abs(total - w.sum() * 96) <= 1e-9 * w.sum() * 96


def test_real_cases_leave_few_rows_under_the_margin_gap():
    """the classes of a real-valued case are compared on every row whose float64 top-two margin reaches the gap, 4 x the measured
    score error: computed from the float64 reference alone, at most 1 % of a case's rows lie under it.  (Without a committed
    measurement the gap of an fp32 chain of 96 + 96 terms on the largest score, 1e-4 of it, stands in.)"""
    for M, nc, form in gu.REAL_CASES:
        classes, scores, distance, margin = gu.real_reference(M, nc, form)
        x, labels = gu.real_rows(M, nc, form)
        assert (classes == -1).sum() == gu.REAL_NAN_ROWS and np.isnan(distance).sum() == gu.REAL_NAN_ROWS
        assert (classes[classes >= 0] == labels[classes >= 0]).mean() > 0.99                     # separated classes
        bar = gu.bars(gu.real_name(M, nc, form))
        rel = 1e-4 if bar is None else bar["scores"]
        gap = rel * np.nanmax(np.abs(scores))
        share = gu.under_gap(margin, classes, gap)
        print(f"{gu.real_name(M, nc, form)}: gap {gap:.3g}, {share:.4%} of the rows under it")
        assert share <= gu.MARGIN_SHARE, (M, nc, form, gap, share)


def test_committed_bars_tell_the_mutants_apart():
    """every bar is 4 x a committed measurement, and every mutated restatement lies beyond a bar of the case that is there to catch it
    (or, where the GPU comparison is exact, differs)"""
    def beyond(err, bar):
        return [q for q in err if not err[q] <= bar[q]]

    x, labels, nc = gu.fit_bank()
    for covariance, shrinkage in gu.FIT_CASES:
        bar = gu.bars(gu.fit_name(covariance, shrinkage))
        assert bar is not None, "profiles/gauss_parity_measured.jsonl is not committed: nothing to hold the mutants against"
        assert set(bar) == set(gu.FIT_QUANTITIES) and all(0 <= v < 1e-3 for v in bar.values()), bar
        ref = gu.fit64(x, labels, nc, covariance, shrinkage)
        for mutant in ("ddof0", "pooled_by_n"):
            if mutant == "pooled_by_n" and covariance == "full" and shrinkage == 0:
                continue                                               # (nothing pooled enters the classifier there)
            err = gu.fit_errors(gu.fit64(x, labels, nc, covariance, shrinkage, mutant=mutant), ref)
            assert beyond(err, bar), (covariance, shrinkage, mutant, err, bar)
            assert "pooled" in beyond(err, bar), (covariance, shrinkage, mutant, err, bar)
    for M, nc_, form in ((3000, 3, "full"), (3000, 16, "full"), (3000, 16, "tied")):
        bar = gu.bars(gu.real_name(M, nc_, form))
        assert set(bar) == {"scores", "distance"} and all(0 <= v < 1e-4 for v in bar.values()), bar
        xr, _ = gu.real_rows(M, nc_, form)
        classes, scores, distance, _ = gu.real_reference(M, nc_, form)
        model = gu.real_model(nc_, form)
        for mutant in ("no_logdet", "no_prior", "whiten_by_lambda", "centre_not_subtracted"):
            if mutant == "no_logdet" and form == "tied":
                continue                                               # (one logdet for all classes: the full cases catch it)
            _, ms, md = gu.score64(xr, model, mutant=mutant)
            err = dict(scores=gu.relmax(ms, scores), distance=gu.relmax(md, distance))
            assert "scores" in beyond(err, bar), (M, nc_, form, mutant, err, bar)
            if mutant in ("whiten_by_lambda", "centre_not_subtracted"):
                assert "distance" in beyond(err, bar), (M, nc_, form, mutant, err, bar)
    # the floor: a class with fewer rows than dimensions has eigenvalues of 0 -- floored they give finite scores, unfloored none
    bar = gu.bars(gu.real_name(3000, 3, "full"))
    low = dict(gu.real_model(3, "full"))
    cov = low["covariances"].copy()
    w, v = np.linalg.eigh(cov[1])
    w[:30] = 0.0
    cov[1] = (v * w) @ v.T
    low["covariances"] = cov
    xr = gu.real_rows(3000, 3, "full")[0][:300]
    _, good, gd = gu.score64(xr, low)
    _, broken, bd = gu.score64(xr, low, mutant="no_floor")
    ok = np.isfinite(xr).all(axis=1)
    assert np.isfinite(good[ok]).all() and not np.isfinite(broken[ok][:, 1]).any()
    # ties: the comparison is exact there (duplicated classes in tests/test_gpu_gauss.py), and the mutant differs
    model = dict(means=np.zeros((2, 96)), covariances=np.stack([np.eye(96)] * 2), priors=[0.5, 0.5], tied=False)
    pts = np.random.default_rng(0).standard_normal((50, 96)).astype(np.float32)
    assert (gu.score64(pts, model)[0] == 0).all() and (gu.score64(pts, model, mutant="ties_highest")[0] == 1).all()
    assert set(gu.MUTANTS) == {"no_logdet", "no_prior", "ddof0", "pooled_by_n", "whiten_by_lambda", "centre_not_subtracted", "no_floor", "ties_highest"}
