"""PCA, whitening and RX scores of frozen features, host side (no GPU needed): the C ABI of msst_feat_moments_scratch_floats /
msst_feat_moments / msst_feat_moments_finish / msst_feat_project (additive under MSST_VERSION 109) and their argument checks (they
run before any HIP call, so null pointers, host buffers and no device are enough to see them), the ValueError / RuntimeError surface
of maskedsst_amd/pca.py, the host eigen rules, the flag of finetune.py, and the float64 restatement of tests/pca_util.py: it tells
itself apart from its mutations at the committed bars, and it satisfies the trace identity."""
import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch

import pca_util as pu

BADARG, UNSUPPORTED = -3, -2   # include/msst.h: MSST_ERR_BADARG, MSST_ERR_UNSUPPORTED
SLAB = 1 + 96 + 96 * 96        # floats of a workgroup's slab row: n | s1 | s2


# --------------------------------------------------------------------------------------------------------------------- C ABI
def test_c_abi_declares_and_exports_the_entry_points():
    from ctypes import c_int, c_long, c_void_p
    from maskedsst_amd import _lib
    header = open(_lib.HEADER_PATH).read()
    assert _lib.header_version() == 109   # additive: the revision does not move
    lib = _lib.load()
    assert lib.msst_version() == 109
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    P = c_void_p
    sigs = {
        # long rows
        "msst_feat_moments_scratch_floats": (c_long, [c_long]),
        # x, int x_layout, long rows, long plane, int dim, centre, slab, long slab_floats, stream
        "msst_feat_moments": (c_int, [P, c_int, c_long, c_long, c_int, P, P, c_long, P]),
        # slab, long slab_floats, long rows, int dim, centre, int ddof, count, mean, cov, raw, stream
        "msst_feat_moments_finish": (c_int, [P, c_long, c_long, c_int, P, c_int, P, P, P, P, P]),
        # x, int x_layout, long rows, long plane, int dim, mean, components, int r, out, int out_layout, sumsq, stream
        "msst_feat_project": (c_int, [P, c_int, c_long, c_long, c_int, P, P, c_int, P, c_int, P, P]),
    }
    for name, sig in sigs.items():
        m = re.search(r"^(int|long) %s\(([^;]*)\);" % name, header, re.M)
        assert m, name
        assert len(m.group(2).split(",")) == len(sig[1]), name                # the header's argument count
        assert name in _lib.declared_symbols() and _lib._SIGS[name] == sig, name
        assert re.search(r" T %s$" % name, out, re.M), name
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == sig, name
    import maskedsst_amd
    for name in ("FeaturePCA", "PcaScene", "AnomalyScene", "fit_pca", "pca_scene", "anomaly_scene"):
        assert name in maskedsst_amd.__all__ and hasattr(maskedsst_amd, name), name
    assert maskedsst_amd.PcaScene._fields == ("components", "cover")
    assert maskedsst_amd.AnomalyScene._fields == ("score", "cover", "pca")
    assert hasattr(maskedsst_amd.ViTSpatialSpectral, "pca_scene") and hasattr(maskedsst_amd.ViTSpatialSpectral, "anomaly_scene")
    assert "msst_pca.hip" in __import__("maskedsst_amd.build", fromlist=["SOURCES"]).SOURCES


def _ptr():
    buf = (ctypes.c_char * 64)()
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)


def test_scratch_floats():
    from maskedsst_amd import _lib
    f = _lib.load().msst_feat_moments_scratch_floats
    assert f(1) == SLAB and f(64) == SLAB and f(65) == 2 * SLAB and f(512 * 64) == 512 * SLAB
    assert f(512 * 64 + 1) == 257 * SLAB                        # two tiles per workgroup from here on
    assert f(262144) == 512 * SLAB and f((1 << 31) - 1) == 512 * SLAB
    for bad in (0, -1, 1 << 31):
        assert f(bad) == 0, bad


def test_feat_moments_refuses_bad_arguments_before_launch():
    from maskedsst_amd import _lib
    lib = _lib.load()
    buf, p = _ptr()
    names = ("x", "centre", "slab")

    def call(x_layout=0, rows=128, plane=1, dim=96, slab_floats=None, **ptr):
        a = {n: ptr.get(n, p) for n in names}
        if slab_floats is None:
            slab_floats = lib.msst_feat_moments_scratch_floats(rows)
        return lib.msst_feat_moments(a["x"], x_layout, rows, plane, dim, a["centre"], a["slab"], slab_floats, None)

    null = {n: None for n in names}
    for bad in (dict(rows=0), dict(rows=-3), dict(dim=0), dict(dim=-96)):
        assert call(**bad) == BADARG and call(**bad, **null) == BADARG, bad
    assert b"msst_feat_moments" in lib.msst_last_error()
    for over in (dict(dim=95), dict(dim=128), dict(rows=1 << 31)):
        assert call(slab_floats=1 << 40, **over) == UNSUPPORTED and call(slab_floats=0, **over, **null) == UNSUPPORTED, over
    assert b"msst_feat_moments" in lib.msst_last_error()
    for layout in (-1, 2):
        assert call(x_layout=layout) == BADARG, layout
    for plane in (0, -4, 5, 256):          # layout 1: plane must divide rows = 128
        assert call(x_layout=1, plane=plane) == BADARG, plane
    assert call(plane=5, **null) == BADARG and b"null" in lib.msst_last_error()      # plane is not read in layout 0
    assert call(rows=(1 << 31) - 1, **null) == BADARG and b"null" in lib.msst_last_error()   # the limit itself is inside
    for n in ("x", "slab"):
        assert call(**{n: None}) == BADARG, n
    assert b"null" in lib.msst_last_error()
    assert call(centre=None, slab_floats=0) == BADARG and b"slab" in lib.msst_last_error()    # a null centre is zeros: the next check refuses
    assert call(x=ctypes.c_void_p(p.value + 4)) == BADARG                            # rows are read 16 bytes at a time
    assert call(x_layout=1, plane=64, x=ctypes.c_void_p(p.value + 4), slab_floats=0) == BADARG and b"slab" in lib.msst_last_error()
    for n in names:
        assert call(**{n: ctypes.c_void_p(p.value + 2)}) == BADARG, n
    need = lib.msst_feat_moments_scratch_floats(128)
    assert need == 2 * SLAB and call(slab_floats=need - 1) == BADARG and b"slab" in lib.msst_last_error()


def test_feat_moments_finish_refuses_bad_arguments_before_launch():
    from maskedsst_amd import _lib
    lib = _lib.load()
    buf, p = _ptr()
    names = ("slab", "centre", "count", "mean", "cov", "raw")

    def call(rows=100, dim=96, ddof=1, slab_floats=None, **ptr):
        a = {n: ptr.get(n, p) for n in names}
        if slab_floats is None:
            slab_floats = lib.msst_feat_moments_scratch_floats(rows)
        return lib.msst_feat_moments_finish(a["slab"], slab_floats, rows, dim, a["centre"], ddof, a["count"], a["mean"], a["cov"], a["raw"], None)

    null = {n: None for n in names}
    for bad in (dict(rows=0), dict(rows=-1), dict(dim=0), dict(ddof=-1)):
        assert call(**bad) == BADARG and call(**bad, **null) == BADARG, bad
    for over in (dict(dim=95), dict(dim=97), dict(rows=1 << 31)):
        assert call(slab_floats=1 << 40, **over) == UNSUPPORTED and call(**over, **null) == UNSUPPORTED, over
    assert b"msst_feat_moments_finish" in lib.msst_last_error()
    for n in ("slab", "count", "mean"):
        assert call(**{n: None}) == BADARG, n
    assert b"null" in lib.msst_last_error()
    for n in names:
        assert call(**{n: ctypes.c_void_p(p.value + 2)}) == BADARG, n
    assert call(count=ctypes.c_void_p(p.value + 4)) == BADARG and b"null or misaligned" in lib.msst_last_error()     # an int64
    # centre, cov and raw are optional: with them null the next refusal is the slab's size
    assert call(centre=None, cov=None, raw=None, slab_floats=SLAB - 1) == BADARG and b"slab" in lib.msst_last_error()
    assert call(slab_floats=lib.msst_feat_moments_scratch_floats(100) - 1) == BADARG and b"slab" in lib.msst_last_error()


def test_feat_project_refuses_bad_arguments_before_launch():
    from maskedsst_amd import _lib
    lib = _lib.load()
    buf, p = _ptr()
    names = ("x", "mean", "components", "out", "sumsq")

    def call(x_layout=0, rows=128, plane=1, dim=96, r=3, out_layout=0, **ptr):
        a = {n: ptr.get(n, p) for n in names}
        return lib.msst_feat_project(a["x"], x_layout, rows, plane, dim, a["mean"], a["components"], r, a["out"], out_layout, a["sumsq"], None)

    null = {n: None for n in names}
    for bad in (dict(rows=0), dict(rows=-3), dict(dim=0)):
        assert call(**bad) == BADARG and call(**bad, **null) == BADARG, bad
    assert b"msst_feat_project" in lib.msst_last_error()
    for over in (dict(dim=95), dict(dim=128), dict(r=0), dict(r=-1), dict(r=97), dict(r=128), dict(rows=1 << 31)):
        assert call(**over) == UNSUPPORTED and call(**over, **null) == UNSUPPORTED, over
    assert b"msst_feat_project" in lib.msst_last_error()
    for kw in (dict(x_layout=-1), dict(x_layout=2), dict(out_layout=-1), dict(out_layout=2)):
        assert call(**kw) == BADARG, kw
    for plane in (0, -4, 5, 256):          # a map on either side: plane must divide rows = 128
        assert call(x_layout=1, plane=plane) == BADARG and call(out_layout=1, plane=plane) == BADARG, plane
    assert call(plane=5, **null) == BADARG and b"null" in lib.msst_last_error()      # plane is not read with rows on both sides
    for r in (1, 96):                                                                # the limits themselves are inside
        assert call(r=r, rows=(1 << 31) - 1, **null) == BADARG and b"null" in lib.msst_last_error()
    for n in ("x", "mean", "components"):
        assert call(**{n: None}) == BADARG, n
    assert b"null" in lib.msst_last_error()
    assert call(x=ctypes.c_void_p(p.value + 4)) == BADARG                            # rows are read 16 bytes at a time
    for n in names:
        assert call(**{n: ctypes.c_void_p(p.value + 2)}) == BADARG, n
    assert call(out=None, sumsq=None) == BADARG and b"both outputs null" in lib.msst_last_error()


# --------------------------------------------------------------------------------------------------------- the Python surface
def make_encoder(**kw):
    from maskedsst_amd import ViTSpatialSpectral
    torch.manual_seed(5)
    args = dict(image_size=8, spatial_patch_size=1, spectral_patch_size=10, num_classes=4, dim=96, depth=1, heads=8, mlp_dim=64,
                channels=50, spectral_pos=torch.arange(5), blockwise_patch_embed=True)
    args.update(kw)
    return ViTSpatialSpectral(**args)


def given_pca(r=96, lam=None):
    from maskedsst_amd import FeaturePCA
    lam = np.exp(-np.arange(96) / 24.0) if lam is None else lam
    return FeaturePCA(torch.zeros(96), torch.eye(96)[:r].contiguous(), lam, 100)


def test_fit_refuses_bad_arguments_before_device_work():
    from maskedsst_amd import KnnBank, SceneEmbedding, fit_pca
    x = torch.randn(40, 96)
    for kw in (dict(features=None), dict(features=torch.zeros(40, 95)), dict(features=torch.zeros(96)), dict(features=torch.zeros(40, 96).double()),
               dict(features=torch.zeros(96, 40).t()), dict(features=[[0.0] * 96]), dict(features=torch.zeros(0, 96)),
               dict(features=torch.zeros(2, 95, 4, 4)), dict(features=torch.zeros(2, 96, 4, 4).double()), dict(features=torch.zeros(2, 96, 0, 4)),
               dict(features=torch.zeros(2, 4, 96, 4).permute(0, 2, 1, 3)), dict(features=torch.zeros(2, 96, 4)),
               dict(n_components=0), dict(n_components=97), dict(n_components=3.0), dict(n_components=True),
               dict(ddof=-1), dict(ddof=1.0), dict(ddof=None), dict(rcond=-1e-3), dict(rcond=1.0), dict(rcond="small"), dict(rcond=None)):
        args = dict(features=x)
        args.update(kw)
        with pytest.raises(ValueError):
            fit_pca(**args)
    bank = KnnBank.__new__(KnnBank)
    bank.features, bank.labels, bank.n_classes = x, torch.zeros(40, dtype=torch.int32), 2
    emb = SceneEmbedding(torch.zeros(2, 96, 4, 4), torch.ones(2, 4, 4, dtype=torch.int32))
    for args in (dict(features=x), dict(features=x, n_components=1, ddof=0, rcond=0), dict(features=bank, n_components=96),
                 dict(features=torch.zeros(2, 96, 4, 4)), dict(features=emb)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):           # everything is in order but the device
            fit_pca(**args)


def test_feature_pca_checks_given_arrays_once():
    from maskedsst_amd import FeaturePCA
    lam = np.exp(-np.arange(96) / 24.0)
    mean, comp = torch.zeros(96), torch.eye(96)
    asc = lam[::-1].copy()
    neg = lam.copy()
    neg[-1] = -1e-9
    nan_mean = torch.zeros(96)
    nan_mean[3] = float("nan")
    for kw in (dict(mean=torch.zeros(95)), dict(mean=torch.zeros(96).double()), dict(mean=[0.0] * 96), dict(mean=nan_mean),
               dict(components=torch.eye(95)), dict(components=torch.zeros(96)), dict(components=torch.zeros(0, 96)), dict(components=torch.zeros(97, 96)),
               dict(components=torch.eye(96).double()), dict(components=torch.full((3, 96), float("inf"))),
               dict(explained_variance=lam[:95]), dict(explained_variance=asc), dict(explained_variance=neg),
               dict(explained_variance=np.full(96, np.nan)), dict(count=-1), dict(count=2.0), dict(rcond=1.0), dict(rcond=-0.1)):
        args = dict(mean=mean, components=comp, explained_variance=lam, count=100)
        args.update(kw)
        with pytest.raises(ValueError):
            FeaturePCA(**args)
    pca = FeaturePCA(mean, comp[:3].contiguous(), torch.from_numpy(lam), 100)
    assert pca.n_components == 3 and pca.rank == 96 and pca.count == 100 and pca.explained_variance.dtype == np.float64
    evr, erank = pu.spectrum64(lam)
    assert np.array_equal(pca.explained_variance_ratio, evr) and pca.effective_rank == erank
    assert abs(given_pca(lam=np.ones(96)).effective_rank - 96.0) < 1e-9                       # isotropic
    one = np.zeros(96)
    one[0] = 2.0
    collapsed = given_pca(lam=one)
    assert collapsed.effective_rank == 1.0 and collapsed.rank == 1 and collapsed.explained_variance_ratio[0] == 1.0
    dead = given_pca(lam=np.zeros(96))
    assert dead.rank == 0 and np.isnan(dead.effective_rank)
    for f in (torch.zeros(5, 95), torch.zeros(96), torch.zeros(0, 96), torch.zeros(5, 96).double(), torch.zeros(96, 5).t(), [[0.0] * 96]):
        with pytest.raises(ValueError):
            pca.transform(f)
        with pytest.raises(ValueError):
            given_pca().mahalanobis(f)
    with pytest.raises(ValueError, match="leading components"):
        pca.mahalanobis(torch.zeros(5, 96))                                # 3 components kept, rank 96
    for call in (lambda: pca.transform(torch.zeros(5, 96)), lambda: pca.transform(torch.zeros(5, 96), whiten=True),
                 lambda: given_pca().mahalanobis(torch.zeros(5, 96))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_scene_calls_refuse_bad_arguments():
    from maskedsst_amd import anomaly_scene, pca_scene
    enc = make_encoder()
    pca = given_pca()
    scene = torch.zeros(2, 50, 16, 16)
    for kw in (dict(pca=None), dict(pca=torch.eye(96)), dict(scene=torch.zeros(2, 40, 16, 16)), dict(scene=torch.zeros(50, 16, 16)),
               dict(scene=torch.zeros(2, 50, 4, 16)), dict(stride=9), dict(stride=0), dict(max_windows=0)):
        args = dict(scene=scene, pca=pca)
        args.update(kw)
        with pytest.raises(ValueError):
            enc.pca_scene(**args)
        with pytest.raises(ValueError):
            pca_scene(enc, **args)
        if kw != dict(pca=None):                                           # pca=None: fitted on the scene itself
            with pytest.raises(ValueError):
                enc.anomaly_scene(**args)
            with pytest.raises(ValueError):
                anomaly_scene(enc, **args)
    for call in (lambda: enc.pca_scene(scene, pca), lambda: enc.pca_scene(scene, pca, whiten=True), lambda: enc.anomaly_scene(scene, pca),
                 lambda: enc.anomaly_scene(scene)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    assert enc.training   # nothing above touched the module's mode


def test_finetune_parser_takes_val_pca():
    import finetune
    ap = finetune.build_parser()
    assert ap.parse_args(["enmap"]).val_pca == 0
    a = ap.parse_args(["enmap", "--val-scenes", "4", "--val-every", "1", "--val-pca", "3"])
    assert a.val_pca == 3
    with pytest.raises(SystemExit):
        finetune.check_val_pca(ap.parse_args(["enmap", "--val-pca", "3"]))                     # needs --val-scenes and --val-every
    with pytest.raises(SystemExit):
        finetune.check_val_pca(ap.parse_args(["enmap", "--val-scenes", "4", "--val-pca", "3"]))
    for r in ("-3", "97"):
        with pytest.raises(SystemExit):
            finetune.check_val_pca(ap.parse_args(["enmap", "--val-scenes", "4", "--val-every", "1", "--val-pca", r]))
    finetune.check_val_pca(a)
    finetune.check_val_pca(ap.parse_args(["enmap"]))


# ------------------------------------------------------------------------------------------------------------ host eigen rules
def check_rules(lam, comp, cov):
    assert lam.shape == (96,) and comp.shape == (96, 96)
    assert (np.diff(lam) <= 0).all() and (lam >= 0).all()                                   # descending, clamped
    assert np.abs(comp @ comp.T - np.eye(96)).max() < 1e-12                                 # unit, orthogonal rows
    big = np.argmax(np.abs(comp), axis=1)                                                   # (argmax: the lowest index on a tie)
    assert (comp[np.arange(96), big] > 0).all()                                             # the sign rule
    assert np.abs((comp.T * lam) @ comp - cov).max() <= 1e-12 * max(np.abs(cov).max(), 1.0)


def test_eigen_rules_on_exact_zeros_and_a_repeated_eigenvalue():
    from maskedsst_amd.pca import FeaturePCA, eigen_rules
    g = np.random.default_rng(21)
    q, _ = np.linalg.qr(g.standard_normal((96, 96)))
    # exact zeros: ten directions carry variance, 86 none; eigh returns some of the zeros as -1e-17
    lam_true = np.concatenate([np.linspace(5.0, 0.5, 10), np.zeros(86)])
    cov = (q * lam_true) @ q.T
    cov = (cov + cov.T) / 2
    assert np.linalg.eigvalsh(cov).min() < 0                                                # there is something to clamp
    for lam, comp in (eigen_rules(cov), pu.eigen64(cov)):
        check_rules(lam, comp, cov)
        assert np.abs(lam - lam_true).max() < 1e-12 and lam.min() == 0.0
        assert pu.rank64(lam) == 10 and pu.rank64(lam, 0.55) == 5 and pu.rank64(lam, 0.0) <= 96
    lam, comp = eigen_rules(cov)
    pca = FeaturePCA(torch.zeros(96), torch.from_numpy(comp).float(), lam, 1000)
    assert pca.rank == 10 and FeaturePCA(torch.zeros(96), torch.from_numpy(comp).float(), lam, 1000, rcond=0.55).rank == 5
    assert np.abs(comp[:10] - pu.eigen64(cov)[1][:10]).max() < 1e-12                        # simple eigenvalues: the vectors themselves agree
    # the sign rule on a tie: entries of equal magnitude, the lowest index decides
    tie = np.zeros((96, 96))
    v = np.zeros(96)
    v[[4, 9]] = -np.sqrt(0.5), np.sqrt(0.5)
    tie += 3.0 * np.outer(v, v)
    lam_t, comp_t = eigen_rules(tie)
    assert abs(lam_t[0] - 3.0) < 1e-14 and comp_t[0, 4] > 0 and comp_t[0, 9] < 0
    # a repeated eigenvalue: the eigenvectors of the 3-fold value are any basis of its eigenspace -- compare through the projector
    lam_rep = np.concatenate([[4.0, 2.0, 2.0, 2.0, 1.0], np.exp(-np.arange(91) / 24.0) * 0.5])
    cov_r = (q * lam_rep) @ q.T
    cov_r = (cov_r + cov_r.T) / 2
    lam_a, comp_a = eigen_rules(cov_r)
    lam_b, comp_b = pu.eigen64(cov_r[::-1, ::-1])                                           # the same matrix with the channels reversed
    check_rules(lam_a, comp_a, cov_r)
    assert np.abs(lam_a - lam_rep).max() < 1e-12 and np.abs(lam_a - lam_b).max() < 1e-12
    proj_a = comp_a[1:4].T @ comp_a[1:4]
    proj_b = (comp_b[1:4].T @ comp_b[1:4])[::-1, ::-1]
    assert np.abs(proj_a - q[:, 1:4] @ q[:, 1:4].T).max() < 1e-10 and np.abs(proj_a - proj_b).max() < 1e-10


# ------------------------------------------------------------------------------------------------ the float64 restatement itself
def test_restatement_rules():
    x = pu.int_case(321, "tile")
    n, s1, s2 = pu.int_moments(x)
    n64, t1, t2 = pu.moments64(x)
    assert n == n64 == 321 - 64 and np.array_equal(s1, t1) and np.array_equal(s2, t2) and np.array_equal(s2, s2.T)
    mean, cov = pu.finish_exact(n, s1, s2, None, 1)
    m64, c64 = pu.finish64(n64, t1, t2, None, 1)
    assert pu.relmax(mean, m64) < 1e-7 and pu.relmax(cov, c64) < 1e-7
    ok = ~np.isnan(x).any(axis=1)
    assert pu.relmax(c64, np.cov(x[ok].astype(np.float64), rowvar=False)) < 1e-13 and pu.relmax(m64, x[ok].mean(axis=0, dtype=np.float64)) < 1e-13
    # a whole-number centre changes neither the mean nor the covariance
    nc, c1, c2 = pu.int_moments(x, pu.int_centre())
    mean_c, cov_c = pu.finish_exact(nc, c1, c2, pu.int_centre(), 1)
    assert np.abs(c1).min() > 0 and pu.relmax(mean_c, m64) < 1e-7 and pu.relmax(cov_c, c64) < 1e-7
    # every row NaN, one row, ddof beyond the count
    n0, z1, z2 = pu.int_moments(pu.int_case(65, "all"))
    mean0, cov0 = pu.finish_exact(n0, z1, z2, None, 1)
    assert n0 == 0 and np.isnan(mean0).all() and np.isnan(cov0).all()
    n1, o1, o2 = pu.int_moments(pu.int_case(1))
    mean1, cov1 = pu.finish_exact(n1, o1, o2, None, 1)
    assert n1 == 1 and np.array_equal(mean1, pu.int_case(1)[0]) and np.isnan(cov1).all()
    assert not np.isnan(pu.finish_exact(n1, o1, o2, None, 0)[1]).any()
    # the two-pass restatement is numpy's covariance of the counted rows
    xr = pu.real_case(3000, "offset")
    okr = np.isfinite(xr).all(axis=1)
    f = pu.fit64(xr)
    assert f["count"] == 3000 - pu.REAL_NAN_ROWS == int(okr.sum())
    assert pu.relmax(f["cov"], np.cov(xr[okr].astype(np.float64), rowvar=False)) < 1e-12
    assert 2.0e3 < f["eigenvalues"][0] / f["eigenvalues"][-1] < 4.0e3 and f["rank"] == 96
    # projection: NaN rows, and the map round trip of the cases
    mean, comp = pu.project_tables(17)
    assert np.abs(comp.astype(np.float64) @ comp.astype(np.float64).T - np.eye(17)).max() < 1e-6
    xp = pu.project_rows(65)
    out, ss = pu.project64(xp, mean, comp)
    bad = np.isnan(xp).any(axis=1)
    assert bad.sum() == 1 and np.isnan(out[bad]).all() and np.isnan(ss[bad]).all() and not np.isnan(out[~bad]).any()
    assert np.array_equal(pu.from_map(pu.to_map(xp, 5, 13)), xp, equal_nan=True)


def test_trace_identity():
    """the sum of the Mahalanobis distances of the counted fitted rows is (n - ddof) x rank: the whitened scores have the covariance I"""
    for M, form in ((32833, "well"), (3000, "offset")):
        x = pu.real_case(M, form)
        ok = np.isfinite(x).all(axis=1)
        for ddof in (1, 0):
            f = pu.fit64(x, ddof=ddof)
            total = pu.mahalanobis64(x[ok], f).sum()
            want = (f["count"] - ddof) * f["rank"]
            assert f["rank"] == 96 and abs(total - want) <= 1e-9 * want, (M, form, ddof, total, want)
    # ... and on a rank-deficient cloud, where only the `rank` leading directions count
    low = pu.real_case(3000, "well").copy()
    low = low[np.isfinite(low).all(axis=1)]
    low[:, 40:80] = low[:, :40] * 0.5
    low[:, 80:] = low[:, :16] - low[:, 16:32]
    f = pu.fit64(low)
    assert f["rank"] == 40 and abs(pu.mahalanobis64(low, f).sum() - (len(low) - 1) * 40) <= 1e-6 * len(low) * 40


def test_committed_bars_tell_the_mutants_apart():
    """every bar is 4 x a committed measurement, and every mutated restatement lies beyond a bar of the case that is there to catch it
    (or, where the GPU comparison is exact, differs).

    The one mutation no fp32 bar can see on real-valued data is the dropped correction term s1 s1^T / n of the second pass: with
    the first mean off by one fp32 ulp d, the term is n d^2 / (n - 1) = 1.4e-11 against covariance entries of order 1 (a relative
    1.4e-10 on the offset cases: printed below), five orders below fp32 resolution.  The comparison that catches it is the exact one:
    on whole-number data about a whole-number centre the finish is checked bit for bit (tests/test_gpu_pca.py), and there the
    mutant differs in every entry whose two residual sums are not zero."""
    for M in pu.REAL_ROWS:
        for form in pu.REAL_FORMS:
            bar = pu.bars(pu.case_name(M, form))
            assert set(bar) == set(pu.FIT_QUANTITIES)
            # fp32 kernels: no relative bar is looser than 1e-5 -- but for the mean of the zero-mean form, a rounding residue of
            # 1e-9 whose error is measured against itself
            assert all(0 <= v < (1e-3 if (form, q) == ("well", "mean") else 1e-5) for q, v in bar.items()), (M, form, bar)
    for r in pu.PROJECT_R:
        bar = pu.bars(f"project_r{r}")
        assert set(bar) == {"out", "sumsq"} and all(0 <= v < 1e-4 for v in bar.values()), (r, bar)
    assert set(pu.bars("transform_offset_3000")) == {"out", "whitened", "mahalanobis"} and all(0 <= v < 1e-3 for v in pu.bars("transform_offset_3000").values())
    for stride in (8, 5):
        assert 0 <= pu.bars(f"trace_scene_stride{stride}")["trace"] < 1e-2

    def beyond(err, bar):
        return [q for q in err if err[q] > bar[q]]

    for M in pu.REAL_ROWS:
        refs = {form: pu.fit64(pu.real_case(M, form)) for form in pu.REAL_FORMS}
        # the one-pass fp32 covariance: the case that motivates the two-pass design
        bar = pu.bars(pu.case_name(M, "offset"))
        err = pu.fit_errors(pu.fit64(pu.real_case(M, "offset"), mutant="one_pass_fp32"), refs["offset"])
        assert err["cov"] > 100 * bar["cov"] and "eigenvalues" in beyond(err, bar), (M, err, bar)
        for form in pu.REAL_FORMS:
            bar = pu.bars(pu.case_name(M, form))
            for mutant in ("ddof0", "nan_counted", "ascending"):
                err = pu.fit_errors(pu.fit64(pu.real_case(M, form), mutant=mutant), refs[form])
                assert beyond(err, bar), (M, form, mutant, err, bar)
        err =pu.fit_errors(pu.fit64(pu.real_case(M, "offset"), mutant="no_correction"), refs["offset"])
        print(f"no_correction on fit_offset_{M}: cov error {err['cov']:.3g} (bar {pu.bars(pu.case_name(M, 'offset'))['cov']:.3g})")
        assert 0 < err["cov"] < 1e-8
    # the dropped correction term where the comparison is exact
    for M in pu.INT_ROWS[1:]:
        x = pu.int_case(M, "ends")
        n, s1, s2 = pu.int_moments(x, pu.int_centre())
        cov = pu.finish_exact(n, s1, s2, pu.int_centre(), 1)[1]
        dropped = (s2.astype(np.float64) / np.float64(n - 1)).astype(np.float32)
        assert (cov != dropped).mean() > 0.9, M
    # the projection and the whitening
    for r in pu.PROJECT_R:
        mean, comp = pu.project_tables(r)
        x = pu.project_rows(65)
        out, ss = pu.project64(x, mean, comp)
        mo, ms = pu.project64(x, mean, comp, mutant="mean_not_subtracted")
        bar = pu.bars(f"project_r{r}")
        assert pu.relmax(mo, out) > bar["out"] and pu.relmax(ms, ss) > bar["sumsq"], r
    f = pu.fit64(pu.real_case(3000, "offset"))
    x = pu.real_case(3000, "offset")[:200]
    d2, mutated = pu.mahalanobis64(x, f), pu.mahalanobis64(x, f, mutant="whiten_by_lambda")
    assert pu.relmax(mutated, d2) > 1.0 > pu.bars("transform_offset_3000")["mahalanobis"]
    ok = np.isfinite(pu.real_case(3000, "offset")).all(axis=1)
    total = pu.mahalanobis64(pu.real_case(3000, "offset")[ok], f, mutant="whiten_by_lambda").sum()
    want = (f["count"] - 1) * f["rank"]
    assert abs(total - want) / want > 1.0 > max(pu.bars(f"trace_scene_stride{stride}")["trace"] for stride in (8, 5))
    assert set(pu.MUTANTS) == {"one_pass_fp32", "ddof0", "nan_counted", "no_correction", "mean_not_subtracted", "whiten_by_lambda", "ascending"}
