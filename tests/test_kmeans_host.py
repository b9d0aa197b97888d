"""k-means, host side (no GPU needed): the C ABI of msst_kmeans_scratch_floats / msst_kmeans_assign / msst_kmeans_update /
msst_kmeans_pick (additive under MSST_VERSION 109) and their argument checks (they run before any HIP call, so null pointers, host
buffers and no device are enough to see them), the ValueError / RuntimeError surface of maskedsst_amd/cluster.py, match_clusters
against brute force and scipy, the flag of finetune.py, and the float64 restatement of tests/kmeans_util.py: it tells itself apart
from its mutations at the committed bars, and the committed gaps leave out at most 1 % of a case's rows."""
import ctypes
import itertools
import math
import re
import subprocess

import numpy as np
import pytest
import torch

import kmeans_util as ku

BADARG, UNSUPPORTED = -3, -2   # include/msst.h: MSST_ERR_BADARG, MSST_ERR_UNSUPPORTED


# --------------------------------------------------------------------------------------------------------------------- C ABI
def test_c_abi_declares_and_exports_the_entry_points():
    from ctypes import c_int, c_long, c_uint32, c_void_p
    from maskedsst_amd import _lib
    header = open(_lib.HEADER_PATH).read()
    assert _lib.header_version() == 109   # additive: the revision does not move
    lib = _lib.load()
    assert lib.msst_version() == 109
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    P = c_void_p
    sigs = {
        # long rows, int k
        "msst_kmeans_scratch_floats": (c_long, [c_long, c_int]),
        # x, int x_layout, long rows, long plane, int dim, centroids, bias, int k, int metric, assign, dist, classes, slab, long slab_floats, stream
        "msst_kmeans_assign": (c_int, [P, c_int, c_long, c_long, c_int, P, P, c_int, c_int, P, P, P, P, c_long, P]),
        # slab, long slab_floats, long rows, int dim, int k, int metric, centroids, bias, counts, shift, history_row, stream
        "msst_kmeans_update": (c_int, [P, c_long, c_long, c_int, c_int, c_int, P, P, P, P, P, P]),
        # x, long rows, int dim, dist, slab, long slab_floats, int j, int k, int metric, uint32 seed, centroids, bias, seed_rows, stream
        "msst_kmeans_pick": (c_int, [P, c_long, c_int, P, P, c_long, c_int, c_int, c_int, c_uint32, P, P, P, P]),
    }
    for name, sig in sigs.items():
        m = re.search(r"^(int|long) %s\(([^;]*)\);" % name, header, re.M)
        assert m, name
        assert len(m.group(2).split(",")) == len(sig[1]), name                # the header's argument count
        assert name in _lib.declared_symbols() and _lib._SIGS[name] == sig, name
        assert re.search(r" T %s$" % name, out, re.M), name
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == sig, name
    from maskedsst_amd import cluster
    for metric, value in cluster.METRICS.items():
        assert re.search(r"^#define\s+MSST_KMEANS_%s\s+%d$" % (metric.upper(), value), header, re.M), metric
    import maskedsst_amd
    for name in ("KMeans", "ClusterScene", "ClusterMatch", "fit_kmeans", "cluster_scene", "contingency", "match_clusters"):
        assert name in maskedsst_amd.__all__ and hasattr(maskedsst_amd, name), name
    assert maskedsst_amd.ClusterScene._fields == ("classes", "distance", "cover")
    assert maskedsst_amd.ClusterMatch._fields == ("mapping", "accuracy", "purity", "nmi")
    assert hasattr(maskedsst_amd.ViTSpatialSpectral, "cluster_scene")
    assert "msst_kmeans.hip" in __import__("maskedsst_amd.build", fromlist=["SOURCES"]).SOURCES


def _ptr():
    buf = (ctypes.c_char * 64)()
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)


def test_scratch_floats():
    from maskedsst_amd import _lib
    f = _lib.load().msst_kmeans_scratch_floats
    per = lambda k: 97 * k + 2   # noqa: E731
    assert f(1, 2) == per(2) and f(64, 16) == per(16) and f(65, 16) == 2 * per(16) and f(512 * 64, 5) == 512 * per(5)
    assert f(512 * 64 + 1, 5) == 257 * per(5)                   # two tiles per workgroup from here on
    assert f(262144, 16) == 512 * per(16) and f(262144, 128) == 512 * per(128)
    for bad in ((0, 5), (-1, 5), (10, 0), (10, 129), (1 << 31, 5)):
        assert f(*bad) == 0, bad


def test_kmeans_assign_refuses_bad_arguments_before_launch():
    from maskedsst_amd import _lib
    lib = _lib.load()
    buf, p = _ptr()
    names = ("x", "centroids", "bias", "assign", "dist", "classes", "slab")

    def call(x_layout=0, rows=128, plane=1, dim=96, k=5, metric=0, slab_floats=None, **ptr):
        a = {n: ptr.get(n, p) for n in names}
        if slab_floats is None:
            slab_floats = lib.msst_kmeans_scratch_floats(rows, k)
        return lib.msst_kmeans_assign(a["x"], x_layout, rows, plane, dim, a["centroids"], a["bias"], k, metric, a["assign"], a["dist"],
                                      a["classes"], a["slab"], slab_floats, None)

    null = {n: None for n in names}
    for bad in (dict(rows=0), dict(rows=-3), dict(k=0), dict(k=-2), dict(dim=0), dict(metric=2), dict(metric=-1)):
        assert call(**bad) == BADARG and call(**bad, **null) == BADARG, bad
    assert b"msst_kmeans_assign" in lib.msst_last_error()
    for over in (dict(dim=95), dict(dim=128), dict(k=129), dict(rows=1 << 31)):
        assert call(slab_floats=1 << 40, **over) == UNSUPPORTED and call(slab_floats=0, **over, **null) == UNSUPPORTED, over
    assert b"msst_kmeans_assign" in lib.msst_last_error()
    for layout in (-1, 2):
        assert call(x_layout=layout) == BADARG, layout
    for plane in (0, -4, 5, 256):          # layout 1: plane must divide rows = 128
        assert call(x_layout=1, plane=plane) == BADARG, plane
    assert call(plane=5, **null) == BADARG and b"null" in lib.msst_last_error()      # plane is not read in layout 0
    assert call(k=128, rows=(1 << 31) - 1, **null) == BADARG and b"null" in lib.msst_last_error()   # the limits themselves are inside
    for n in ("x", "centroids", "bias", "assign", "dist"):
        assert call(**{n: None}) == BADARG, n
    assert call(x=ctypes.c_void_p(p.value + 4)) == BADARG                            # rows are read 16 bytes at a time
    assert call(classes=ctypes.c_void_p(p.value + 4)) == BADARG
    for n in ("centroids", "bias", "assign", "dist", "slab"):
        assert call(**{n: ctypes.c_void_p(p.value + 2)}) == BADARG, n
    need = lib.msst_kmeans_scratch_floats(128, 5)
    assert need > 0 and call(slab_floats=need - 1) == BADARG and b"slab" in lib.msst_last_error()


def test_kmeans_update_refuses_bad_arguments_before_launch():
    from maskedsst_amd import _lib
    lib = _lib.load()
    buf, p = _ptr()
    names = ("slab", "centroids", "bias", "counts", "shift", "history_row")

    def call(rows=100, dim=96, k=5, metric=1, slab_floats=None, **ptr):
        a = {n: ptr.get(n, p) for n in names}
        if slab_floats is None:
            slab_floats = lib.msst_kmeans_scratch_floats(rows, k)
        return lib.msst_kmeans_update(a["slab"], slab_floats, rows, dim, k, metric, a["centroids"], a["bias"], a["counts"], a["shift"],
                                      a["history_row"], None)

    null = {n: None for n in names}
    for bad in (dict(rows=0), dict(rows=-1), dict(k=0), dict(dim=0), dict(metric=7)):
        assert call(**bad) == BADARG and call(**bad, **null) == BADARG, bad
    for over in (dict(dim=95), dict(k=129)):
        assert call(slab_floats=1 << 40, **over) == UNSUPPORTED and call(**over, **null) == UNSUPPORTED, over
    assert b"msst_kmeans_update" in lib.msst_last_error()
    for n in names:
        assert call(**{n: None}) == BADARG, n
        assert call(**{n: ctypes.c_void_p(p.value + 2)}) == BADARG, n
    assert b"null" in lib.msst_last_error()
    assert call(slab_floats=lib.msst_kmeans_scratch_floats(100, 5) - 1) == BADARG and b"slab" in lib.msst_last_error()


def test_kmeans_pick_refuses_bad_arguments_before_launch():
    from maskedsst_amd import _lib
    lib = _lib.load()
    buf, p = _ptr()
    names = ("x", "dist", "slab", "centroids", "bias", "seed_rows")

    def call(rows=100, dim=96, j=2, k=5, metric=1, seed=3, slab_floats=None, **ptr):
        a = {n: ptr.get(n, p) for n in names}
        if slab_floats is None:
            slab_floats = lib.msst_kmeans_scratch_floats(rows, max(j, 1))
        return lib.msst_kmeans_pick(a["x"], rows, dim, a["dist"], a["slab"], slab_floats, j, k, metric, seed, a["centroids"], a["bias"],
                                    a["seed_rows"], None)

    null = {n: None for n in names}
    for bad in (dict(rows=0), dict(k=0), dict(dim=0), dict(metric=2), dict(j=-1), dict(j=5), dict(j=9)):
        assert call(**bad) == BADARG and call(**bad, **null) == BADARG, bad
    assert b"msst_kmeans_pick" in lib.msst_last_error()
    for over in (dict(dim=97), dict(k=129), dict(rows=1 << 31)):
        assert call(slab_floats=1 << 40, **over) == UNSUPPORTED and call(**over, **null) == UNSUPPORTED, over
    for n in ("x", "dist", "slab", "centroids", "bias", "seed_rows"):
        assert call(**{n: None}) == BADARG, n
        assert call(**{n: ctypes.c_void_p(p.value + 2)}) == BADARG, n
    assert b"null" in lib.msst_last_error()
    # centre 0 reads neither dist nor the slab: the next refusal is the null x
    assert call(j=0, dist=None, slab=None, slab_floats=0, x=None) == BADARG and b"null" in lib.msst_last_error()
    assert call(slab_floats=lib.msst_kmeans_scratch_floats(100, 2) - 1) == BADARG and b"slab" in lib.msst_last_error()


# --------------------------------------------------------------------------------------------------------- the Python surface
def make_encoder(**kw):
    from maskedsst_amd import ViTSpatialSpectral
    torch.manual_seed(5)
    args = dict(image_size=8, spatial_patch_size=1, spectral_patch_size=10, num_classes=4, dim=96, depth=1, heads=8, mlp_dim=64,
                channels=50, spectral_pos=torch.arange(5), blockwise_patch_embed=True)
    args.update(kw)
    return ViTSpatialSpectral(**args)


def test_fit_refuses_bad_arguments_before_device_work():
    from maskedsst_amd import KMeans, KnnBank, fit_kmeans
    x = torch.randn(40, 96)
    zero_row = torch.randn(4, 96)
    zero_row[2] = 0.0
    for kw in (dict(features=None), dict(features=torch.zeros(40, 95)), dict(features=torch.zeros(96)), dict(features=torch.zeros(40, 96).double()),
               dict(features=torch.zeros(96, 40).t()), dict(features=[[0.0] * 96]), dict(features=torch.zeros(0, 96)),
               dict(k=0), dict(k=129), dict(k=4.0), dict(k=True), dict(k=41), dict(iters=0), dict(iters=-1), dict(iters=2.5),
               dict(metric="l2"), dict(metric=None), dict(metric=0), dict(init="random"), dict(init=None), dict(init=torch.zeros(3, 96) + 1),
               dict(init=torch.ones(4, 95)), dict(init=torch.ones(4, 96).double()), dict(init=zero_row), dict(init=torch.full((4, 96), float("nan"))),
               dict(seed=-1), dict(seed=1.5), dict(seed=2 ** 32), dict(n_init=0), dict(n_init=1.0), dict(check_every=0), dict(check_every=2.0)):
        args = dict(features=x, k=4, iters=3)
        args.update(kw)
        with pytest.raises(ValueError):
            fit_kmeans(**args)
    fit_zero = dict(features=x, k=4, iters=3, metric="euclidean", init=zero_row)      # a zero row is a fine euclidean centre
    bank = KnnBank.__new__(KnnBank)
    bank.features, bank.labels, bank.n_classes = x, torch.zeros(40, dtype=torch.int32), 2
    for args in (dict(features=x, k=4, iters=3), dict(features=x, k=40, iters=1, init="sample"), fit_zero, dict(features=bank, k=4, iters=2),
                 dict(features=x, k=4, iters=3, init=torch.ones(4, 96), n_init=2, check_every=1)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):           # everything is in order but the device
            fit_kmeans(**args)
    for cent, metric in ((torch.zeros(4, 95), "cosine"), (torch.zeros(96), "cosine"), (torch.zeros(0, 96), "cosine"), (torch.zeros(129, 96), "cosine"),
                         (torch.zeros(4, 96).double(), "cosine"), (torch.zeros(96, 4).t(), "cosine"), (torch.zeros(4, 96), "manhattan")):
        with pytest.raises(ValueError):
            KMeans(cent, metric)
    km = KMeans(torch.ones(4, 96), "euclidean")
    assert km.k == 4 and km.bias.tolist() == [-48.0] * 4 and km.history is None and math.isnan(km.inertia) and km.counts is None
    assert not KMeans(torch.ones(4, 96), "cosine").bias.any()
    for f in (torch.zeros(5, 95), torch.zeros(96), torch.zeros(0, 96), torch.zeros(5, 96).double(), torch.zeros(96, 5).t(), [[0.0] * 96]):
        with pytest.raises(ValueError):
            km.assign(f)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        km.assign(torch.zeros(5, 96))


def test_cluster_scene_and_contingency_refuse_bad_arguments():
    from maskedsst_amd import KMeans, cluster_scene, contingency
    enc = make_encoder()
    km = KMeans(torch.ones(4, 96), "cosine")
    scene = torch.zeros(2, 50, 16, 16)
    for kw in (dict(km=None), dict(km=torch.ones(4, 96)), dict(scene=torch.zeros(2, 40, 16, 16)), dict(scene=torch.zeros(50, 16, 16)),
               dict(scene=torch.zeros(2, 50, 4, 16)), dict(stride=9), dict(stride=0), dict(max_windows=0)):
        args = dict(scene=scene, km=km)
        args.update(kw)
        with pytest.raises(ValueError):
            enc.cluster_scene(**args)
        with pytest.raises(ValueError):
            cluster_scene(enc, **args)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc.cluster_scene(scene, km)
    assert enc.training   # nothing above touched the module's mode
    lab, tru = torch.tensor([0, 1, 1, -1, 2, 2, 1]), torch.tensor([1, 1, 0, 0, -1, 5, 1])
    assert contingency(lab, tru, 3, 2).tolist() == [[0, 1], [1, 2], [0, 0]]        # -1 cluster, ignored truth, truth out of range: left out
    assert contingency(lab, tru, 3, 2, ignored_label=0).tolist() == [[0, 1], [0, 2], [0, 0]]
    assert contingency(lab.view(7, 1), tru.view(7, 1).int(), 3, 6).sum() == 5 and contingency(lab, tru, 3, 2).dtype == torch.int64
    for kw in (dict(labels=lab[:3]), dict(labels=lab.float()), dict(truth=tru.double()), dict(k=0), dict(n_classes=0), dict(k=2.0), dict(labels=[0, 1])):
        args = dict(labels=lab, truth=tru, k=3, n_classes=2)
        args.update(kw)
        with pytest.raises(ValueError):
            contingency(**args)


def test_finetune_parser_takes_val_cluster():
    import finetune
    ap = finetune.build_parser()
    assert ap.parse_args(["enmap"]).val_cluster == 0
    a = ap.parse_args(["enmap", "--val-scenes", "4", "--val-every", "1", "--val-cluster", "4"])
    assert a.val_cluster == 4
    with pytest.raises(SystemExit):
        finetune.check_val_cluster(ap.parse_args(["enmap", "--val-cluster", "4"]))                     # needs --val-scenes and --val-every
    with pytest.raises(SystemExit):
        finetune.check_val_cluster(ap.parse_args(["enmap", "--val-scenes", "4", "--val-cluster", "4"]))
    for k in ("-3", "129"):
        with pytest.raises(SystemExit):
            finetune.check_val_cluster(ap.parse_args(["enmap", "--val-scenes", "4", "--val-every", "1", "--val-cluster", k]))
    finetune.check_val_cluster(a)
    finetune.check_val_cluster(ap.parse_args(["enmap"]))


# ------------------------------------------------------------------------------------------------------------- match_clusters
def brute_force(table):
    """the largest matched count over all one-to-one assignments of the zero-padded square table"""
    k, nc = table.shape
    n = max(k, nc)
    sq = np.zeros((n, n), dtype=np.int64)
    sq[:k, :nc] = table
    return max(sum(sq[i, perm[i]] for i in range(n)) for perm in itertools.permutations(range(n)))


def test_match_clusters_against_brute_force():
    from maskedsst_amd import match_clusters
    g = np.random.default_rng(11)
    shapes = [(1, 1), (2, 2), (3, 3), (4, 4), (5, 5), (6, 6), (2, 5), (5, 2), (6, 3), (3, 6), (1, 4), (4, 1)]
    for k, nc in shapes:
        for rep in range(12):
            table = g.integers(0, 40, size=(k, nc)) * (g.random((k, nc)) < (0.4 + 0.1 * (rep % 6)))
            m = match_clusters(torch.from_numpy(table))
            total = int(table.sum())
            if total == 0:
                assert math.isnan(m.accuracy)
                continue
            mapping = m.mapping.tolist()
            used = [c for c in mapping if c >= 0]
            assert len(mapping) == k and len(set(used)) == len(used) == min(k, nc) and all(0 <= c < nc for c in used)
            matched = sum(int(table[c, mapping[c]]) for c in range(k) if mapping[c] >= 0)
            assert matched == brute_force(table), (k, nc, rep)
            assert m.accuracy == matched / total and m.purity == table.max(axis=1).sum() / total
            assert m.accuracy <= m.purity + 1e-15 and 0.0 <= m.nmi <= 1.0 + 1e-12
    for bad in (torch.zeros(3), torch.zeros(2, 2, 2), -torch.ones(2, 2), torch.full((2, 2), float("nan")), torch.zeros(0, 3)):
        with pytest.raises(ValueError):
            match_clusters(bad)
    assert match_clusters([[3, 0], [0, 2]]).accuracy == 1.0 and match_clusters(np.array([[0, 4], [5, 0]])).mapping.tolist() == [1, 0]


def test_match_clusters_against_scipy():
    opt = pytest.importorskip("scipy.optimize")
    from maskedsst_amd import match_clusters
    g = np.random.default_rng(12)
    for k, nc in ((16, 16), (128, 20), (20, 128), (37, 41), (128, 128)):
        table = g.integers(0, 1000, size=(k, nc)) * (g.random((k, nc)) < 0.3)
        r, c = opt.linear_sum_assignment(table, maximize=True)
        m = match_clusters(table)
        mapping = m.mapping.numpy()
        assert sum(table[i, mapping[i]] for i in range(k) if mapping[i] >= 0) == table[r, c].sum(), (k, nc)


def test_nmi_of_identical_and_independent_labelings():
    from maskedsst_amd import contingency, match_clusters
    g = torch.Generator().manual_seed(13)
    a = torch.randint(0, 6, (5000,), generator=g)
    same = match_clusters(contingency(a, a, 6, 6))
    assert abs(same.nmi - 1.0) < 1e-12 and same.accuracy == 1.0 and same.purity == 1.0 and same.mapping.tolist() == list(range(6))
    perm = torch.tensor([3, 0, 5, 1, 2, 4])
    moved = match_clusters(contingency(perm[a], a, 6, 6))                 # a relabeling: still perfect, the mapping undoes it
    assert abs(moved.nmi - 1.0) < 1e-12 and moved.accuracy == 1.0 and moved.mapping[perm].tolist() == list(range(6))
    independent = match_clusters(torch.outer(torch.tensor([10, 20, 30]), torch.tensor([1, 2, 3, 4])))   # p(c, y) = p(c) p(y) exactly
    assert abs(independent.nmi) < 1e-12
    # sklearn's definition (arithmetic mean of the entropies) on a hand-computed table: I = ln 2 - 0.5 (h(1/4)) ...
    t = np.array([[3, 1], [1, 3]], dtype=float)
    p = t / t.sum()
    mi = sum(p[i, j] * math.log(p[i, j] / (p[i].sum() * p[:, j].sum())) for i in range(2) for j in range(2))
    assert abs(match_clusters(t).nmi - mi / math.log(2)) < 1e-12
    assert match_clusters([[5, 3, 2]]).nmi == 0.0 and match_clusters([[5]]).nmi == 1.0       # one cluster against three classes; both trivial


# ------------------------------------------------------------------------------------------------- the float64 restatement itself
def test_hash_restatements_agree():
    seeds = [0, 1, 7, 12345, 2 ** 31, 2 ** 32 - 1]
    js = [0, 1, 2, 63, 127]
    for s in seeds:
        got = ku.km_hash_np(np.full(len(js), s), np.array(js))
        assert [int(v) for v in got] == [ku.km_hash(s, j) for j in js]
    u = np.array([ku.draw_u(s, j) for s in range(4096) for j in (0, 1)])
    assert 0.0 <= u.min() and u.max() < 1.0 and abs(u.mean() - 0.5) < 0.02 and abs((u < 0.25).mean() - 0.25) < 0.03
    assert ku.pick64(torch.zeros(300, 96), None, [], 5, 0) == int(ku.draw_u(5, 0) * 300)     # centre 0: floor(u M)


def test_restatement_rules():
    x, cent = ku.int_case(321, 17)
    r = ku.step64(x, cent, "euclidean")
    assert bool(r["bad"].any()) and (r["labels"][r["bad"]] == -1).all() and torch.isnan(r["dist"][r["bad"]]).all()
    assert int(r["counts"].sum()) == int((~r["bad"]).sum()) and r["moved"] == int((~r["bad"]).sum())
    assert r["counts"][16] == 0 and r["counts"][7] == 0 and torch.equal(r["centroids"][16], cent[16].double())    # ties, kept centroids
    brute = ((x.double().unsqueeze(1) - cent.double().unsqueeze(0)) ** 2).sum(dim=2)
    ok = ~r["bad"]
    assert torch.equal(r["dist"][ok], brute[ok].min(dim=1).values) and torch.equal(r["labels"][ok], brute[ok].argmin(dim=1))
    again = ku.step64(x, r["centroids"], "euclidean", prev=r["labels"])
    assert again["moved"] == int((again["labels"] != r["labels"]).sum())
    xc, cc = ku.blob_case("cosine", 16)
    rc = ku.step64(xc, cc, "cosine")
    assert float((rc["centroids"].norm(dim=1) - 1).abs().max()) < 1e-12
    assert ku.relmax(rc["dist"], ((xc.double().unsqueeze(1) - cc.double().unsqueeze(0)) ** 2).sum(dim=2).min(dim=1).values) < 1e-6   # unit vectors
    for metric, k, M in ku.TRAJ_CASES:
        xt, init = ku.traj_case(metric, k, M)
        f = ku.fit64(xt, init, metric, ku.TRAJ_ITERS)
        assert f["history"][-1, 1] == 0 and int((f["history"][:, 1] > 0).sum()) >= 3 and f["history"][-1, 3] == 0
        assert f["min_margin"] > 1e-3 and f["min_margin"] >= 100 * ku.gap(f"traj_{ku.case_name(metric, k)}")    # far above the gap, every iteration


def test_committed_bars_tell_the_mutants_apart():
    """every bar is 4 x a committed measurement, and every mutated reference lies beyond a bar (or, where the comparison is exact,
    differs) on the committed cases"""
    for metric, k in ku.PARITY_CASES:
        bar = ku.bars(ku.case_name(metric, k))
        assert set(bar) == {"dist", "inertia", "centroids", "shift", "score"}
        # fp32 kernels: no relative bar is looser than 1e-5; the gap (an ABSOLUTE score error; euclidean scores reach 1e2) stays below 1e-3
        assert all(0 <= v < 1e-5 for q, v in bar.items() if q != "score") and 0 < bar["score"] < 1e-3, (metric, k, bar)
    assert 0 <= ku.bars("integer_cosine")["centroids"] < 1e-5

    def distance(x, cent, metric, mutant):
        ref, mut = ku.step64(x, cent, metric), ku.step64(x, cent, metric, mutant=mutant)
        return ku.step_errors(mut["dist"], mut["inertia"], mut["centroids"], mut["shift"], ref), ref, mut

    for metric, k in ku.PARITY_CASES:
        case = ku.case_name(metric, k)
        bar = ku.bars(case)
        x, cent = ku.blob_case(metric, k)
        mutants = ["sum_not_divided"] + (["mean_without_normalisation"] if metric == "cosine" else ["no_bias"])
        for mutant in mutants:
            d, ref, mut = distance(x, cent, metric, mutant)
            decided = ref["margin"] >= bar["score"]
            assert any(d[q] > bar[q] for q in d) or not torch.equal(ref["labels"][decided], mut["labels"][decided]), (case, mutant, d)
    # the exact comparisons: ties, the empty cluster, the k-means++ pick
    for M, k in ((321, 17), (64, 2), (65, 128)):
        x, cent = ku.int_case(M, k)
        for metric in ("euclidean", "cosine"):
            ref = ku.step64(x, cent, metric)
            assert not torch.equal(ref["labels"], ku.step64(x, cent, metric, mutant="ties_to_highest")["labels"]), (M, k, metric)
            zeroed = ku.step64(x, cent, metric, mutant="empty_zeroed")
            assert ref["empty"] >= 1 and not torch.equal(ref["centroids"], zeroed["centroids"])
    x, _ = ku.int_case(321, 16)
    x = x[~torch.isnan(x).any(dim=1)]
    assert any(ku.seed64(x, 8, "euclidean", s)[0] != ku.seed64(x, 8, "euclidean", s, mutant="prefix_off_by_one")[0] for s in (0, 1, 2))
    assert set(ku.MUTANTS) == {"ties_to_highest", "no_bias", "mean_without_normalisation", "empty_zeroed", "sum_not_divided", "prefix_off_by_one"}


def test_excluded_share():
    """the rows the assignment comparison leaves out (float64 margin below the committed gap): at most 1 % of every committed case"""
    for metric, k in ku.PARITY_CASES:
        x, cent = ku.blob_case(metric, k)
        margin = ku.assign64(x, cent, metric)["margin"]
        share = float((margin < ku.gap(ku.case_name(metric, k))).double().mean())
        assert share <= ku.EXCLUDED_SHARE, (metric, k, share)
