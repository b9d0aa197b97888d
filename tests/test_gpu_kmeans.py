"""GPU: k-means on frozen features -- msst_kmeans_assign / msst_kmeans_update / msst_kmeans_pick (maskedsst_amd/csrc/msst_kmeans.hip)
against the float64 restatement of tests/kmeans_util.py: exact on integer data (no tolerance: the tie rule, an empty cluster, a NaN
row, both layouts, the k-means++ picks), one teacher-forced iteration on real-valued data, whole trajectories, equal bits from equal
inputs, the seeding distribution, the route through the model and the two scripts.  The bars are 4 x the errors measured on the
MI355X (profiles/kmeans_parity_measured.jsonl); tests/test_kmeans_host.py checks on the CPU that they still tell the
mutated references apart.  Every device output is prefilled with NaN or a sentinel."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT
import kmeans_util as ku

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


class Work:
    """the buffers of a fit driven iteration by iteration (maskedsst_amd.cluster.lloyd_iteration), every output prefilled"""

    def __init__(self, x, cent, metric):
        from maskedsst_amd import _lib, cluster
        self.x, self.metric = x.cuda().contiguous(), metric
        self.cent = cent.clone().cuda().contiguous()
        self.bias = cluster._bias(self.cent, metric)
        M, k = x.shape[0], cent.shape[0]
        self.assign = torch.full((M,), -1, dtype=torch.int32, device="cuda")
        self.dist = torch.full((M,), 12345.0, device="cuda")
        self.slab = torch.full((int(_lib.load().msst_kmeans_scratch_floats(M, k)),), float("nan"), device="cuda")
        self.k = k

    def step(self):
        """-> dict(labels, dist, centroids, bias, counts, history [4]) on the CPU, after one iteration"""
        from maskedsst_amd import cluster
        rec = torch.full((1, cluster.record_width(self.k)), float("nan"), device="cuda")
        cluster.lloyd_iteration(self.x, self.cent, self.bias, self.metric, self.assign, self.dist, self.slab, rec[0])
        hist, counts = cluster.read_records(rec.cpu(), self.k)
        return dict(labels=self.assign.cpu().long(), dist=self.dist.cpu(), centroids=self.cent.cpu().clone(), bias=self.bias.cpu().clone(),
                    counts=counts[0], history=hist[0])


# --------------------------------------------------------------------------------------------- 1. exact on integer data, no tolerance
def map_of(x):
    """rows [M, 96] as a map [Bs, 96, plane] with M = Bs plane, plane no multiple of the 64-row tile where M allows"""
    M = x.shape[0]
    Bs = next(b for b in (5, 3, 2, 1) if M % b == 0)
    return x.view(Bs, M // Bs, 96).permute(0, 2, 1).contiguous(), M // Bs


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("M,k", ku.INT_SHAPES)
def test_exact_on_integer_data(M, k, metric):
    from maskedsst_amd import KMeans
    from maskedsst_amd.cluster import kmeans_assign
    x, cent = ku.int_case(M, k)
    ref = ku.step64(x, cent, metric)
    got = Work(x, cent, metric).step()
    assert torch.equal(got["labels"], ref["labels"])
    assert torch.equal(got["counts"], ref["counts"])
    assert int(got["history"][1]) == ref["moved"] == int((~ref["bad"]).sum()) and int(got["history"][2]) == ref["empty"]
    bad = ref["bad"]
    assert torch.isnan(got["dist"][bad]).all() and (got["labels"][bad] == -1).all() and bool(bad.any()) == (M >= 8)
    if k >= 2:
        assert ref["empty"] >= 1 and ref["counts"][k - 1] == 0          # the later copy of a duplicated centroid never wins a tie
    filled = ref["counts"] > 0
    assert same_bits(got["centroids"][~filled], cent[~filled])            # an empty cluster keeps its centroid
    if metric == "euclidean":
        assert ref["inertia"] < 2 ** 24 and float(got["history"][0]) == ref["inertia"]
        assert torch.equal(got["dist"][~bad].double(), ref["dist"][~bad])
        want = ref["sums"].float() / ref["counts"].float().unsqueeze(1)   # exact integer sums, one IEEE division
        assert same_bits(got["centroids"][filled], want[filled])
        assert ku.relmax(got["bias"], -0.5 * (got["centroids"].double() ** 2).sum(dim=1)) < 1e-6
    else:
        err = ku.relmax(got["centroids"][filled], ref["centroids"][filled])
        print(f"kmeans integer cosine ({M}, {k}): direction error {err:.3e}")
        ku.note("integer_cosine", dict(centroids=err))
        assert err <= ku.bars("integer_cosine")["centroids"]
        assert not got["bias"].any()
    # the assignment alone, rows and the map read in place: the same bits
    km = KMeans(cent.cuda(), metric)
    labels, dist = km.assign(x.cuda())
    assert torch.equal(labels.cpu(), ref["labels"]) and same_bits(dist.cpu(), got["dist"])
    fmap, plane = map_of(x.cuda())
    classes = torch.full((M,), -77, dtype=torch.int64, device="cuda")
    dmap = torch.full((M,), 12345.0, device="cuda")
    a32 = kmeans_assign(km, fmap, 1, M, plane, classes, dmap)
    assert torch.equal(classes, labels) and same_bits(dmap, dist) and torch.equal(a32.long(), labels)


@pytest.mark.parametrize("M,k", [(321, 8), (127, 17), (65, 3)])
def test_kmeanspp_picks_on_integer_data(M, k):
    from maskedsst_amd import fit_kmeans
    x, _ = ku.int_case(M, 16)
    x = x[~torch.isnan(x).any(dim=1)].contiguous()
    xd = x.cuda()
    for seed in (0, 1, 2, 3, 4, 12345, 2 ** 32 - 1):
        rows, cent, largest = ku.seed64(x, k, "euclidean", seed)
        assert largest < 2 ** 24                                          # every prefix sum is exact in fp32
        km = fit_kmeans(xd, k=k, iters=1, metric="euclidean", init="kmeans++", seed=seed)
        assert km.seed_rows.tolist() == rows, seed
        assert len(set(rows)) == k


# -------------------------------------------------------------------------------------- 2. against float64 on real-valued data
def parity_figures(metric, k):
    x, cent = ku.blob_case(metric, k)
    ref = ku.step64(x, cent, metric)
    got = Work(x, cent, metric).step()
    err = ku.step_errors(got["dist"], got["history"][0], got["centroids"], got["history"][3], ref)
    return err, got, ref


@pytest.mark.parametrize("metric,k", ku.PARITY_CASES)
def test_one_iteration_against_float64(metric, k):
    case = ku.case_name(metric, k)
    err, got, ref = parity_figures(metric, k)
    print(f"kmeans parity {case}: {err}")
    ku.note(case, err)
    bar = ku.bars(case)
    bad = ku.within(err, bar)
    assert not bad, bad
    decided = ref["margin"] >= bar["score"]                               # the gap: 4 x the largest measured score error
    assert float((~decided).double().mean()) <= ku.EXCLUDED_SHARE
    assert torch.equal(got["labels"][decided], ref["labels"][decided])
    if bool(decided.all()):
        assert torch.equal(got["counts"], ref["counts"]) and int(got["history"][1]) == ref["moved"]


# ------------------------------------------------------------------------------------------------------------- 3. trajectories
@pytest.mark.parametrize("metric,k,M", ku.TRAJ_CASES)
def test_trajectory_against_float64(metric, k, M):
    from maskedsst_amd import fit_kmeans
    case = f"traj_{ku.case_name(metric, k)}"
    x, init = ku.traj_case(metric, k, M)
    ref = ku.fit64(x, init, metric, ku.TRAJ_ITERS)
    assert ref["history"][-1, 1] == 0 and int((ref["history"][:, 1] > 0).sum()) >= 3
    from maskedsst_amd import cluster
    w = Work(x, cluster._unit_rows(init.cuda()).cpu() if metric == "cosine" else init, metric)      # the bits fit_kmeans starts from
    steps = []
    for t in range(ku.TRAJ_ITERS):
        s = w.step()
        assert torch.equal(s["labels"], ref["labels"][t]), t
        assert torch.equal(s["counts"], ref["counts"][t]), t
        assert int(s["history"][1]) == int(ref["history"][t, 1]) and int(s["history"][2]) == int(ref["history"][t, 2]), t
        steps.append(s)
    # the iteration after moved == 0 leaves every output bit unchanged
    first = next(t for t in range(ku.TRAJ_ITERS) if int(steps[t]["history"][1]) == 0)
    assert first + 1 < ku.TRAJ_ITERS
    for t in range(first + 1, ku.TRAJ_ITERS):
        a, b = steps[first], steps[t]
        assert all(same_bits(a[n], b[n]) for n in ("dist", "centroids", "bias", "history")) and torch.equal(a["labels"], b["labels"]) \
            and torch.equal(a["counts"], b["counts"]), t
    assert float(steps[first]["history"][3]) == 0.0
    last = steps[-1]
    dref = ku.assign64(x, ku.fit64(x, init, metric, ku.TRAJ_ITERS - 1)["centroids"], metric)["dist"]
    err = dict(centroids=ku.relmax(last["centroids"], ref["centroids"]), inertia=ku.relmax(last["history"][0], ref["history"][-1, 0]),
               score=float((last["dist"].double() - dref).abs().max() / 2.0))
    print(f"kmeans trajectory {case}: {err}")
    ku.note(case, err)
    bad = ku.within(err, ku.bars(case))
    assert not bad, bad
    # the public fit from the same init: the bits of the loop above
    km = fit_kmeans(x.cuda(), k=k, iters=ku.TRAJ_ITERS, metric=metric, init=init.cuda())
    assert same_bits(km.centroids.cpu(), last["centroids"]) and same_bits(km.bias.cpu(), last["bias"])
    assert torch.equal(km.counts.cpu(), last["counts"]) and torch.equal(km.counts_history, ref["counts"]) and km.seed_rows is None
    assert same_bits(km.history, torch.stack([s["history"] for s in steps]))
    assert km.history.shape == (ku.TRAJ_ITERS, 4) and km.history[:, 1].tolist() == ref["history"][:, 1].tolist()


# --------------------------------------------------------------------------------------------------------------- 4. guarantees
def km_bits_equal(a, b):
    return same_bits(a.centroids, b.centroids) and same_bits(a.bias, b.bias) and torch.equal(a.counts, b.counts) \
        and same_bits(a.history, b.history) and torch.equal(a.counts_history, b.counts_history) and \
        ((a.seed_rows is None and b.seed_rows is None) or torch.equal(a.seed_rows, b.seed_rows))


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
@pytest.mark.parametrize("init", ["kmeans++", "sample", "tensor"])
def test_two_fits_give_the_same_bits(init, metric):
    from maskedsst_amd import fit_kmeans
    x, cent = ku.blob_case(metric, 16, M=2500, seed=3)
    xd = x.cuda()
    kw = dict(k=16, iters=12, metric=metric, init=cent.cuda() if init == "tensor" else init, seed=7)
    a, b = fit_kmeans(xd, **kw), fit_kmeans(xd, **kw)
    assert km_bits_equal(a, b) and not torch.isnan(a.centroids).any() and not torch.isnan(a.history).any()
    assert a.history.shape == (12, 4) and int(a.counts.sum()) == 2500 and a.history[0, 1] == 2500
    if init != "tensor":
        assert len(set(a.seed_rows.tolist())) == 16 and a.seed_rows.dtype == torch.int64
    if init == "sample":
        assert a.seed_rows.tolist() == torch.randperm(2500, generator=torch.Generator().manual_seed(7))[:16].tolist()
    if metric == "cosine":
        assert float((a.centroids.double().norm(dim=1) - 1).abs().max()) < 1e-6
    # check_every: stops at the fixed point, the bits of the full run
    long_kw = dict(kw, iters=40)
    full, early = fit_kmeans(xd, **long_kw), fit_kmeans(xd, check_every=1, **long_kw)
    assert km_bits_equal(full, early)
    assert km_bits_equal(full, fit_kmeans(xd, check_every=7, **long_kw))


def test_assign_does_not_depend_on_the_batch():
    from maskedsst_amd import KMeans
    from maskedsst_amd.cluster import kmeans_assign
    x, cent = ku.blob_case("euclidean", 16, M=1000, seed=5)
    x[17, 3] = float("nan")
    xd = x.cuda()
    km = KMeans(cent.cuda(), "euclidean")
    labels, dist = km.assign(xd)
    for lo, hi in ((0, 1), (0, 65), (13, 700), (17, 18), (936, 1000)):
        l2, d2 = km.assign(xd[lo:hi].contiguous())
        assert torch.equal(l2, labels[lo:hi]) and same_bits(d2, dist[lo:hi]), (lo, hi)
    assert int(labels[17]) == -1 and bool(torch.isnan(dist[17])) and int((labels < 0).sum()) == 1
    fmap = xd.view(4, 250, 96).permute(0, 2, 1).contiguous()
    classes = torch.full((1000,), -77, dtype=torch.int64, device="cuda")
    dmap = torch.full((1000,), 12345.0, device="cuda")
    kmeans_assign(km, fmap, 1, 1000, 250, classes, dmap)
    assert torch.equal(classes, labels) and same_bits(dmap, dist)


def test_n_init_keeps_the_lowest_inertia():
    from maskedsst_amd import fit_kmeans
    x, _ = ku.blob_case("euclidean", 16, M=1500, seed=9)
    xd = x.cuda()
    kw = dict(k=8, iters=6, metric="euclidean", init="kmeans++")
    singles = [fit_kmeans(xd, seed=s, **kw) for s in (20, 21, 22)]
    inertias = [s.inertia for s in singles]
    assert len(set(inertias)) > 1, inertias
    best = fit_kmeans(xd, seed=20, n_init=3, **kw)
    assert km_bits_equal(best, singles[inertias.index(min(inertias))]) and best.seed == 20 + inertias.index(min(inertias))


def test_knn_bank_is_accepted():
    from maskedsst_amd import KnnBank, fit_kmeans
    x, _ = ku.blob_case("cosine", 3, M=300)
    bank = KnnBank(x.cuda(), torch.zeros(300, dtype=torch.int64).cuda(), 2)
    a, b = fit_kmeans(bank, k=3, iters=4), fit_kmeans(x.cuda(), k=3, iters=4)
    assert km_bits_equal(a, b)
    bad = x.clone()
    bad[5, 5] = float("inf")
    with pytest.raises(ValueError, match="finite"):
        fit_kmeans(bad.cuda(), k=3, iters=4)


# ------------------------------------------------------------------------------------------------------ 5. seeding distribution
def test_seeding_follows_the_d2_distribution():
    """three tight groups: over 256 seeds, the second centre given that the first fell in group A lands in B with the D^2 probability"""
    from maskedsst_amd import fit_kmeans
    x, group = ku.group_case()
    xd, x64 = x.cuda(), x.double()
    hits, expect, var, n = 0, 0.0, 0.0, 0
    for seed in range(256):
        rows = fit_kmeans(xd, k=3, iters=1, metric="euclidean", init="kmeans++", seed=seed).seed_rows.tolist()
        assert len(set(rows)) == 3 and rows[0] == ku.pick64(x, None, [], seed, 0)
        if int(group[rows[0]]) != 0:
            continue
        d2 = ((x64 - x64[rows[0]]) ** 2).sum(dim=1)
        p = float(d2[group == 1].sum() / d2.sum())
        n, expect, var = n + 1, expect + p, var + p * (1 - p)
        hits += int(group[rows[1]]) == 1
    print(f"kmeans seeding: {n} first centres in A, second in B {hits} times, expected {expect:.1f} +- {math.sqrt(var):.1f}")
    assert n >= 100 and abs(hits - expect) <= 5.0 * math.sqrt(var), (n, hits, expect, var)


# ----------------------------------------------------------------------------------------------------------- 6. through the model
def make_model(nc=5):
    from maskedsst_amd import ViTSpatialSpectral
    torch.manual_seed(5)
    return ViTSpatialSpectral(image_size=8, spatial_patch_size=1, spectral_patch_size=10, num_classes=nc, dim=96, depth=2, heads=8,
                              mlp_dim=64, channels=50, spectral_pos=torch.arange(5), blockwise_patch_embed=True, precision="fp32").cuda()


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
@pytest.mark.parametrize("stride", [8, 5])
def test_cluster_scene_through_the_model(stride, metric):
    from maskedsst_amd import ClusterScene, cluster_scene, fit_kmeans
    model = make_model()
    model.train()
    g = torch.Generator().manual_seed(3)
    scene = torch.randn(2, 50, 16, 16, generator=g).cuda()
    emb = model.encode_scene(scene, stride=stride, normalize=metric == "cosine")
    covered = emb.cover > 0
    assert bool(covered.all()) == (stride == 8)                              # stride 5: rows and columns 13 .. 15 lie in no window
    rows = emb.features.permute(0, 2, 3, 1).reshape(-1, 96).contiguous()
    km = fit_kmeans(rows[covered.reshape(-1)].contiguous(), k=4, iters=8, metric=metric)
    res = model.cluster_scene(scene, km, stride=stride)
    assert isinstance(res, ClusterScene) and model.training
    assert res.classes.shape == (2, 16, 16) and res.classes.dtype == torch.int64 and res.distance.shape == (2, 16, 16)
    assert torch.equal(res.cover, emb.cover)
    assert (res.classes[~covered] == -1).all() and torch.isnan(res.distance[~covered]).all()
    assert (res.classes[covered] >= 0).all() and not torch.isnan(res.distance[covered]).any()
    labels, dist = km.assign(rows)
    assert torch.equal(labels.view(2, 16, 16), res.classes) and same_bits(dist.view(2, 16, 16), res.distance)
    other = cluster_scene(model, scene, km, stride=stride)
    assert torch.equal(other.classes, res.classes) and same_bits(other.distance, res.distance)


# ------------------------------------------------------------------------------------------------------------------------ 7. scripts
def test_finetune_val_cluster_script():
    """finetune.py --val-cluster: one more line per validation pass"""
    out = child([sys.executable, "finetune.py", "--steps", "2", "--val-scenes", "4", "--val-every", "1", "--val-cluster", "4"], 600)
    cl = [l.split() for l in out.splitlines() if l.startswith("val-cluster step ")]
    assert [e[2] for e in cl] == ["1", "2"], out
    for e in cl:
        assert e[3:5] == ["k", "4"] and e[5] == "cluster_acc" and 0.0 <= float(e[6]) <= 1.0, e
        assert e[7] == "purity" and float(e[6]) <= float(e[8]) + 1e-9 <= 1.0 + 1e-9 and e[9] == "nmi" and 0.0 <= float(e[10]) <= 1.0, e
        assert e[11] == "inertia" and float(e[12]) >= 0 and e[13] == "test_pixels" and int(e[14]) > 0, e


def test_kmeans_time_script():
    """tools/kmeans_time.py --smoke: exit 0 and ONE JSON line, nothing appended"""
    out = child([sys.executable, os.path.join("tools", "kmeans_time.py"), "--smoke"], 300)
    lines = [l for l in out.splitlines() if l.strip()]
    assert len(lines) == 1, out
    row = json.loads(lines[0])
    assert row["tool"] == "kmeans_time" and row["M"] == 8192 and row["k"] == 16
    assert row["iteration_us"] > 0 and row["eager_iteration_us"] > 0 and row["fit_ms"] > 0 and row["eager_fit_ms"] > 0
