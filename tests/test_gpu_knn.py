"""GPU: kNN evaluation of frozen features -- msst_knn_topk / msst_knn_vote (maskedsst_amd/csrc/msst_knn.hip) against the float64
restatement of tests/knn_util.py: an exact fixture full of ties (index, similarity bits, counts), random unit features (error
bounds, order, the neighbour set, votes, classes), independence of the bank split, of repetition and of the batch, the map layout
and absent pixels, knn_predict_scene / feature_bank through the model, tools/knn_time.py and finetune.py --val-knn.  Every output
is prefilled with NaN or a sentinel: nothing needs initialising."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from util import record
import knn_util
from knn_util import SHAPES

pytestmark = pytest.mark.gpu


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()   # (a copy: the fixtures are read-only and shared)


def make_bank(bank, labels, n_classes):
    from maskedsst_amd import KnnBank
    return KnnBank(dev(bank), dev(labels), n_classes)


def run(bank, queries, k, temperature, splits=None, q_layout=0, plane=1, vote_layout=0):
    """the two launches on prefilled outputs.  queries: a device tensor, rows [Q, 96] or a map [Bs, 96, plane]"""
    from maskedsst_amd.knn import knn_launch, KnnResult
    Q = queries.shape[0] if q_layout == 0 else queries.shape[0] * plane
    nc = bank.n_classes
    index = torch.full((Q, k), 123456789, dtype=torch.int32, device="cuda")
    sim = torch.full((Q, k), float("nan"), device="cuda")
    votes = torch.full((Q, nc) if vote_layout == 0 else (Q // plane, nc, plane), float("nan"), device="cuda")
    classes = torch.full((Q,), -77, dtype=torch.int64, device="cuda")
    knn_launch(bank, queries, q_layout, Q, plane, k, temperature, splits, votes, vote_layout, classes, index=index, sim=sim)
    torch.cuda.synchronize()
    return KnnResult(classes, votes, index, sim)


def to_np(r):
    return r.classes.cpu().numpy(), r.votes.cpu().numpy(), r.index.cpu().numpy(), r.sim.cpu().numpy()


# ------------------------------------------------------------------------------------------------- 1. exact fixture: ties and order
@pytest.mark.parametrize("M,Q,k,nc", SHAPES)
def test_exact_fixture_ties_and_order(M, Q, k, nc):
    """every similarity is exact in fp32, so the result is decided by the order alone: ALL queries, no exclusions"""
    bank, queries, labels = knn_util.exact_fixture(M, Q, nc)
    s64 = knn_util.sims64(bank, queries)
    ref_index, ref_sim = knn_util.topk_ref(s64, k)
    r = run(make_bank(bank, labels, nc), dev(queries), k, 0.0)
    classes, votes, index, sim = to_np(r)
    assert (index == ref_index).all(), np.flatnonzero((index != ref_index).any(axis=1))[:10]
    assert (sim.view(np.int32) == ref_sim.astype(np.float32).view(np.int32)).all()
    counts = knn_util.votes_ref(ref_index, ref_sim, labels, nc, 0.0)
    assert (votes.astype(np.float64) == counts).all() and (counts.sum(axis=1) == min(k, M)).all()
    assert (classes == knn_util.classes_ref(counts, ref_index)).all()


# ---------------------------------------------------------------------------------------------------------- 2. random unit features
@pytest.mark.parametrize("M,Q,k,nc", SHAPES)
def test_random_unit_features_against_float64(M, Q, k, nc):
    bank, queries, labels = knn_util.unit_fixture(M, Q, nc)
    b = make_bank(bank, labels, nc)
    qd = dev(queries)
    votes_by_t, classes_by_t = {}, {}
    for t in (0.07, 0.0):
        classes, votes, index, sim = to_np(run(b, qd, k, t))
        votes_by_t[t], classes_by_t[t] = votes, classes
    fig = knn_util.check_against_float64(bank, queries, labels, nc, k, index, sim, votes_by_t, classes_by_t, what=(M, Q, k, nc))
    print(f"knn ({M}, {Q}, {k}, {nc}): {fig}")
    record("test_gpu_knn.random_unit_features", M=M, Q=Q, k=k, n_classes=nc, **fig)


# -------------------------------------------------------------------------------------------------------------------- 3. independence
@pytest.mark.parametrize("M,Q,k,nc", [s for s in SHAPES if s[0] == 4097])
@pytest.mark.parametrize("fixture", ["exact", "unit"])
def test_independent_of_splits_repetition_and_batch(fixture, M, Q, k, nc):
    bank, queries, labels = (knn_util.exact_fixture if fixture == "exact" else knn_util.unit_fixture)(M, Q, nc)
    b = make_bank(bank, labels, nc)
    qd = dev(queries)
    base = run(b, qd, k, 0.07, splits=1)
    for splits in (2, 3, 7, None, 1):            # forced slices, the library's choice, and the first call again
        r = run(b, qd, k, 0.07, splits=splits)
        for name in base._fields:
            assert same_bits(getattr(r, name), getattr(base, name)), (splits, name)
    if Q > 63:
        for splits in (None, 3):
            alone = run(b, qd[:63].contiguous(), k, 0.07, splits=splits)
            for name in base._fields:
                assert same_bits(getattr(alone, name), getattr(base, name)[:63]), (splits, name)


# ------------------------------------------------------------------------------------------------------ 4. layouts and absent pixels
def test_map_layout_and_absent_pixels():
    """a [2, 96, 150] map with NaN pixels scattered through it, read in place, against the row layout on its permuted copy"""
    M, nc, k, plane = 1000, 8, 20, 150
    bank, queries, labels = knn_util.unit_fixture(M, 300, nc)
    g = np.random.default_rng(11)
    absent = np.sort(g.choice(300, size=37, replace=False))
    q = queries.copy()
    q[absent] = np.nan                                        # an uncovered pixel of encode_scene: NaN in all 96 channels
    q[5, 17] = np.nan                                         # one channel is enough
    absent = np.union1d(absent, [5])
    fmap = torch.from_numpy(q).view(2, plane, 96).permute(0, 2, 1).contiguous().cuda()       # [2, 96, 150]
    rows = fmap.permute(0, 2, 1).reshape(300, 96).contiguous()
    b = make_bank(bank, labels, nc)
    for t in (0.07, 0.0):
        a = run(b, rows, k, t)
        m = run(b, fmap, k, t, q_layout=1, plane=plane, vote_layout=1)
        assert same_bits(a.index, m.index) and same_bits(a.sim, m.sim) and torch.equal(a.classes, m.classes)
        assert m.votes.shape == (2, nc, plane)
        assert same_bits(m.votes, a.votes.view(2, plane, nc).permute(0, 2, 1).contiguous())
        classes, votes, index, sim = to_np(a)
        assert (index[absent] == -1).all() and np.isneginf(sim[absent]).all() and (votes[absent] == 0).all() and (classes[absent] == -1).all()
        present = np.setdiff1d(np.arange(300), absent)
        assert (index[present] >= 0).all() and (classes[present] >= 0).all() and not np.isnan(votes).any()
    # the rules of the random-feature test hold on the map, NaN pixels included
    classes, votes, index, sim = to_np(run(b, fmap, k, 0.07, q_layout=1, plane=plane))
    knn_util.check_against_float64(bank, q, labels, nc, k, index, sim, {0.07: votes}, {0.07: classes}, what="map", assert_gap=False)


# ------------------------------------------------------------------------------------------------------------- 5. through the model
def make_encoder(precision):
    from maskedsst_amd import ViTSpatialSpectral
    torch.manual_seed(5)
    return ViTSpatialSpectral(image_size=8, spatial_patch_size=1, spectral_patch_size=10, num_classes=8, dim=96, depth=1, heads=8,
                              mlp_dim=64, channels=50, spectral_pos=torch.arange(5), blockwise_patch_embed=True,
                              precision=precision).cuda()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("stride", [8, 5])
def test_knn_predict_scene_through_the_model(precision, stride):
    from maskedsst_amd import SimMIMSpatialSpectral, feature_bank, knn_classify, knn_predict_scene
    enc = make_encoder(precision)
    g = torch.Generator().manual_seed(3)
    scene = torch.randn(2, 50, 16, 16, generator=g).cuda()
    labels = torch.randint(-1, 8, (2, 16, 16), generator=g).cuda()
    enc.train()
    k = 5
    bank = feature_bank(enc, scene, labels, stride=stride, per_class=8, generator=torch.Generator().manual_seed(4))
    assert 8 <= len(bank) <= 64 and bank.n_classes == 8 and bank.labels.dtype == torch.int32
    res = enc.knn_predict_scene(scene, bank, k=k, stride=stride)
    emb = enc.encode_scene(scene, stride=stride, normalize=True)
    assert enc.training                                                      # the module's mode is left as found
    assert res.classes.shape == (2, 16, 16) and res.classes.dtype == torch.int64 and res.votes.shape == (2, 8, 16, 16)
    assert torch.equal(res.cover, emb.cover)
    covered = emb.cover > 0
    assert bool(covered.all()) == (stride == 8)                              # stride 5: rows and columns 13 .. 15 lie in no window
    assert (res.classes[~covered] == -1).all() and (res.votes.permute(0, 2, 3, 1)[~covered] == 0).all()
    assert (res.classes[covered] >= 0).all()
    # the same bits as the row route on the permuted copy
    rows = emb.features.permute(0, 2, 3, 1).reshape(-1, 96).contiguous()
    flat = knn_classify(bank, rows, k=k)
    assert torch.equal(flat.classes.view(2, 16, 16), res.classes)
    assert same_bits(flat.votes.view(2, 16, 16, 8).permute(0, 3, 1, 2).contiguous(), res.votes)
    # ... the free function, a second call and the encoder inside a SimMIM wrapper too
    other = knn_predict_scene(enc, scene, bank, k=k, stride=stride)
    assert torch.equal(other.classes, res.classes) and same_bits(other.votes, res.votes)
    mim = SimMIMSpatialSpectral(encoder=enc, masking_ratio=0.7, mask_patch_size=4, tube_masking=True,
                                to_pixels_per_spectral_block=True).cuda()
    other = mim.encoder.knn_predict_scene(scene, bank, k=k, stride=stride)
    assert torch.equal(other.classes, res.classes) and same_bits(other.votes, res.votes)
    # ... and the float64 restatement on those features, under the rules of the random-feature test
    flat0 = knn_classify(bank, rows, k=k, temperature=0.0)
    fig = knn_util.check_against_float64(
        bank.features.cpu().numpy(), rows.cpu().numpy(), bank.labels.cpu().numpy(), 8, k, flat.index.cpu().numpy(), flat.sim.cpu().numpy(),
        {0.07: flat.votes.cpu().numpy(), 0.0: flat0.votes.cpu().numpy()}, {0.07: flat.classes.cpu().numpy(), 0.0: flat0.classes.cpu().numpy()},
        what=(precision, stride), assert_gap=False)
    print(f"knn_predict_scene ({precision}, stride {stride}): bank {len(bank)} {fig}")
    # a bank of all labelled covered pixels classifies them with k = 1 perfectly: each pixel finds itself
    full = feature_bank(enc, scene, labels, stride=stride)
    ok = covered & (labels != -1)
    assert len(full) == int(ok.sum())
    own = enc.knn_predict_scene(scene, full, k=1, stride=stride)
    assert torch.equal(own.classes[ok], labels[ok])
    assert (own.votes.permute(0, 2, 3, 1)[covered].sum(dim=1) == 1).all()    # w_1 = 1


def test_bank_checks_its_contents_once():
    from maskedsst_amd import KnnBank
    f = torch.nn.functional.normalize(torch.randn(10, 96, generator=torch.Generator().manual_seed(1)), dim=1).cuda()
    l = torch.arange(10).cuda() % 4
    assert len(KnnBank(f, l, 4)) == 10
    for labels in (l - 1, l + 1):
        with pytest.raises(ValueError, match="labels"):
            KnnBank(f, labels, 4)
    for bad in (float("nan"), float("inf")):
        g = f.clone()
        g[7, 95] = bad
        with pytest.raises(ValueError, match="finite"):
            KnnBank(g, l, 4)


# ------------------------------------------------------------------------------------------------------------------------ 6. scripts
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


def test_finetune_val_knn_script():
    """finetune.py --val-knn: one more line per validation pass, beside --val-embed's, on the same split"""
    out = child([sys.executable, "finetune.py", "--steps", "2", "--val-scenes", "4", "--val-every", "1", "--val-knn", "5", "--val-embed"], 600)
    lines = out.splitlines()
    knn = [l.split() for l in lines if l.startswith("val-knn step ")]
    emb = [l.split() for l in lines if l.startswith("val-embed step ")]
    assert [e[2] for e in knn] == ["1", "2"] and [e[2] for e in emb] == ["1", "2"], out
    for e, m in zip(knn, emb):
        assert e[3:5] == ["k", "5"] and e[5] == "knn_acc" and 0.0 <= float(e[6]) <= 1.0, e
        assert e[7] == "bank_pixels" and int(e[8]) > 0 and e[9] == "test_pixels" and int(e[10]) > 0 and e[11:] == ["scenes", "4"], e
        assert (e[8], e[10]) == (m[8], m[10])          # the split of --val-embed: the two accuracies are comparable


def test_knn_time_script():
    """tools/knn_time.py at a tiny shape: exit 0, ONE JSON line, nothing appended with --append ''"""
    out = child([sys.executable, os.path.join("tools", "knn_time.py"), "--shapes", "300x1000", "--ks", "5", "--steps", "2", "--warmup", "1",
                 "--scene-size", "16", "--bands", "50", "--depth", "1", "--append", ""], 300)
    lines = [l for l in out.splitlines() if l.strip()]
    assert len(lines) == 1, out
    row = json.loads(lines[0])
    assert row["tool"] == "knn_time" and len(row["results"]) == 1
    r = row["results"][0]
    assert (r["Q"], r["M"], r["k"]) == (300, 1000, 5)
    assert r["knn_kernels_ms"] > 0 and r["eager_ms"] > 0 and r["knn_predict_scene_ms"] > 0 and r["eager_scene_ms"] > 0
    assert r["classes_equal_share"] >= 0.95 and r["index_equal_share"] >= 0.95, r   # the eager route rounds differently: not a parity bar
