"""GPU: PCA, whitening and RX scores of frozen features -- msst_feat_moments / msst_feat_moments_finish / msst_feat_project
(maskedsst_amd/csrc/msst_pca.hip) against the restatement of tests/pca_util.py: exact on whole-number data (no tolerance: counts, raw
sums, the symmetry of s2, NaN rows, both layouts, the finish bit for bit), the two-pass fit against float64 on a well-conditioned and
an offset cloud, the projection onto given components, equal bits from equal inputs, the route through the model and the two
scripts.  The bars are 4 x the errors measured on the MI355X (profiles/pca_parity_measured.jsonl);
tests/test_pca_host.py checks on the CPU that they still tell the mutated restatements apart."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import pca_util as pu

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


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def moments(features, centre=None, ddof=1):
    """feature_moments with every output prefilled: (count, mean [96], cov [96, 96], s1 [96], s2 [96, 96]) on the CPU"""
    from maskedsst_amd.pca import feature_moments
    out = torch.full((2 + 96 + 96 * 96,), float("nan"), device="cuda")
    m = feature_moments(features, None if centre is None else dev(centre), ddof, raw=True, out=out)
    return int(m.count.cpu()[0]), m.mean.cpu(), m.cov.cpu(), m.raw[:96].cpu(), m.raw[96:].view(96, 96).cpu()


def check_exact(x, features):
    """the moments of `features` (x [M, 96] numpy as rows or as a map) against the whole-number reference, bit for bit"""
    for centre in (None, pu.int_centre()):
        n, s1, s2 = pu.int_moments(x, centre)
        assert np.abs(s2).max() < 2 ** 24
        for ddof in (1, 0):
            count, mean, cov, r1, r2 = moments(features, centre, ddof)
            assert count == n
            assert torch.equal(r1, torch.from_numpy(s1.astype(np.float32))) and torch.equal(r2, torch.from_numpy(s2.astype(np.float32)))
            assert same_bits(r2, r2.t().contiguous())                                        # symmetric bit for bit
            want_mean, want_cov = pu.finish_exact(n, s1, s2, centre, ddof)
            assert same_bits(mean, torch.from_numpy(want_mean)) or (n == 0 and bool(torch.isnan(mean).all()))
            if n - ddof <= 0:
                assert bool(torch.isnan(cov).all())
            else:
                assert same_bits(cov, torch.from_numpy(want_cov)) and same_bits(cov, cov.t().contiguous())
        again = moments(features, centre, 0)
        assert again[0] == count and all(same_bits(a, b) or (n == 0 and a.shape == b.shape) for a, b in zip(again[1:], (mean, cov, r1, r2)))


# --------------------------------------------------------------------------------------------------- 1. exact on whole numbers
@pytest.mark.parametrize("M", pu.INT_ROWS)
def test_moments_are_exact_on_rows(M):
    for kind in pu.NAN_KINDS:
        x = pu.int_case(M, kind)
        check_exact(x, dev(x))


@pytest.mark.parametrize("shape", pu.INT_MAPS)
def test_moments_are_exact_on_a_map_read_in_place(shape):
    Bs, Hs, Ws = shape
    for kind in pu.NAN_KINDS:
        x = pu.int_case(Bs * Hs * Ws, kind)
        check_exact(x, dev(pu.to_map(x, Bs, Hs * Ws)).view(Bs, 96, Hs, Ws))


# ------------------------------------------------------------------------------------------------------------ 2. against float64
@pytest.mark.parametrize("form", pu.REAL_FORMS)
@pytest.mark.parametrize("M", pu.REAL_ROWS)
def test_fit_against_float64(M, form):
    from maskedsst_amd import fit_pca
    x = pu.real_case(M, form)
    ref = pu.fit64(x)
    xd = dev(x)
    pca = fit_pca(xd)
    lam = pca.explained_variance
    got = dict(mean=pca.mean.cpu().double().numpy(), cov=pca.covariance, eigenvalues=lam, evr=pca.explained_variance_ratio,
               effective_rank=pca.effective_rank)
    err = pu.fit_errors(got, ref)
    case = pu.case_name(M, form)
    print(f"{case}: {err}")
    pu.note(case, err)
    assert pca.count == ref["count"] == M - pu.REAL_NAN_ROWS and pca.rank == ref["rank"] == 96
    assert pu.within(err, pu.bars(case)) == []
    # the rules: descending and clamped, unit rows, the largest entry of every component positive
    comp = pca.components.cpu().double().numpy()
    assert comp.shape == (96, 96) and (np.diff(lam) <= 0).all() and (lam >= 0).all()
    assert np.abs((comp * comp).sum(axis=1) - 1).max() < 1e-6 and (comp[np.arange(96), np.argmax(np.abs(comp), axis=1)] > 0).all()
    # the leading directions, 8 % apart in eigenvalue, are the float64 ones (the later ones turn inside near-degenerate planes)
    assert (np.abs((comp[:8] * ref["components"][:8]).sum(axis=1)) > 1 - 1e-6).all()
    # the covariance is symmetric bit for bit, and a second fit repeats every bit
    assert np.array_equal(pca.covariance, pca.covariance.T)
    again = fit_pca(xd, n_components=3)
    assert same_bits(again.mean, pca.mean) and np.array_equal(again.covariance, pca.covariance) and again.n_components == 3
    assert same_bits(again.components, pca.components[:3]) and np.array_equal(again.explained_variance, lam)


def test_fit_refuses_too_few_counted_rows_and_takes_a_bank():
    from maskedsst_amd import KnnBank, fit_pca
    x = pu.int_case(65, "all")
    with pytest.raises(ValueError, match="rows without a NaN"):
        fit_pca(dev(x))
    one = pu.int_case(65, "none")
    one[1:, 0] = np.nan
    with pytest.raises(ValueError, match="rows without a NaN"):
        fit_pca(dev(one))
    assert fit_pca(dev(one), ddof=0).count == 1
    xr = pu.real_case(3000, "offset")
    xr = xr[np.isfinite(xr).all(axis=1)]
    bank = KnnBank(dev(xr), torch.zeros(len(xr), dtype=torch.int64).cuda(), 2)
    a, b = fit_pca(bank), fit_pca(dev(xr))
    assert same_bits(a.mean, b.mean) and np.array_equal(a.covariance, b.covariance) and a.count == len(xr)


# ---------------------------------------------------------------------------------------------------------------- 3. projection
@pytest.mark.parametrize("r", pu.PROJECT_R)
def test_projection_onto_given_components(r):
    from maskedsst_amd.pca import feature_project
    mean, comp = pu.project_tables(r)
    md, cd = dev(mean), dev(comp)
    worst = dict(out=0.0, sumsq=0.0)
    for rows, Bs, plane in pu.project_shapes(r):
        x = pu.project_rows(rows)
        want_out, want_ss = pu.project64(x, mean, comp)
        xr, xm = dev(x), dev(pu.to_map(x, Bs, plane)).view(Bs, 96, plane, 1)
        out, ss = feature_project(xr, md, cd, sumsq=True)
        assert out.shape == (rows, r) and ss.shape == (rows,)
        bad = torch.from_numpy(np.isnan(x).any(axis=1))
        assert bool(torch.isnan(out.cpu()[bad]).all()) and bool(torch.isnan(ss.cpu()[bad]).all()) and int(bad.sum()) == (rows > 1)
        worst["out"] = max(worst["out"], pu.relmax(out.cpu().numpy(), want_out))                # (NaN positions must coincide)
        worst["sumsq"] = max(worst["sumsq"], pu.relmax(ss.cpu().numpy(), want_ss))
        # the same bits from a map, into a map, and without `out`
        for src, out_layout in ((xm, 0), (xm, 1)):
            o, s = feature_project(src, md, cd, out_layout=out_layout, sumsq=True)
            if out_layout == 1:
                assert o.shape == (Bs, r, plane, 1)
                o = torch.from_numpy(pu.from_map(o.view(Bs, r, plane).cpu().numpy())).cuda()
            assert same_bits(o, out) and same_bits(s.reshape(-1), ss)
        assert same_bits(feature_project(xr, md, cd, out=False, sumsq=True)[1], ss)
        assert same_bits(feature_project(xm, md, cd, out=False, sumsq=True)[1].reshape(-1), ss)
        assert same_bits(feature_project(xr, md, cd)[0], out) and feature_project(xr, md, cd)[1] is None
        # a row alone has the bits it has in the batch
        for k in sorted({0, rows // 3, rows - 1}):
            o1, s1 = feature_project(xr[k:k + 1].contiguous(), md, cd, sumsq=True)
            assert same_bits(o1[0], out[k]) and same_bits(s1[0], ss[k])
    case = f"project_r{r}"
    print(f"{case}: {worst}")
    pu.note(case, worst)
    assert pu.within(worst, pu.bars(case)) == []


def test_transform_whiten_and_mahalanobis():
    """FeaturePCA on a fit: transform is the projection onto the components, whitening divides by sqrt(lambda) and drops the columns
    from rank on, mahalanobis is the squared norm of the whitened scores"""
    from maskedsst_amd import FeaturePCA, fit_pca
    x = pu.real_case(3000, "offset")
    xd = dev(x)
    pca = fit_pca(xd)
    ref = dict(mean=pca.mean.cpu().numpy(), components=pca._c64, eigenvalues=pca.explained_variance, rank=pca.rank)
    z, zw, d2 = pca.transform(xd), pca.transform(xd, whiten=True), pca.mahalanobis(xd)
    assert z.shape == (3000, 96) and zw.shape == (3000, pca.rank) and d2.shape == (3000,)
    want_w, want_d2 = pu.project64(x, ref["mean"], pu.whiten64(ref).astype(np.float32))      # the directions as the kernel gets them
    err = dict(out=pu.relmax(z.cpu().numpy(), pu.project64(x, ref["mean"], pca.components.cpu().numpy())[0]),
               whitened=pu.relmax(zw.cpu().numpy(), want_w), mahalanobis=pu.relmax(d2.cpu().numpy(), want_d2))
    print(f"transform_offset_3000: {err}")
    pu.note("transform_offset_3000", err)
    assert pu.within(err, pu.bars("transform_offset_3000")) == []
    assert int(torch.isnan(d2).sum()) == pu.REAL_NAN_ROWS
    # a rank below the component count: the columns from rank on are dropped
    lam = pca.explained_variance.copy()
    lam[40:] = 0.0
    low = FeaturePCA(pca.mean, pca.components, lam, pca.count)
    assert low.rank == 40 and low.transform(xd, whiten=True).shape == (3000, 40) and low.transform(xd).shape == (3000, 96)
    # (against the same given fp32 components: the fit scales its float64 ones, so its whitened directions round differently)
    full = FeaturePCA(pca.mean, pca.components, pca.explained_variance, pca.count)
    assert same_bits(low.transform(xd, whiten=True), full.transform(xd, whiten=True)[:, :40].contiguous())
    assert same_bits(full.transform(xd), z)
    few = fit_pca(xd, n_components=3)
    assert same_bits(few.transform(xd), z[:, :3].contiguous())
    with pytest.raises(ValueError, match="leading components"):
        few.mahalanobis(xd)


# ----------------------------------------------------------------------------------------------------------- 4. through the model
def make_model(nc=5):
    from maskedsst_amd import ViTSpatialSpectral
    torch.manual_seed(5)
    return ViTSpatialSpectral(image_size=8, spatial_patch_size=1, spectral_patch_size=10, num_classes=nc, dim=96, depth=2, heads=8,
                              mlp_dim=64, channels=50, spectral_pos=torch.arange(5), blockwise_patch_embed=True, precision="fp32").cuda()


@pytest.mark.parametrize("stride", [8, 5])
def test_scene_calls_through_the_model(stride):
    from maskedsst_amd import AnomalyScene, PcaScene, anomaly_scene, fit_pca, pca_scene
    model = make_model()
    model.train()
    g = torch.Generator().manual_seed(3)
    scene = torch.randn(2, 50, 16, 16, generator=g).cuda()
    emb = model.encode_scene(scene, stride=stride, normalize=False)
    covered = emb.cover > 0
    assert bool(covered.all()) == (stride == 8)                              # stride 5: rows and columns 13 .. 15 lie in no window
    n = int(covered.sum())
    rows = emb.features.permute(0, 2, 3, 1).reshape(-1, 96).contiguous()
    # the map read in place is the rows in the same order: every bit of the fit agrees
    on_map, on_emb, on_rows = fit_pca(emb.features), fit_pca(emb), fit_pca(rows)
    for other in (on_emb, on_rows):
        assert other.count == on_map.count == n and same_bits(other.mean, on_map.mean) and np.array_equal(other.covariance, on_map.covariance)
        assert same_bits(other.components, on_map.components)
    # ... and the gathered covered rows: the same rows in other tiles.  All covered: the same tiles, the same bits; otherwise two
    # fp32 two-pass sums of n <= 512 rows, each within n 2^-24 / 2 = 1.6e-5 of the exact covariance at the worst
    gathered = fit_pca(rows[covered.reshape(-1)].contiguous())
    assert gathered.count == n
    if stride == 8:
        assert same_bits(gathered.mean, on_map.mean) and np.array_equal(gathered.covariance, on_map.covariance)
    else:
        assert pu.relmax(gathered.covariance, on_map.covariance) <= 3.2e-5 and pu.relmax(gathered.mean.cpu().numpy(), on_map.mean.cpu().numpy()) <= 3.2e-5
    # pca_scene is transform on the permuted map
    pca = fit_pca(emb.features, n_components=3)
    for whiten in (False, True):
        res = model.pca_scene(scene, pca, stride=stride, whiten=whiten)
        assert isinstance(res, PcaScene) and model.training and res.components.shape == (2, 3, 16, 16) and torch.equal(res.cover, emb.cover)
        z = pca.transform(rows, whiten=whiten)
        assert same_bits(res.components.permute(0, 2, 3, 1).reshape(-1, 3).contiguous(), z)
        nan = torch.isnan(res.components)
        assert torch.equal(nan.any(dim=1), ~covered) and torch.equal(nan.all(dim=1), ~covered)
        other = pca_scene(model, scene, pca, stride=stride, whiten=whiten)
        assert same_bits(other.components, res.components)
    # anomaly_scene: global RX on the scene's own covered pixels
    res = model.anomaly_scene(scene, stride=stride)
    assert isinstance(res, AnomalyScene) and model.training and res.score.shape == (2, 16, 16) and torch.equal(res.cover, emb.cover)
    assert torch.equal(torch.isnan(res.score), ~covered) and bool((res.score[covered] >= 0).all())
    assert res.pca.count == n and same_bits(res.pca.mean, on_map.mean) and np.array_equal(res.pca.covariance, on_map.covariance)
    total, want = float(res.score[covered].double().sum()), (n - 1) * res.pca.rank
    err = dict(trace=abs(total - want) / want)
    case = f"trace_scene_stride{stride}"
    print(f"{case}: sum {total} against {n - 1} x {res.pca.rank}: {err}")
    pu.note(case, err)
    assert res.pca.rank >= 1 and pu.within(err, pu.bars(case)) == []
    given = anomaly_scene(model, scene, on_map, stride=stride)
    assert same_bits(given.score, res.score) and given.pca is on_map
    assert same_bits(on_map.mahalanobis(rows).view(2, 16, 16), res.score)


# ------------------------------------------------------------------------------------------------------------------------ 5. scripts
def test_finetune_val_pca_script():
    """finetune.py --val-pca: one more line per validation pass"""
    out = child([sys.executable, "finetune.py", "--steps", "2", "--val-scenes", "4", "--val-every", "1", "--val-pca", "3"], 600)
    lines = [l.split() for l in out.splitlines() if l.startswith("val-pca step ")]
    assert [e[2] for e in lines] == ["1", "2"], out
    for e in lines:
        assert e[3] == "rows" and int(e[4]) == 2 * 64 * 64 and e[5] == "evr", e
        evr = [float(v) for v in e[6:9]]
        assert 1.0 >= evr[0] >= evr[1] >= evr[2] >= 0.0 and sum(evr) <= 1.0 + 1e-6, e
        assert e[9] == "effective_rank" and 1.0 <= float(e[10]) <= 96.0, e
        assert e[11] == "rx_mean" and float(e[12]) > 0 and e[13] == "rx_max" and float(e[14]) >= float(e[12]) and e[15:] == ["scenes", "4"], e


def test_pca_time_script():
    """tools/pca_time.py --smoke: exit 0 and ONE JSON line, nothing appended"""
    out = child([sys.executable, os.path.join("tools", "pca_time.py"), "--smoke"], 300)
    lines = [l for l in out.splitlines() if l.strip()]
    assert len(lines) == 1, out
    row = json.loads(lines[0])
    assert row["tool"] == "pca_time" and row["M"] == 8192 and row["r"] == 3
    assert row["fit_us"] > 0 and row["eager_fit_us"] > 0 and row["project_us"] > 0 and row["eager_project_us"] > 0
