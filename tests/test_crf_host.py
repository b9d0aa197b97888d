"""Feature-guided CRF refinement, host side (no GPU needed): the C ABI of msst_crf_affinity and msst_crf_step (additive under
MSST_VERSION 109) and their argument checks (they run before any HIP call, so null pointers and host buffers are enough to see them),
the ValueError / RuntimeError surface of maskedsst_amd/crf.py, the flags of finetune.py, and the float64 restatement of
tests/crf_util.py: it agrees with a plain loop over pixels and neighbours, it tells itself apart from its mutations at the committed
bars, and its real-valued cases leave at most 1 % of their live pixels under the margin."""
import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch

import crf_util as cu

BADARG, UNSUPPORTED = -3, -2   # include/msst.h: MSST_ERR_BADARG, MSST_ERR_UNSUPPORTED


# --------------------------------------------------------------------------------------------------------------------- C ABI
def test_c_abi_declares_and_exports_the_entry_points():
    from ctypes import c_float, c_int, c_void_p
    from maskedsst_amd import _lib
    header = open(_lib.HEADER_PATH).read()
    assert _lib.header_version() == 109   # additive: the revision does not move
    lib = _lib.load()
    assert lib.msst_version() == 109
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    P = c_void_p
    sigs = {
        # feat, cover, int Bs, int dim, int Hs, int Ws, int radius, a_tab (host), s_tab (host), float g, k, live, stream
        "msst_crf_affinity": (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, P, P, c_float, P, P, P]),
        # scores, int unary, float unary_scale, q_in, k, live, int Bs, int nc, int Hs, int Ws, int radius, q_out, classes, prev_classes,
        # changed, stream
        "msst_crf_step": (c_int, [P, c_int, c_float, P, P, P, c_int, c_int, c_int, c_int, c_int, P, P, P, P, P]),
    }
    for name, sig in sigs.items():
        m = re.search(r"^int %s\(([^;]*)\);" % name, header, re.M)
        assert m and len(m.group(1).split(",")) == len(sig[1]), name
        assert name in _lib.declared_symbols() and _lib._SIGS[name] == sig
        assert re.search(r" T %s$" % name, out, re.M)
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == sig
    import maskedsst_amd
    for n in ("CrfAffinity", "CrfResult", "RefinedScene", "crf_affinity", "crf_refine", "refine_scene"):
        assert n in maskedsst_amd.__all__ and hasattr(maskedsst_amd, n), n
    assert maskedsst_amd.CrfAffinity._fields == ("weights", "live", "radius")
    assert maskedsst_amd.CrfResult._fields == ("classes", "probs", "history")
    assert maskedsst_amd.RefinedScene._fields == ("classes", "probs", "history", "cover")
    assert hasattr(maskedsst_amd.ViTSpatialSpectral, "refine_scene")
    assert "msst_crf.hip" in __import__("maskedsst_amd.build", fromlist=["SOURCES"]).SOURCES


def _ptr():
    buf = (ctypes.c_char * 1024)()
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)


def test_affinity_refuses_bad_arguments_before_launch():
    from maskedsst_amd import _lib
    lib = _lib.load()
    buf, p = _ptr()
    names = ("feat", "cover", "a_tab", "s_tab", "k", "live")

    def call(Bs=2, dim=96, Hs=5, Ws=7, radius=2, g=2.0, **ptr):
        a = {n: ptr.get(n, p) for n in names}
        return lib.msst_crf_affinity(a["feat"], a["cover"], Bs, dim, Hs, Ws, radius, a["a_tab"], a["s_tab"], g, a["k"], a["live"], None)

    null = {n: None for n in names}
    for bad in (dict(Bs=0), dict(Bs=-1), dict(dim=0), dict(Hs=0), dict(Ws=0), dict(Ws=-3)):
        assert call(**bad) == BADARG and call(**bad, **null) == BADARG, bad
        assert b"msst_crf_affinity" in lib.msst_last_error(), bad
    for over in (dict(dim=95), dict(dim=128), dict(radius=0), dict(radius=-1), dict(radius=4), dict(Bs=1 << 30, Hs=64, Ws=64)):
        assert call(**over) == UNSUPPORTED and call(**over, **null) == UNSUPPORTED, over
        assert b"msst_crf_affinity" in lib.msst_last_error(), over
    for g in (-1.0, float("nan"), float("inf")):
        assert call(g=g) == BADARG and b"g negative" in lib.msst_last_error(), g
    for R in (1, 2, 3):                                              # the limits themselves are inside
        assert call(radius=R, **null) == BADARG and b"null" in lib.msst_last_error()
    for n in names:
        if n != "cover":                                             # cover may be null
            assert call(**{n: None}) == BADARG and b"null" in lib.msst_last_error(), n
        if n != "live":                                              # bytes
            assert call(**{n: ctypes.c_void_p(p.value + 2)}) == BADARG and b"misaligned" in lib.msst_last_error(), n


def test_step_refuses_bad_arguments_before_launch():
    from maskedsst_amd import _lib
    lib = _lib.load()
    buf, p = _ptr()
    buf2, p2 = _ptr()
    names = ("scores", "q_in", "k", "live", "q_out", "classes", "prev_classes", "changed")

    def call(unary=0, unary_scale=1.0, Bs=2, nc=5, Hs=5, Ws=7, radius=2, **ptr):
        a = {n: ptr.get(n, p2 if n == "q_out" else p) for n in names}
        return lib.msst_crf_step(a["scores"], unary, unary_scale, a["q_in"], a["k"], a["live"], Bs, nc, Hs, Ws, radius, a["q_out"], a["classes"],
                                 a["prev_classes"], a["changed"], None)

    null = {n: None for n in names}
    for bad in (dict(Bs=0), dict(nc=0), dict(nc=-1), dict(Hs=0), dict(Ws=-1)):
        assert call(**bad) == BADARG and call(**bad, **null) == BADARG, bad
        assert b"msst_crf_step" in lib.msst_last_error(), bad
    for over in (dict(nc=129), dict(radius=0), dict(radius=4), dict(Bs=1 << 30, Hs=64, Ws=64)):
        assert call(**over) == UNSUPPORTED and call(**over, **null) == UNSUPPORTED, over
    for kw in (dict(unary=-1), dict(unary=2), dict(unary_scale=0.0), dict(unary_scale=-1.0), dict(unary_scale=float("nan")),
               dict(unary_scale=float("inf"))):
        assert call(**kw) == BADARG and b"unary" in lib.msst_last_error(), kw
    for nc in (1, 128):
        assert call(nc=nc, **null) == BADARG and b"null" in lib.msst_last_error()
    for n in ("scores", "k", "live", "q_out"):
        assert call(**{n: None}) == BADARG and b"null" in lib.msst_last_error(), n
    for n in names:
        if n != "live":
            assert call(**{n: ctypes.c_void_p(p.value + 2)}) == BADARG and b"misaligned" in lib.msst_last_error(), n
    assert call(q_in=p2) == BADARG and b"q_in == q_out" in lib.msst_last_error()
    assert call(prev_classes=None) == BADARG and b"changed without" in lib.msst_last_error()


# --------------------------------------------------------------------------------------------------------- the Python surface
def cpu_affinity(Bs=2, Hs=6, Ws=5, R=2):
    from maskedsst_amd import CrfAffinity
    K = (2 * R + 1) ** 2 - 1
    return CrfAffinity(torch.zeros(Bs, K, Hs, Ws), torch.ones(Bs, Hs, Ws, dtype=torch.bool), R)


def test_crf_affinity_refuses_bad_arguments_before_device_work():
    from maskedsst_amd import SceneEmbedding, crf_affinity
    good = torch.zeros(2, 96, 6, 5)
    for f in (torch.zeros(2, 95, 6, 5), torch.zeros(96, 6, 5), torch.zeros(2, 96, 0, 5), good.double(), good.permute(0, 1, 3, 2), None, [[0.0]]):
        with pytest.raises(ValueError):
            crf_affinity(f)
    for cover in (torch.ones(2, 6, 5), torch.ones(2, 6, 4, dtype=torch.int32), torch.ones(1, 6, 5, dtype=torch.int32), "x"):
        with pytest.raises(ValueError):
            crf_affinity(good, cover=cover)
    for kw in (dict(radius=0), dict(radius=4), dict(radius=1.0), dict(radius=True), dict(w_appearance=-1.0), dict(w_smooth=float("nan")),
               dict(theta_feature=0.0), dict(theta_feature=1e-30), dict(theta_position=0.0), dict(theta_smooth=-2.0), dict(theta_smooth="1")):
        with pytest.raises(ValueError):
            crf_affinity(good, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crf_affinity(good)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crf_affinity(SceneEmbedding(good, torch.ones(2, 6, 5, dtype=torch.int32)))


def test_crf_refine_refuses_bad_arguments_before_device_work():
    from maskedsst_amd import ViTSpatialSpectral, crf_refine, refine_scene
    aff = cpu_affinity()
    good = torch.zeros(2, 4, 6, 5)
    for s in (torch.zeros(2, 4, 6, 4), torch.zeros(1, 4, 6, 5), torch.zeros(2, 129, 6, 5), torch.zeros(2, 0, 6, 5), torch.zeros(4, 6, 5),
              good.double(), good.permute(0, 1, 3, 2), None):
        with pytest.raises(ValueError):
            crf_refine(s, aff)
    for kw in (dict(iters=-1), dict(iters=1.5), dict(iters=True), dict(unary="probs"), dict(unary=None), dict(unary_scale=0.0),
               dict(unary_scale=-1.0), dict(unary_scale=float("inf"))):
        with pytest.raises(ValueError):
            crf_refine(good, aff, **kw)
    for bad in (None, (aff.weights, aff.live, 2), aff._replace(radius=4), aff._replace(radius=1), aff._replace(live=aff.live.int()),
                aff._replace(weights=aff.weights.double())):
        with pytest.raises(ValueError):
            crf_refine(good, bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crf_refine(good, aff)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crf_refine(good, aff, iters=0)
    model = ViTSpatialSpectral(image_size=8, spatial_patch_size=1, spectral_patch_size=10, num_classes=4, dim=96, depth=1, heads=8, mlp_dim=64,
                               channels=50, spectral_pos=torch.arange(5), blockwise_patch_embed=True, precision="fp32")
    scene = torch.zeros(2, 50, 16, 16)
    for kw in (dict(embedding="x"), dict(iters=-1), dict(unary="x"), dict(unary_scale=0)):
        with pytest.raises(ValueError):
            refine_scene(model, scene, torch.zeros(2, 4, 16, 16), **kw)
    with pytest.raises(ValueError):
        model.refine_scene(scene, torch.zeros(2, 4, 16))


def test_tables_are_rounded_once_from_float64():
    from maskedsst_amd.crf import crf_offsets, crf_tables
    for R in (1, 2, 3):
        assert crf_offsets(R) == cu.offsets(R) and len(crf_offsets(R)) == (2 * R + 1) ** 2 - 1
        a, s = crf_tables(R, 3.0, 2.0, 1.0, 1.0)
        wa, ws, _ = cu.tables(R)
        assert a.dtype == np.float32 and np.array_equal(a, wa) and np.array_equal(s, ws)
        assert np.array_equal(a, a[::-1]) and np.array_equal(s, s[::-1])            # symmetric under o -> -o: j' = K - 1 - j


def test_finetune_parser_takes_val_crf():
    import finetune
    ap = finetune.build_parser()
    assert ap.parse_args(["enmap"]).val_crf == 0 and ap.parse_args(["enmap"]).val_crf_radius == 2
    a = ap.parse_args(["enmap", "--val-scenes", "4", "--val-every", "1", "--val-crf", "3", "--val-crf-radius", "1"])
    assert a.val_crf == 3 and a.val_crf_radius == 1
    with pytest.raises(SystemExit):
        finetune.check_val_crf(ap.parse_args(["enmap", "--val-crf", "3"]))                       # needs --val-scenes and --val-every
    with pytest.raises(SystemExit):
        finetune.check_val_crf(ap.parse_args(["enmap", "--val-scenes", "4", "--val-every", "1", "--val-crf", "3", "--val-crf-radius", "4"]))
    with pytest.raises(SystemExit):
        finetune.check_val_crf(ap.parse_args(["enmap", "--val-scenes", "4", "--val-every", "1", "--val-crf", "-1"]))
    finetune.check_val_crf(a)
    finetune.check_val_crf(ap.parse_args(["enmap"]))


# ------------------------------------------------------------------------------------------------ the float64 restatement itself
def small_case(R, seed=3):
    rng = np.random.default_rng(seed)
    feat = rng.normal(size=(2, 96, 5, 4)).astype(np.float32)
    cover = np.ones((2, 5, 4), dtype=np.int32)
    feat[0, 5, 1, 2] = np.nan
    feat[1, :, 4, 3] = 0.0
    cover[1, 0, 0] = 0
    return feat, cover


@pytest.mark.parametrize("R", [1, 2, 3])
def test_restatement_against_a_plain_loop(R):
    feat, cover = small_case(R)
    a, s, g = cu.tables(R)
    k, live = cu.affinity(feat, cover, R, a, s, g)
    k2, live2 = cu.affinity_loops(feat, cover, R, a, s, g)
    assert np.array_equal(live, live2) and int((~live).sum()) == 3
    assert np.abs(k - k2).max() < 1e-13 and np.array_equal(k == 0, k2 == 0)
    rng = np.random.default_rng(R)
    scores = rng.normal(size=(2, 3, 5, 4)).astype(np.float32)
    scores[0, 1, 2, 2] = np.nan
    scores[1, 2] = -np.inf
    lv = cu.live_refine(live, scores)
    assert int((live & ~lv).sum()) == 1
    U = cu.unaries(scores, "logits", 0.7)
    q = cu.step(U, lv, k, None, R)
    for _ in range(2):
        q2 = cu.step_loops(U, lv, k, q, R)
        q = cu.step(U, lv, k, q, R)
        assert np.array_equal(np.isnan(q), np.isnan(q2)) and np.nanmax(np.abs(q - q2)) < 1e-13
    assert np.array_equal(np.isnan(q).all(axis=1), ~lv) and bool((q[1, 2][lv[1]] == 0).all())
    assert abs(np.nansum(q, axis=1)[lv] - 1).max() < 1e-13


def test_restatement_rules():
    # ties go to the lowest class; a dead pixel is -1; votes of 0 are floored, not -inf
    q = np.array([0.25, 0.25, 0.25, 0.25]).reshape(1, 4, 1, 1).repeat(2, axis=3)
    live = np.array([[[True, False]]])
    assert cu.argmax(q, live).tolist() == [[[0, -1]]] and cu.argmax(q, live, "ties_highest").tolist() == [[[3, -1]]]
    assert cu.unaries(np.array([0.0, 1.0], dtype=np.float32), "votes", 2.0).tolist() == [2.0 * np.log(1e-30), 0.0]
    # the whole-number affinity: s[j] = j + 1 where both ends live, 0 elsewhere, the neighbour order dy-major
    feat, cover, dead = cu.int_case((3, 4), "corner")
    a, s = cu.int_tables(1)
    k, live = cu.affinity(feat, cover, 1, a, s, 2.0)
    assert np.array_equal(live, ~dead) and set(np.unique(k)) <= set(range(9))
    assert k[0, :, 1, 1].tolist() == [0, 2, 3, 4, 5, 6, 7, 8] and k[0, :, 0, 1].tolist() == [0, 0, 0, 0, 5, 6, 7, 8]
    assert bool((k[:, :, 0, 0] == 0).all())


def committed(case):
    bar = cu.bars(case)
    assert bar is not None, "profiles/crf_parity_measured.jsonl is not committed: nothing to hold the mutants against"
    return bar


def test_committed_bars_tell_the_mutants_apart():
    """every bar is 4 x a committed measurement, and every mutated restatement lies beyond the bar of a case that is there to catch it
    (or, where the GPU comparison is exact, differs)"""
    seen = set()
    # the exact affinity: no bar, any difference shows
    feat, cover, _ = cu.int_case((7, 9), "row")
    a, s = cu.int_tables(2)
    ref, _ = cu.affinity(feat, cover, 2, a, s, 2.0)
    for m in ("centre_counted", "order_transposed", "wrap_around", "next_scene"):
        assert not np.array_equal(cu.affinity(feat, cover, 2, a, s, 2.0, mutate=m)[0], ref), m
        seen.add(m)
    # the real-valued affinity
    for R, form in cu.AFF_REAL:
        bar = committed(f"affinity_R{R}_{form}")
        assert set(bar) == {"k"} and 0 < bar["k"] < 1e-4, bar
        feat, cover, _ = cu.real_features(cu.AFF_REAL_SHAPE, form, 5)
        a, s, g = cu.tables(R)
        ref, _ = cu.affinity(feat, cover, R, a, s, g)
        for m in cu.AFF_MUTANTS:
            if m == "no_rn" and form == "normalized":
                continue                                            # unit vectors: the raw dot is the cosine
            am, sm, gm = cu.tables(R, mutate=m)
            assert cu.rel_err(cu.affinity(feat, cover, R, am, sm, gm, mutate=m)[0], ref) > bar["k"], (R, form, m)
            seen.add(m)
    # the step and the refinement
    for nc, R, unary in cu.REFINE_CASES:
        bar = committed(f"refine_nc{nc}_R{R}_{unary}")
        assert set(bar) == {"probs"} and 0 < bar["probs"] < 1e-4, bar
        scores, k, live = cu.refine_case(nc, R, unary)
        cls, probs, hist, _, lv = cu.refine(scores, k, live, R, cu.REFINE_ITERS, unary)
        for m in cu.STEP_MUTANTS:
            c2, p2, h2, _, _ = cu.refine(scores, k, live, R, cu.REFINE_ITERS, unary, mutate=m)
            if m == "ties_highest":
                continue                                            # (no ties in a real-valued case: the exact case below)
            differs = not np.array_equal(np.isnan(p2), np.isnan(probs)) or cu.rel_err(p2, probs) > bar["probs"]
            assert differs, (nc, R, unary, m)
            seen.add(m)
    flat = np.zeros((1, 4, 3, 3), dtype=np.float32)                  # equal scores, zero weights: every class ties
    kz, lz = np.zeros((1, 8, 3, 3), dtype=np.float32), np.ones((1, 3, 3), dtype=bool)
    assert not np.array_equal(cu.refine(flat, kz, lz, 1, 1)[0], cu.refine(flat, kz, lz, 1, 1, mutate="ties_highest")[0])
    seen.add("ties_highest")
    assert seen == set(cu.MUTANTS)


def test_real_cases_leave_few_pixels_under_the_margin():
    """the classes of a real-valued case are compared on every live pixel whose float64 top-two margin reaches 4 x the measured
    probability error: computed from the float64 restatement alone, at most 1 % of a case's live pixels lie under it, at every step"""
    for nc, R, unary in cu.REFINE_CASES:
        gap = committed(f"refine_nc{nc}_R{R}_{unary}")["probs"]
        scores, k, live = cu.refine_case(nc, R, unary)
        _, _, hist, qs, lv = cu.refine(scores, k, live, R, cu.REFINE_ITERS, unary)
        assert lv.sum() > 1000 and hist.sum() > 0, (nc, R, unary, hist)           # the refinement does move pixels
        for q in qs:
            under = (cu.margin(q, lv) < gap) & lv
            assert under.sum() <= cu.MARGIN_SHARE * lv.sum(), (nc, R, unary, int(under.sum()))
    for nc in cu.STEP_NC:
        for R in cu.STEP_R:
            for unary in ("logits", "votes"):
                gap = committed(f"step_nc{nc}_R{R}_{unary}")["q1"]
                scores, k, live, q0 = cu.step_case(nc, R, unary)
                lv = cu.live_refine(live, scores)
                q1 = cu.step(cu.unaries(scores, unary, 1.0), lv, k, q0, R)
                for q in (q0.astype(np.float64), q1):
                    under = (cu.margin(q, lv) < gap) & lv
                    assert under.sum() <= cu.MARGIN_SHARE * lv.sum(), (nc, R, unary, int(under.sum()))
