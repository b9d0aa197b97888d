"""Float64 numpy restatement of the CRF refinement (maskedsst_amd/crf.py, msst_crf_affinity, msst_crf_step), the case generators of
tests/test_gpu_crf.py and the bars (profiles/crf_parity_measured.jsonl: 4 x the error measured on the MI355X).  Written with padded
arrays -- no unfold, none of the product's code paths.  Nothing here needs a GPU.

The mutants are restatements with one rule broken; tests/test_crf_host.py checks that the bars still tell each from the true one."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY_FILE = os.path.join(ROOT, "profiles", "crf_parity_measured.jsonl")
D = 96
AFF_TILE = (8, 16)        # the tile of msst_crf_affinity (rows, columns)
STEP_TILE = (8, 32)       # the tile of msst_crf_step
MARGIN_SHARE = 0.01       # the share of live pixels a case may leave under the margin
MUTANTS = ["centre_counted", "order_transposed", "wrap_around", "next_scene", "dead_times_zero", "theta_not_squared", "potts_sign",
           "no_rn", "ties_highest"]
AFF_MUTANTS = ["centre_counted", "order_transposed", "wrap_around", "next_scene", "theta_not_squared", "no_rn"]
STEP_MUTANTS = ["centre_counted", "order_transposed", "wrap_around", "next_scene", "dead_times_zero", "potts_sign", "ties_highest"]

# ---- the exact cases
INT_SHAPES = [(1, 1), (1, 5), (7, 9), (3, 65), (9, 17), (17, 33)]     # 9 x 17: one pixel past the affinity's tile both ways; 17 x 33: past two
INT_BS = 3
DEAD_KINDS = ["none", "corner", "row", "tile", "all"]
# ---- the real-valued cases
AFF_REAL = [(R, form) for R in (1, 2, 3) for form in ("raw", "normalized")]
AFF_REAL_SHAPE = (2, 19, 37)
STEP_NC = [1, 2, 17, 128]
STEP_R = [1, 3]
STEP_SHAPE = (2, 11, 37)                                               # past the step's tile both ways
REFINE_CASES = [(17, 2, "logits"), (5, 3, "votes")]                   # (nc, R, unary)
REFINE_SHAPE = (2, 21, 37)
REFINE_ITERS = 5


def offsets(R, mutate=None):
    r = range(-R, R + 1)
    if mutate == "order_transposed":
        return [(dy, dx) for dx in r for dy in r if (dy, dx) != (0, 0)]
    if mutate == "centre_counted":
        return [(dy, dx) for dy in r for dx in r][:-1]
    return [(dy, dx) for dy in r for dx in r if (dy, dx) != (0, 0)]


def tables(R, w_appearance=3.0, theta_feature=0.5, theta_position=2.0, w_smooth=1.0, theta_smooth=1.0, mutate=None):
    """(a [K], s [K], g) as the kernel takes them: float64 values rounded to fp32 once"""
    o2 = np.array([dy * dy + dx * dx for dy, dx in offsets(R)], dtype=np.float64)
    sq = (lambda t: t) if mutate == "theta_not_squared" else (lambda t: t * t)
    a = w_appearance * np.exp(-o2 / (2.0 * sq(theta_position)))
    s = w_smooth * np.exp(-o2 / (2.0 * sq(theta_smooth)))
    return a.astype(np.float32), s.astype(np.float32), float(np.float32(1.0 / (2.0 * sq(theta_feature))))


def shifted(x, R, dy, dx, fill, mutate=None):
    """x [Bs, C, Hs, Ws] read at p + (dy, dx), `fill` outside the scene: a padded array and a slice"""
    Bs, C, Hs, Ws = x.shape
    if mutate == "wrap_around":
        return np.roll(x, (-dy, -dx), axis=(2, 3))
    if mutate == "next_scene":                      # the scenes of the batch stacked into one tall scene
        t = x.transpose(1, 0, 2, 3).reshape(1, C, Bs * Hs, Ws)
        return shifted(t, R, dy, dx, fill).reshape(C, Bs, Hs, Ws).transpose(1, 0, 2, 3)
    pad = np.full((Bs, C, Hs + 2 * R, Ws + 2 * R), fill, dtype=x.dtype)
    pad[:, :, R:R + Hs, R:R + Ws] = x
    return pad[:, :, R + dy:R + dy + Hs, R + dx:R + dx + Ws]


def live_affinity(feat, cover=None):
    f = feat.astype(np.float64)
    fin = np.isfinite(f).all(axis=1)
    norm = np.sqrt((np.where(fin[:, None], f, 0.0) ** 2).sum(axis=1))
    live = fin & (norm > 0)
    if cover is not None:
        live &= cover > 0
    return live, norm


def affinity(feat, cover, R, a, s, g, mutate=None):
    """(k [Bs, K, Hs, Ws] float64, live [Bs, Hs, Ws] bool)"""
    live, norm = live_affinity(feat, cover)
    f = np.where(live[:, None], feat.astype(np.float64), 0.0)
    if mutate != "no_rn":
        f = f / np.where(live, norm, 1.0)[:, None]
    a, s = np.asarray(a, dtype=np.float64), np.asarray(s, dtype=np.float64)
    lv = live[:, None].astype(np.float64)
    k = np.zeros((feat.shape[0], len(a)) + feat.shape[2:])
    for j, (dy, dx) in enumerate(offsets(R, mutate)):
        fq = shifted(f, R, dy, dx, 0.0, mutate)
        lq = shifted(lv, R, dy, dx, 0.0, mutate)[:, 0] > 0
        d2 = np.maximum(0.0, 2.0 * (1.0 - (f * fq).sum(axis=1)))
        k[:, j] = np.where(live & lq, a[j] * np.exp(-d2 * g) + s[j], 0.0)
    return k, live


def affinity_loops(feat, cover, R, a, s, g):
    """the same by a plain loop over scenes, pixels and neighbours"""
    Bs, _, Hs, Ws = feat.shape
    offs = offsets(R)
    k = np.zeros((Bs, len(offs), Hs, Ws))
    live = np.zeros((Bs, Hs, Ws), dtype=bool)
    f = feat.astype(np.float64)
    for b in range(Bs):
        for y in range(Hs):
            for x in range(Ws):
                v = f[b, :, y, x]
                live[b, y, x] = np.isfinite(v).all() and np.sqrt((v * v).sum()) > 0 and (cover is None or cover[b, y, x] > 0)
    for b in range(Bs):
        for y in range(Hs):
            for x in range(Ws):
                for j, (dy, dx) in enumerate(offs):
                    qy, qx = y + dy, x + dx
                    if not (0 <= qy < Hs and 0 <= qx < Ws) or not live[b, y, x] or not live[b, qy, qx]:
                        continue
                    p, q = f[b, :, y, x], f[b, :, qy, qx]
                    cos = (p * q).sum() / (np.sqrt((p * p).sum()) * np.sqrt((q * q).sum()))
                    k[b, j, y, x] = a[j] * np.exp(-max(0.0, 2.0 * (1.0 - cos)) * g) + s[j]
    return k, live


def unaries(scores, unary, scale):
    sc = scores.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return scale * sc if unary == "logits" else scale * np.log(np.maximum(np.where(np.isnan(sc), 0.0, sc), 1e-30))


def live_refine(live, scores):
    return live & ~np.isnan(scores).any(axis=1) & (scores > -np.inf).any(axis=1)


def softmax(x, live):
    """softmax over axis 1 with the maximum subtracted; NaN where dead"""
    x = np.where(live[:, None], x, 0.0)
    with np.errstate(invalid="ignore"):
        e = np.exp(x - x.max(axis=1, keepdims=True))
    return np.where(live[:, None], e / e.sum(axis=1, keepdims=True), np.nan)


def step(U, live, k, q_in, R, mutate=None):
    """one mean-field step (q_in None: step 0); k as the kernel is given it"""
    if q_in is None:
        return softmax(U, live)
    msg = np.zeros_like(U)
    sends = ~np.isnan(q_in).any(axis=1, keepdims=True)
    for j, (dy, dx) in enumerate(offsets(R, mutate)):
        qq = shifted(q_in.astype(np.float64), R, dy, dx, np.nan, mutate)
        kj = k[:, j:j + 1].astype(np.float64)
        if mutate == "dead_times_zero":
            msg = msg + np.where(shifted(sends.astype(np.float64), R, dy, dx, 0.0) > 0, 1.0, 0.0) * kj * qq
        else:
            msg = msg + np.where(np.isnan(qq), 0.0, kj * qq)
    with np.errstate(invalid="ignore"):
        x = U - msg if mutate == "potts_sign" else U + msg
    return softmax(x, live & ~np.isnan(x).any(axis=1) if mutate == "dead_times_zero" else live)


def step_loops(U, live, k, q_in, R):
    """the same by a plain loop over scenes, pixels, classes and neighbours"""
    Bs, nc, Hs, Ws = U.shape
    out = np.full(U.shape, np.nan)
    for b in range(Bs):
        for y in range(Hs):
            for x in range(Ws):
                if not live[b, y, x]:
                    continue
                v = U[b, :, y, x].copy()
                for c in range(nc):
                    for j, (dy, dx) in enumerate(offsets(R)):
                        qy, qx = y + dy, x + dx
                        if 0 <= qy < Hs and 0 <= qx < Ws and not np.isnan(q_in[b, c, qy, qx]):
                            v[c] += k[b, j, y, x] * q_in[b, c, qy, qx]
                e = np.exp(v - v.max())
                out[b, :, y, x] = e / e.sum()
    return out


def argmax(q, live, mutate=None):
    """value descending, then class ascending; -1 where dead"""
    z = np.where(live[:, None], q, 0.0)
    c = z.shape[1] - 1 - np.argmax(z[:, ::-1], axis=1) if mutate == "ties_highest" else np.argmax(z, axis=1)
    return np.where(live, c, -1).astype(np.int64)


def margin(q, live):
    """the top-two probability gap per pixel (inf where dead or with one class)"""
    z = np.sort(np.where(live[:, None], q, 0.0), axis=1)
    gap = z[:, -1] - z[:, -2] if q.shape[1] > 1 else np.full(live.shape, np.inf)
    return np.where(live, gap, np.inf)


def refine(scores, k, live_aff, R, iters, unary="logits", scale=1.0, mutate=None):
    """(classes int64, probs float64, history [iters], every Q_t, live)"""
    live = live_refine(live_aff, scores)
    U = unaries(scores, unary, scale)
    qs = [step(U, live, k, None, R)]
    cls = [argmax(qs[0], live, mutate)]
    hist = []
    for _ in range(iters):
        q = step(U, live, k, qs[-1], R, mutate)
        lv = live & ~np.isnan(q).any(axis=1)
        qs.append(q)
        cls.append(argmax(q, lv, mutate))
        hist.append(int((live & (cls[-1] != cls[-2])).sum()))
    return cls[-1], qs[-1], np.array(hist, dtype=np.int64), qs, live


# ------------------------------------------------------------------------------------------------------------------- the cases
def int_tables(R):
    K = (2 * R + 1) ** 2 - 1
    return np.zeros(K, dtype=np.float32), np.arange(1, K + 1, dtype=np.float32)


def kill(feat, cover, kind):
    """dead pixels in every scene of a map, the cause cycling NaN features / zero features / cover == 0 by pixel"""
    Bs, _, Hs, Ws = feat.shape
    dead = np.zeros((Hs, Ws), dtype=bool)
    if kind == "corner":
        dead[0, 0] = dead[-1, -1] = True
    elif kind == "row":
        dead[Hs // 2] = True
    elif kind == "tile":
        dead[:AFF_TILE[0], :AFF_TILE[1]] = True
    elif kind == "all":
        dead[:] = True
    ys, xs = np.nonzero(dead)
    for i, (y, x) in enumerate(zip(ys, xs)):
        for b in range(Bs):
            cause = (i + b) % 3
            if cause == 0:
                feat[b, (i * 7) % D, y, x] = np.nan if i % 2 else np.inf
            elif cause == 1:
                feat[b, :, y, x] = 0.0
            else:
                cover[b, y, x] = 0
    return np.broadcast_to(dead, (Bs, Hs, Ws))


def int_case(shape, kind, seed=0):
    """(feat [Bs, 96, Hs, Ws] fp32, cover int32, dead [Bs, Hs, Ws]): small whole numbers, so that nothing but liveness decides"""
    rng = np.random.default_rng(seed)
    feat = rng.integers(1, 4, size=(INT_BS, D) + tuple(shape)).astype(np.float32)
    cover = np.ones((INT_BS,) + tuple(shape), dtype=np.int32)
    dead = kill(feat, cover, kind)
    return feat, cover, dead


def fields(shape, n_fields, rng):
    """a label map [Bs, Hs, Ws] of blocky homogeneous fields"""
    Bs, Hs, Ws = shape
    by, bx = max(1, Hs // 3), max(1, Ws // 4)
    grid = rng.integers(0, n_fields, size=(Bs, Hs // by + 1, Ws // bx + 1))
    return np.repeat(np.repeat(grid, by, axis=1), bx, axis=2)[:, :Hs, :Ws]


def real_features(shape, form, seed):
    """(feat fp32, cover, labels): planted fields -- a prototype per field plus small noise, a third of the pixels the bare prototype
    (cos exactly 1 in float64), raw features near 50 or unit vectors; a few dead pixels of each cause"""
    rng = np.random.default_rng(seed)
    lab = fields(shape, 6, rng)
    proto = rng.normal(size=(6, D)) + 3.0
    f = proto[lab].transpose(0, 3, 1, 2)
    noise = rng.normal(size=f.shape) * 0.15 * (rng.random(lab.shape) > 0.33)[:, None]
    f = (f + noise) * (12.0 if form == "raw" else 1.0)
    if form == "normalized":
        f = f / np.sqrt((f * f).sum(axis=1, keepdims=True))
    feat = f.astype(np.float32)
    cover = np.ones(shape, dtype=np.int32)
    kill(feat, cover, "corner")
    feat[:, :, 3, 5] = 0.0
    cover[:, 7, 20] = 0
    return feat, cover, lab


def real_scores(lab, nc, unary, seed, sharp=6.0):
    """score maps [Bs, nc, Hs, Ws] fp32 over a label map: a sharp peak at the (noisy) label plus noise; one class -inf on a stripe,
    NaN scores on two pixels, a pixel with every score -inf"""
    rng = np.random.default_rng(seed)
    Bs, Hs, Ws = lab.shape
    noisy = np.where(rng.random(lab.shape) < 0.15, rng.integers(0, nc, size=lab.shape), lab % nc)
    s = rng.normal(size=(Bs, nc, Hs, Ws)) + sharp * (np.arange(nc)[None, :, None, None] == noisy[:, None])
    if unary == "votes":
        s = np.exp(s - s.max(axis=1, keepdims=True))
        s = np.where(s < 1e-3, 0.0, s)                          # classes without a vote
    elif nc > 1:
        s[:, nc - 1, :, Ws // 2:] = -np.inf                     # a class without rows
    s = s.astype(np.float32)
    s[0, 0, 1, 1] = np.nan
    s[-1, nc - 1, Hs - 2, Ws - 3] = np.nan
    if unary == "logits":
        s[0, :, 4, 2] = -np.inf
    return s


def dense_weights(feat, cover, R):
    """(k fp32, live): the float64 affinity rounded once, its zeros (a dead end, a neighbour outside the scene) replaced by 0.5 -- the
    step takes k as it is, and must skip those neighbours by its own test, not lean on a zero weight"""
    a, s, g = tables(R)
    k, live = affinity(feat, cover, R, a, s, g)
    return np.where(k == 0, 0.5, k).astype(np.float32), live


def step_case(nc, R, unary, shape=STEP_SHAPE, seed=11):
    """(scores fp32, k fp32, live_aff, q_in fp32): k from the float64 affinity rounded once -- an INPUT of the step, to the kernel and to
    the restatement alike; q_in = the restatement's Q_0 rounded"""
    feat, cover, lab = real_features(shape, "normalized", seed + R)
    k, live = dense_weights(feat, cover, R)
    scores = real_scores(lab, nc, unary, seed + 100 + nc)
    lv = live_refine(live, scores)
    q0 = step(unaries(scores, unary, 1.0), lv, k, None, R).astype(np.float32)
    return scores, k, live, q0


def refine_case(nc, R, unary, seed=23):
    feat, cover, lab = real_features(REFINE_SHAPE, "normalized", seed + R)
    k, live = dense_weights(feat, cover, R)
    return real_scores(lab, nc, unary, seed + 100 + nc), k, live


# -------------------------------------------------------------------------------------------------------------------- the bars
def measured():
    """the committed measurements by case, or None while the file does not exist (a run then measures and asserts no bar)"""
    if not os.path.exists(PARITY_FILE):
        return None
    out = {}
    with open(PARITY_FILE) as f:
        for line in f:
            if line.strip():
                row = json.loads(line)
                out[row["case"]] = row["measured"]
    return out


def bars(case):
    """4 x the committed measurement per quantity (the project's convention); None while nothing is committed, or -- in a measuring
    run (MSST_RECORD_DIR) only -- nothing for this case"""
    m = measured()
    if m is None:
        return None
    m = m.get(case)
    if m is None and os.environ.get("MSST_RECORD_DIR"):
        return None
    assert m, f"no committed measurement for {case} in {PARITY_FILE}"
    return {k: 4.0 * v for k, v in m.items()}


def note(case, err):
    """MSST_RECORD_DIR=<directory>: append a case's measured errors to crf_parity_dev.jsonl there, BEFORE the bars are asserted"""
    d = os.environ.get("MSST_RECORD_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "crf_parity_dev.jsonl"), "a") as f:
            f.write(json.dumps(dict(case=case, measured=err)) + "\n")


def check(case, err):
    """print and record, then assert the committed bars (where there are any)"""
    print(f"{case}: {err}")
    note(case, err)
    bar = bars(case)
    if bar is not None:
        assert set(bar) == set(err), (case, sorted(bar), sorted(err))
        over = [(q, e, bar[q]) for q, e in err.items() if not e <= bar[q]]
        assert over == [], (case, over)
    return bar


def rel_err(got, want):
    """the largest error over the largest value; NaN places must agree"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN places differ"
    ok = ~np.isnan(want)
    if not ok.any():
        return 0.0
    return float(np.abs(got[ok] - want[ok]).max() / max(np.abs(want[ok]).max(), 1e-300))
