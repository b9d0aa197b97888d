"""Float64 numpy restatement of the SLIC superpixels and the object-based class maps (maskedsst_amd/superpixel.py, msst_slic_assign,
msst_slic_update, msst_slic_pool, msst_slic_pool_finish, msst_slic_broadcast), the case generators of tests/test_gpu_slic.py and the bars
(profiles/slic_parity_measured.jsonl: 4 x the error measured on the MI355X).  Written with gathers over the nine candidate cells --
no tiles, no windows, none of the product's code paths -- and checked against a plain per-pixel loop (tests/test_slic_host.py).  Nothing
here needs a GPU.

The mutants are restatements with one rule broken; tests/test_slic_host.py checks that the bars still tell each from the true one."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY_FILE = os.path.join(ROOT, "profiles", "slic_parity_measured.jsonl")
D = 96
MARGIN_SHARE = 0.01       # the share of live pixels a case may leave under the margin
MUTANTS = ["plus_candidates", "dead_centre_candidate", "ties_highest", "no_bias", "compactness_not_squared", "absolute_position",
           "empty_zeroed", "sum_not_divided", "dead_pixel_counted", "pool_across_scenes"]

# ---- the exact cases
INT_SHAPES = [(1, 1), (7, 9), (8, 8), (9, 17), (17, 33)]
INT_STEPS = [4, 8, 16]
INT_BS = 3
DEAD_KINDS = ["none", "corner", "row", "cell", "all"]
POOL_CHANNELS = [1, 2, 17, 128]
# ---- the real-valued cases: (Hs, Ws, S)
REAL_CASES = [(19, 27, 4), (33, 41, 8), (35, 50, 16)]
REAL_BS = 2
REAL_ITERS = 8
REAL_COMPACTNESS = 0.2
FAR = 32000               # where the absolute_position mutant places the scene's window inside a larger scene


def grid(Hs, Ws, S):
    return (Hs + S - 1) // S, (Ws + S - 1) // S


def hl_of(compactness, S, mutate=None):
    r = compactness / S
    return float(np.float32(0.5 * (r if mutate == "compactness_not_squared" else r * r)))


def live_map(feat, cover=None):
    live = np.isfinite(feat.astype(np.float64)).all(axis=1)
    if cover is not None:
        live &= cover > 0
    return live


def cells(Hs, Ws, S):
    """(pi [Hs, Ws], pj [Hs, Ws]): the cell of every pixel"""
    return np.broadcast_to((np.arange(Hs) // S)[:, None], (Hs, Ws)), np.broadcast_to((np.arange(Ws) // S)[None, :], (Hs, Ws))


def home_labels(live, S):
    Bs, Hs, Ws = live.shape
    pi, pj = cells(Hs, Ws, S)
    return np.where(live, pi * grid(Hs, Ws, S)[1] + pj, -1).astype(np.int64)


def new_centres(Bs, n_sp):
    return dict(cent=np.zeros((Bs, n_sp, D)), off=np.zeros((Bs, n_sp, 2)), bias=np.zeros((Bs, n_sp)), counts=np.zeros((Bs, n_sp), dtype=np.int64))


def candidate_offsets(mutate=None):
    """(di, dj) ascending: the order of the superpixel ids"""
    r = (-1, 0, 1)
    return [(di, dj) for di in r for dj in r if mutate != "plus_candidates" or di == 0 or dj == 0]


def candidate_scores(feat, live, cen, S, hl, mutate=None):
    """(ids [K, Bs, Hs, Ws] int64, -1 where there is no such candidate; scores [K, Bs, Hs, Ws] float64, -inf there), candidates in id order"""
    Bs, _, Hs, Ws = feat.shape
    gy, gx = grid(Hs, Ws, S)
    f = np.where(live[:, None], feat.astype(np.float64), 0.0).transpose(0, 2, 3, 1)
    pi, pj = cells(Hs, Ws, S)
    yy, xx = np.broadcast_to(np.arange(Hs)[:, None], (Hs, Ws)), np.broadcast_to(np.arange(Ws)[None, :], (Hs, Ws))
    cent, off, bias, counts = (np.asarray(cen[k], dtype=np.float64 if k != "counts" else np.int64) for k in ("cent", "off", "bias", "counts"))
    ids, scores = [], []
    bidx = np.arange(Bs)[:, None, None]
    for di, dj in candidate_offsets(mutate):
        ci, cj = pi + di, pj + dj
        inside = (ci >= 0) & (ci < gy) & (cj >= 0) & (cj < gx)
        k = np.where(inside, ci * gx + cj, 0)
        kb = np.broadcast_to(k, (Bs, Hs, Ws))
        ok = inside[None] & live
        if mutate != "dead_centre_candidate":
            ok = ok & (counts[bidx, kb] > 0)
        if mutate == "absolute_position":                        # the centre's place as an absolute fp32 number inside a larger scene
            py = (np.float32(FAR + ci * S)[None] + off[bidx, kb, 0].astype(np.float32)).astype(np.float32)
            px = (np.float32(FAR + cj * S)[None] + off[bidx, kb, 1].astype(np.float32)).astype(np.float32)
            dy = (np.float32(FAR + yy)[None] - py).astype(np.float64)
            dx = (np.float32(FAR + xx)[None] - px).astype(np.float64)
        else:
            dy = (yy - ci * S)[None] - off[bidx, kb, 0]
            dx = (xx - cj * S)[None] - off[bidx, kb, 1]
        s = (f * cent[bidx, kb]).sum(axis=-1) - hl * (dy * dy + dx * dx)
        if mutate != "no_bias":
            s = s + bias[bidx, kb]
        ids.append(np.where(ok, kb, -1))
        scores.append(np.where(ok, s, -np.inf))
    return np.stack(ids), np.stack(scores)


def assign(feat, cover, cen, S, hl, mutate=None):
    """(labels [Bs, Hs, Ws] int64, best score float64 (NaN where -1), top-two margin (inf where -1 or with one candidate))"""
    live = live_map(feat, cover)
    ids, sc = candidate_scores(feat, live, cen, S, hl, mutate)
    K = sc.shape[0]
    pick = K - 1 - np.argmax(sc[::-1], axis=0) if mutate == "ties_highest" else np.argmax(sc, axis=0)
    best = np.take_along_axis(sc, pick[None], axis=0)[0]
    lab = np.take_along_axis(ids, pick[None], axis=0)[0]
    has = np.isfinite(best) | (best == np.inf)
    assert not (live & ~has).any(), "a live pixel without a candidate: its own centre must have rows"
    srt = np.sort(sc, axis=0)
    with np.errstate(invalid="ignore"):
        gap = np.where(np.isfinite(srt[-2]), srt[-1] - srt[-2], np.inf) if K > 1 else np.full(best.shape, np.inf)
    return np.where(has, lab, -1).astype(np.int64), np.where(has, best, np.nan), np.where(has, gap, np.inf)


def update(feat, cover, labels, S, prev, mutate=None):
    """the centres from the labels; `prev` (new_centres or the centres before) is what an empty centre keeps"""
    Bs, _, Hs, Ws = feat.shape
    gy, gx = grid(Hs, Ws, S)
    n_sp = gy * gx
    live = live_map(feat, cover)
    f = np.where(live[:, None], feat.astype(np.float64), 0.0).transpose(0, 2, 3, 1)
    yy, xx = np.broadcast_to(np.arange(Hs)[:, None], (Hs, Ws)), np.broadcast_to(np.arange(Ws)[None, :], (Hs, Ws))
    out = {k: np.array(v, dtype=np.float64 if k != "counts" else np.int64) for k, v in prev.items()}
    for b in range(Bs):
        lab = labels[b].copy()
        if mutate == "dead_pixel_counted":
            pi, pj = cells(Hs, Ws, S)
            lab = np.where(lab < 0, pi * gx + pj, lab)
        m = lab >= 0
        cnt = np.bincount(lab[m], minlength=n_sp)
        fs = np.zeros((n_sp, D))
        np.add.at(fs, lab[m], f[b][m])
        oy = np.bincount(lab[m], weights=(yy[m] - (lab[m] // gx) * S).astype(np.float64), minlength=n_sp)
        ox = np.bincount(lab[m], weights=(xx[m] - (lab[m] % gx) * S).astype(np.float64), minlength=n_sp)
        has = cnt > 0
        div = np.where(has, cnt, 1)[:, None] if mutate != "sum_not_divided" else 1.0
        c = fs / div
        out["cent"][b] = np.where(has[:, None], c, 0.0 if mutate == "empty_zeroed" else out["cent"][b])
        out["off"][b] = np.where(has[:, None], np.stack([oy, ox], axis=1) / np.where(has, cnt, 1)[:, None],
                                 0.0 if mutate == "empty_zeroed" else out["off"][b])
        out["bias"][b] = np.where(has, -0.5 * (c * c).sum(axis=1), 0.0 if mutate == "empty_zeroed" else out["bias"][b])
        out["counts"][b] = cnt
    return out


def fit(feat, cover, S, compactness, iters, mutate=None):
    """(labels, centres, history [iters, 2], every (labels, centres) by iteration)"""
    Bs, _, Hs, Ws = feat.shape
    gy, gx = grid(Hs, Ws, S)
    hl = hl_of(compactness, S, mutate)
    labels = home_labels(live_map(feat, cover), S)
    cen = update(feat, cover, labels, S, new_centres(Bs, gy * gx), mutate)
    trace, hist = [(labels, cen)], []
    for _ in range(iters):
        new, _, _ = assign(feat, cover, cen, S, hl, mutate)
        cen = update(feat, cover, new, S, cen, mutate)
        hist.append((int((new != labels).sum()), int((cen["counts"] == 0).sum())))
        labels = new
        trace.append((labels, cen))
    return labels, cen, np.array(hist, dtype=np.int64).reshape(iters, 2), trace


def positions(cen, Hs, Ws, S):
    gy, gx = grid(Hs, Ws, S)
    org = np.stack(np.meshgrid(np.arange(gy) * S, np.arange(gx) * S, indexing="ij"), axis=-1).reshape(1, gy * gx, 2)
    return cen["off"] + org


def pool(maps, labels, n_sp, mutate=None):
    """(table [Bs, n_sp, C] float64, NaN for an empty superpixel; region classes [Bs, n_sp], -1 there; classes [Bs, Hs, Ws])"""
    Bs, C, Hs, Ws = maps.shape
    table = np.full((Bs, n_sp, C), np.nan)
    m64 = maps.astype(np.float64)
    for b in range(Bs):
        src = range(Bs) if mutate == "pool_across_scenes" else [b]
        for k in range(n_sp):
            rows = [m64[s][:, labels[s] == k].T for s in src]
            rows = np.concatenate(rows, axis=0)
            if len(rows):
                with np.errstate(invalid="ignore"):
                    table[b, k] = rows.sum(axis=0) / len(rows)
    ok = np.where(np.isnan(table), -np.inf, table)
    region = np.where((ok > -np.inf).any(axis=2), np.argmax(ok, axis=2), -1).astype(np.int64)
    classes = np.where(labels >= 0, np.take_along_axis(region, np.maximum(labels, 0).reshape(Bs, -1), axis=1).reshape(labels.shape), -1)
    return table, region, classes.astype(np.int64)


# ------------------------------------------------------------------------------------------------------------- the plain loops
def assign_loops(feat, cover, cen, S, hl):
    Bs, _, Hs, Ws = feat.shape
    gy, gx = grid(Hs, Ws, S)
    lab = np.full((Bs, Hs, Ws), -1, dtype=np.int64)
    best = np.full((Bs, Hs, Ws), np.nan)
    for b in range(Bs):
        for y in range(Hs):
            for x in range(Ws):
                v = feat[b, :, y, x].astype(np.float64)
                if not np.isfinite(v).all() or (cover is not None and cover[b, y, x] <= 0):
                    continue
                top = None
                for ci in range(y // S - 1, y // S + 2):
                    for cj in range(x // S - 1, x // S + 2):
                        if not (0 <= ci < gy and 0 <= cj < gx) or cen["counts"][b, ci * gx + cj] <= 0:
                            continue
                        k = ci * gx + cj
                        py, px = ci * S + cen["off"][b, k, 0], cj * S + cen["off"][b, k, 1]
                        s = float(v @ cen["cent"][b, k]) + cen["bias"][b, k] - hl * ((y - py) ** 2 + (x - px) ** 2)
                        if top is None or s > top[0]:
                            top = (s, k)
                if top is not None:
                    best[b, y, x], lab[b, y, x] = top
    return lab, best


def update_loops(feat, cover, labels, S, prev):
    Bs, _, Hs, Ws = feat.shape
    gy, gx = grid(Hs, Ws, S)
    out = {k: np.array(v, dtype=np.float64 if k != "counts" else np.int64) for k, v in prev.items()}
    for b in range(Bs):
        for k in range(gy * gx):
            px = [(y, x) for y in range(Hs) for x in range(Ws) if labels[b, y, x] == k]
            out["counts"][b, k] = len(px)
            if px:
                c = sum(feat[b, :, y, x].astype(np.float64) for y, x in px) / len(px)
                out["cent"][b, k] = c
                out["off"][b, k] = [sum(y for y, _ in px) / len(px) - (k // gx) * S, sum(x for _, x in px) / len(px) - (k % gx) * S]
                out["bias"][b, k] = -0.5 * float(c @ c)
    return out


# ------------------------------------------------------------------------------------------------------------------- the cases
def kill(feat, cover, kind, S):
    """dead pixels in every scene of a map, the cause cycling NaN / inf features and cover == 0 by pixel"""
    Bs, _, Hs, Ws = feat.shape
    dead = np.zeros((Hs, Ws), dtype=bool)
    if kind == "corner":
        dead[0, 0] = dead[-1, -1] = True
    elif kind == "row":
        dead[Hs // 2] = True
    elif kind == "cell":
        gy, gx = grid(Hs, Ws, S)
        i, j = (gy - 1) // 2, (gx - 1) // 2
        dead[i * S:(i + 1) * S, j * S:(j + 1) * S] = True
    elif kind == "all":
        dead[:] = True
    ys, xs = np.nonzero(dead)
    for n, (y, x) in enumerate(zip(ys, xs)):
        for b in range(Bs):
            cause = (n + b) % 3
            if cause == 0:
                feat[b, (n * 7) % D, y, x] = np.nan
            elif cause == 1:
                feat[b, (n * 5) % D, y, x] = np.inf if n % 2 else -np.inf
            else:
                cover[b, y, x] = 0
    return np.broadcast_to(dead, (Bs, Hs, Ws))


def int_case(shape, S, kind, seed=0):
    """(feat fp32, cover int32, dead, centres, hl, prev_labels): whole-number features in [-3, 3] drawn from a few prototypes, GIVEN
    whole-number centroids with duplicates among them, offsets that are multiples of 0.5, compactness = S / 2 (hl = 0.125) -- every
    score is exact in fp32, ties included.  Some centres have count 0 and a centroid that would win: they must never be chosen."""
    rng = np.random.default_rng(1000 * S + 10 * shape[0] + shape[1] + seed)
    Hs, Ws = shape
    gy, gx = grid(Hs, Ws, S)
    n_sp = gy * gx
    protos = rng.integers(-3, 4, size=(4, D)).astype(np.float32)
    feat = protos[rng.integers(0, 4, size=(INT_BS, Hs, Ws))].transpose(0, 3, 1, 2).copy()
    feat[:, :8] = rng.integers(-3, 4, size=(INT_BS, 8, Hs, Ws))
    feat[0] = protos[0][:, None, None]                                                 # scene 0 is flat: the place alone decides, every mean is whole
    cover = np.ones((INT_BS, Hs, Ws), dtype=np.int32)
    dead = kill(feat, cover, kind, S)
    cen = new_centres(INT_BS, n_sp)
    cen["cent"][:] = protos[rng.integers(0, 3, size=(INT_BS, n_sp))]                    # duplicates: ties by the feature term
    cen["off"][:] = (S - 1) / 2.0                                                      # the cell's middle: ties by the spatial term
    move = rng.random((INT_BS, n_sp)) < 0.3
    cen["off"][move] += rng.integers(-S, S + 1, size=(int(move.sum()), 2)) * 0.5
    cen["off"] = np.clip(cen["off"], -S, 2 * S - 0.5)
    cen["bias"] = -0.5 * (cen["cent"] ** 2).sum(axis=2)
    cen["counts"][:] = rng.integers(1, 9, size=(INT_BS, n_sp))
    if n_sp > 1:
        cen["counts"][rng.random((INT_BS, n_sp)) < 0.2] = 0
    pi, pj = cells(Hs, Ws, S)
    home = pi * gx + pj
    for b in range(INT_BS):                                                            # a live pixel's own centre has rows; a dead cell's has none
        alive = np.unique(home[~dead[b]])
        cen["counts"][b, alive] = np.maximum(cen["counts"][b, alive], 1)
        cen["counts"][b, np.setdiff1d(np.arange(n_sp), alive)] = 0
    prev = np.where(rng.random((INT_BS, Hs, Ws)) < 0.5, np.broadcast_to(home, (INT_BS, Hs, Ws)), -1).astype(np.int64)
    assert hl_of(S / 2.0, S) == 0.125
    return feat, cover, dead, cen, 0.125, prev


def int_maps(shape, C, seed=0):
    """whole-number score maps [INT_BS, C, Hs, Ws] fp32: values in [-2, 2] (many ties), channel C - 1 is -inf on the right half"""
    rng = np.random.default_rng(77 * C + shape[0] + shape[1] + seed)
    m = rng.integers(-2, 3, size=(INT_BS, C) + tuple(shape)).astype(np.float32)
    if C > 1:
        m[:, C - 1, :, shape[1] // 2:] = -np.inf
    return m


def real_case(case, seed=5):
    """(feat fp32, cover int32): planted Voronoi fields -- 7 unit prototypes, Gaussian noise 0.15, renormalised; two scenes; a dead
    3 x 5 corner, its cause cycling"""
    Hs, Ws, S = case
    rng = np.random.default_rng(seed + S)
    proto = rng.normal(size=(7, D))
    proto /= np.sqrt((proto * proto).sum(axis=1, keepdims=True))
    feat = np.empty((REAL_BS, D, Hs, Ws), dtype=np.float32)
    yy, xx = np.mgrid[0:Hs, 0:Ws]
    for b in range(REAL_BS):
        sites = rng.random((7, 2)) * (Hs, Ws)
        lab = np.argmin((yy[None] - sites[:, 0, None, None]) ** 2 + (xx[None] - sites[:, 1, None, None]) ** 2, axis=0)
        f = proto[lab] + rng.normal(size=(Hs, Ws, D)) * 0.15
        f /= np.sqrt((f * f).sum(axis=2, keepdims=True))
        feat[b] = f.transpose(2, 0, 1)
    cover = np.ones((REAL_BS, Hs, Ws), dtype=np.int32)
    for n, (y, x) in enumerate((y, x) for y in range(3) for x in range(5)):
        if n % 3 == 0:
            feat[:, n % D, y, x] = np.nan
        elif n % 3 == 1:
            cover[:, y, x] = 0
        else:
            feat[:, (3 * n) % D, y, x] = np.inf
    return feat, cover


def case_name(case):
    return f"fit_{case[0]}x{case[1]}_S{case[2]}"


def centres32(cen):
    """the centres as the device holds them: fp32 values (as float64 numbers)"""
    return dict(cent=cen["cent"].astype(np.float32).astype(np.float64), off=cen["off"].astype(np.float32).astype(np.float64),
                bias=cen["bias"].astype(np.float32).astype(np.float64), counts=cen["counts"].copy())


def teacher_forced(case, iters=REAL_ITERS, mutate=None, assign_mutate=None):
    """the float64 iteration with its centres rounded to fp32 after every update, as a teacher-forced device run would hand them over:
    per iteration (labels, best, margin, centres)"""
    Hs, Ws, S = case
    feat, cover = real_case(case)
    gy, gx = grid(Hs, Ws, S)
    hl = hl_of(REAL_COMPACTNESS, S, mutate)
    labels = home_labels(live_map(feat, cover), S)
    cen = centres32(update(feat, cover, labels, S, new_centres(REAL_BS, gy * gx), mutate))
    out = [(labels, None, None, cen)]
    for _ in range(iters):
        labels, best, gap = assign(feat, cover, cen, S, hl, assign_mutate or mutate)
        cen = centres32(update(feat, cover, labels, S, cen, mutate))
        out.append((labels, best, gap, cen))
    return out


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
    """MSST_RECORD_DIR=<directory>: append a case's measured errors to slic_parity_dev.jsonl there, BEFORE the bars are asserted"""
    d = os.environ.get("MSST_RECORD_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "slic_parity_dev.jsonl"), "a") as f:
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


def abs_err(got, want, where=None):
    """the largest absolute error; NaN places must agree"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if where is not None:
        got, want = got[where], want[where]
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN places differ"
    ok = ~np.isnan(want)
    return float(np.abs(got[ok] - want[ok]).max()) if ok.any() else 0.0
