"""A numpy restatement of maskedsst_amd/regions.py for the tests: connected-component labelling by flood fill from each unvisited live
pixel in raster order, and one merge round in both modes written PER REGION (a list of regions, their neighbour sets, one decision per
flagged region), so that it shares no structure with the per-pixel kernels.  `mutate` names a deliberate error; the host tests check
that every one of them shows on a committed case.  Also the maps the tests run on."""
import numpy as np

CROSS = ((0, -1), (-1, 0), (0, 1), (1, 0))
SQUARE = CROSS + ((-1, -1), (-1, 1), (1, -1), (1, 1))
LABEL_MUTANTS = ("conn8_for_4", "row_wrap", "scene_leak", "dead_bridge", "foreground_only", "root_largest")
MERGE_MUTANTS = ("size_le", "flagged_target", "ties_highest", "sequential", "no_cell_box", "keep_lowest_root")
TILE = 16          # maskedsst_amd/csrc/msst_regions.hip: RG_T


def offsets(connectivity):
    assert connectivity in (4, 8)
    return CROSS if connectivity == 4 else SQUARE


def grid(Hs, Ws, S):
    return -(-Hs // S), -(-Ws // S)


# --------------------------------------------------------------------------------------------------------------------- labelling
def _neighbours(values, b, y, x, offs, mutate):
    Bs, Hs, Ws = values.shape
    for dy, dx in offs:
        ny, nx = y + dy, x + dx
        if 0 <= ny < Hs and 0 <= nx < Ws:
            yield b, ny, nx
            if mutate == "dead_bridge" and values[b, ny, nx] < 0 and dy * dx == 0 and 0 <= ny + dy < Hs and 0 <= nx + dx < Ws:
                yield b, ny + dy, nx + dx
        elif mutate == "scene_leak" and 0 <= nx < Ws and ny == Hs and b + 1 < Bs:
            yield b + 1, 0, nx
        elif mutate == "scene_leak" and 0 <= nx < Ws and ny == -1 and b > 0:
            yield b - 1, Hs - 1, nx
    if mutate == "row_wrap":
        for i in (y * Ws + x - 1, y * Ws + x + 1):
            if 0 <= i < Hs * Ws:
                yield b, i // Ws, i % Ws


def label(values, connectivity=4, mutate=None):
    """(labels int64 [Bs, Hs, Ws]: the root y0 Ws + x0 of the pixel's region, -1 dead; sizes int32: the pixel count at the root, 0
    elsewhere; count int32 [Bs])"""
    values = np.asarray(values)
    Bs, Hs, Ws = values.shape
    offs = offsets(8 if mutate == "conn8_for_4" else connectivity)
    labels = np.full(values.shape, -1, dtype=np.int64)
    sizes = np.zeros(values.shape, dtype=np.int32)
    count = np.zeros(Bs, dtype=np.int32)
    seen = values < 0
    for b in range(Bs):
        for y in range(Hs):
            for x in range(Ws):
                if seen[b, y, x]:
                    continue
                v = values[b, y, x]
                seen[b, y, x] = True
                stack, members = [(b, y, x)], []
                while stack:
                    cur = stack.pop()
                    members.append(cur)
                    for nb in _neighbours(values, *cur, offs, mutate):
                        if not seen[nb] and (values[nb] == v or mutate == "foreground_only"):
                            seen[nb] = True
                            stack.append(nb)
                root = y * Ws + x                      # the scan is in raster order: the first pixel met is the smallest index
                if mutate == "root_largest":
                    root = max(my * Ws + mx for mb, my, mx in members if mb == b)
                for m in members:
                    labels[m] = root
                sizes[b, root // Ws, root % Ws] = len(members)
                count[b] += 1
    return labels, sizes, count


def label_pairwise(values, connectivity=4):
    """a second labelling that shares nothing with the flood fill: every pixel starts with its own index, and every pair of neighbours
    of equal live value takes the smaller of its two labels until nothing moves.  For tiny maps."""
    values = np.asarray(values)
    Bs, Hs, Ws = values.shape
    labels = np.where(values >= 0, np.arange(Hs * Ws, dtype=np.int64).reshape(1, Hs, Ws), -1)
    moved = True
    while moved:
        moved = False
        for b in range(Bs):
            for y in range(Hs):
                for x in range(Ws):
                    for dy, dx in offsets(connectivity):
                        ny, nx = y + dy, x + dx
                        if 0 <= ny < Hs and 0 <= nx < Ws and values[b, y, x] >= 0 and values[b, y, x] == values[b, ny, nx] \
                                and labels[b, ny, nx] < labels[b, y, x]:
                            labels[b, y, x] = labels[b, ny, nx]
                            moved = True
    return labels


def ids_of(labels):
    """dense ids per scene by ascending root, -1 dead; n per scene"""
    ids = np.full(labels.shape, -1, dtype=np.int64)
    n = np.zeros(labels.shape[0], dtype=np.int64)
    for b in range(labels.shape[0]):
        roots = np.unique(labels[b][labels[b] >= 0])
        n[b] = len(roots)
        for k, r in enumerate(roots):
            ids[b][labels[b] == r] = k
    return ids, n


# ------------------------------------------------------------------------------------------------------------------ one merge round
def _pairs(lab, dy, dx):
    H, W = lab.shape
    a = lab[max(0, -dy):H - max(0, dy), max(0, -dx):W - max(0, dx)]
    b = lab[max(0, dy):H - max(0, -dy), max(0, dx):W - max(0, -dx)]
    return a.ravel(), b.ravel()


class Region:
    def __init__(self, root, value, pix):
        self.root, self.value, self.pix, self.size = int(root), int(value), pix, len(pix)
        self.near = set()
        self.flagged = False


def regions_of(values, connectivity):
    """the regions of ONE scene [Hs, Ws], dead ones left out: {root: Region}, with their neighbour sets under connectivity"""
    Hs, Ws = values.shape
    lab = label(values[None], connectivity)[0][0]
    regs = {}
    order = np.argsort(lab.ravel(), kind="stable")
    flat = lab.ravel()[order]
    starts = np.flatnonzero(np.r_[True, flat[1:] != flat[:-1]])
    for s, e in zip(starts, np.r_[starts[1:], len(flat)]):
        if flat[s] >= 0:
            idx = order[s:e]
            regs[int(flat[s])] = Region(flat[s], values.ravel()[flat[s]], np.stack([idx // Ws, idx % Ws], axis=1))
    for dy, dx in offsets(connectivity):
        a, b = _pairs(lab, dy, dx)
        m = (a >= 0) & (b >= 0) & (a != b)
        for r, t in set(zip(a[m].tolist(), b[m].tolist())):
            regs[r].near.add(t)
    return regs


def _flag(regs, mode, min_size, n_sp, mutate):
    live = {r: (mode == 0 or g.value < n_sp) for r, g in regs.items()}
    if mode == 0:
        for g in regs.values():
            g.flagged = g.size <= min_size if mutate == "size_le" else g.size < min_size
    else:
        by_id = {}
        for r, g in regs.items():
            if live[r]:
                by_id.setdefault(g.value, []).append(g)
        for pieces in by_id.values():
            kept = min(pieces, key=(lambda g: g.root) if mutate == "keep_lowest_root" else (lambda g: (-g.size, g.root)))
            for g in pieces:
                g.flagged = g is not kept
    return live


def _winner(g, regs, live, mode, S, gx, mutate):
    cands = []
    for t in g.near:
        T = regs[t]
        if not live[t] or (T.flagged and mutate != "flagged_target"):
            continue
        if mode == 1 and mutate != "no_cell_box":
            i0, j0 = (g.pix // S).min(axis=0)
            i1, j1 = (g.pix // S).max(axis=0)
            im, jm = T.value // gx, T.value % gx
            if not (im - 1 <= i0 and i1 <= im + 1 and jm - 1 <= j0 and j1 <= jm + 1):
                continue
        cands.append(T)
    if not cands:
        return None
    return max(cands, key=(lambda T: (T.size, T.root)) if mutate == "ties_highest" else (lambda T: (T.size, -T.root)))


def merge_round(values, connectivity=4, mode=0, min_size=1, step=8, mutate=None):
    """one simultaneous round: (values_out, history [4]: live regions, flagged, merged, changed pixels, summed over the batch)"""
    values = np.asarray(values)
    Bs, Hs, Ws = values.shape
    gy, gx = grid(Hs, Ws, step)
    out = values.copy()
    hist = np.zeros(4, dtype=np.int64)
    for b in range(Bs):
        regs = regions_of(values[b], connectivity)
        live = _flag(regs, mode, min_size, gy * gx, mutate)
        hist[0] += sum(live.values())
        hist[1] += sum(1 for r, g in regs.items() if live[r] and g.flagged)
        if mutate == "sequential":
            cur = values[b].copy()
            for r in sorted(r for r, g in regs.items() if live[r] and g.flagged):
                now = regions_of(cur, connectivity)
                live_now = _flag(now, mode, min_size, gy * gx, None)
                g = next(q for q in now.values() if (q.pix == (r // Ws, r % Ws)).all(axis=1).any())
                T = _winner(g, now, live_now, mode, step, gx, None) if g.flagged else None
                if T is not None:
                    cur[g.pix[:, 0], g.pix[:, 1]] = T.value
                    hist[2] += 1
            hist[3] += int((cur != values[b]).sum())
            out[b] = cur
            continue
        for r in sorted(regs):
            g = regs[r]
            if not live[r] or not g.flagged:
                continue
            T = _winner(g, regs, live, mode, step, gx, mutate)
            if T is not None:
                out[b, g.pix[:, 0], g.pix[:, 1]] = T.value
                hist[2] += 1
                hist[3] += g.size if T.value != g.value else 0
    return out, hist


def rounds(values, connectivity, n, mode=0, min_size=1, step=8):
    """n x (label, merge): (values, history [n, 4])"""
    hist = np.zeros((n, 4), dtype=np.int64)
    for t in range(n):
        values, hist[t] = merge_round(values, connectivity, mode, min_size, step)
    return values, hist


def fragments(labels, connectivity, step):
    """per scene: the pieces of the live ids beyond one per id"""
    Bs, Hs, Ws = labels.shape
    gy, gx = grid(Hs, Ws, step)
    n = 0
    for b in range(Bs):
        regs = [g for g in regions_of(labels[b], connectivity).values() if g.value < gy * gx]
        n += len(regs) - len({g.value for g in regs})
    return n


# --------------------------------------------------------------------------------------------------------------------------- maps
PATTERNS = ("one", "dead", "corners", "dead_row", "dead_tile", "checker", "serpentine", "spiral", "rings", "diagonal", "random3")


def spiral(Hs, Ws):
    g = np.zeros((Hs, Ws), dtype=np.int64)
    y = x = 0
    dy, dx = 0, 1
    g[0, 0] = 1

    def inside(a, b):
        return 0 <= a < Hs and 0 <= b < Ws

    while True:
        for _ in range(2):
            ny, nx = y + dy, x + dx
            if inside(ny, nx) and g[ny, nx] == 0 and not (inside(ny + dy, nx + dx) and g[ny + dy, nx + dx] == 1):
                y, x = ny, nx
                g[y, x] = 1
                break
            dy, dx = dx, -dy
        else:
            return g


def pattern(name, Hs, Ws, seed=0):
    """one scene [Hs, Ws] int64"""
    ys, xs = np.mgrid[0:Hs, 0:Ws]
    rnd = np.random.default_rng(1000 * Hs + Ws + seed).integers(0, 3, size=(Hs, Ws)).astype(np.int64)
    if name == "one":
        return np.full((Hs, Ws), 5, dtype=np.int64)
    if name == "dead":
        return np.where(rnd == 0, -1, -2).astype(np.int64)
    if name == "corners":
        rnd[0, 0] = rnd[0, -1] = rnd[-1, 0] = rnd[-1, -1] = -1
        return rnd
    if name == "dead_row":
        v = np.full((Hs, Ws), 2, dtype=np.int64)
        v[Hs // 2] = -1
        return v
    if name == "dead_tile":
        rnd[:TILE, :TILE] = -2
        return rnd
    if name == "checker":
        return ((ys + xs) % 2).astype(np.int64)
    if name == "serpentine":
        v = np.zeros((Hs, Ws), dtype=np.int64)
        v[0::2] = 1
        v[1::4, -1] = 1
        v[3::4, 0] = 1
        return v
    if name == "spiral":
        return spiral(Hs, Ws)
    if name == "rings":
        return (np.minimum(np.minimum(ys, xs), np.minimum(Hs - 1 - ys, Ws - 1 - xs)) % 3).astype(np.int64)
    if name == "diagonal":
        return ((ys + xs) % 3).astype(np.int64)
    if name == "random3":
        return rnd
    raise KeyError(name)


def salt_blobs(Hs, Ws, classes=4, seed=0, salt=0.05):
    """smooth blobs (the nearest of a few planted points) with salt-and-pepper pixels and a few dead ones: what a sieve is for"""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(0, 1, size=(3 * classes, 2)) * (Hs, Ws)
    ys, xs = np.mgrid[0:Hs, 0:Ws]
    d = (ys[..., None] - pts[:, 0]) ** 2 + (xs[..., None] - pts[:, 1]) ** 2
    v = (np.argmin(d, axis=2) % classes).astype(np.int64)
    m = rng.uniform(size=(Hs, Ws)) < salt
    v[m] = rng.integers(0, classes, size=int(m.sum()))
    v[rng.uniform(size=(Hs, Ws)) < 0.01] = -1
    v[rng.uniform(size=(Hs, Ws)) < 0.005] = -2
    return v


def home(Hs, Ws, S):
    gy, gx = grid(Hs, Ws, S)
    ys, xs = np.mgrid[0:Hs, 0:Ws]
    return ((ys // S) * gx + xs // S).astype(np.int64)


def fragment_maps():
    """hand-built superpixel label maps [Bs, Hs, Ws] at step 4 (16 x 16: 4 x 4 cells): (name, map)"""
    maps = []
    # an orphan piece of id 0 inside cell (1, 1), next to id 5 (eligible), id 15 planted beside it (ineligible: cell (3, 3))
    v = home(16, 16, 4)
    v[5, 5] = 0
    v[5, 6] = 15
    v[6, 5] = 15
    maps.append(("orphan", v))
    # two pieces of id 5 of equal size: the lower root is kept, the other goes to its largest neighbour
    v = home(16, 16, 4)
    v[4:8, 4:8] = 6
    v[4:6, 4] = 5
    v[6:8, 7] = 5
    maps.append(("equal_pieces", v))
    # an id >= n_sp and dead pixels: both stay, neither is a target
    v = home(16, 16, 4)
    v[9, 9] = 16
    v[9, 10] = 2
    v[10, 9] = -1
    v[10, 10] = 99
    v[2, 2] = 5
    maps.append(("out_of_range", v))
    # a piece that spans two cells: only ids around both cells are eligible
    v = home(16, 16, 4)
    v[8, 2:7] = 0
    maps.append(("wide_piece", v))
    # an orphan of id 0 in cell (1, 1) between the kept piece of id 15 (8 pixels, the larger, not eligible) and id 5 (7 pixels, eligible)
    v = home(16, 16, 4)
    v[4:8, 6:8] = 15
    v[12:16, 12:16] = 11
    v[15, 15] = 15
    v[5, 5] = 0
    maps.append(("ineligible_larger", v))
    # an orphan whose only neighbours are other orphans: waits a round
    v = home(16, 16, 4)
    v[5:8, 5:8] = 0
    v[6, 6] = 10
    maps.append(("nested", v))
    return maps


def sieve_maps():
    """hand-built class maps [Hs, Ws] with the min_size that makes their point: (name, map, min_size)"""
    maps = []
    v = np.full((12, 20), 3, dtype=np.int64)                          # isolated pixels in a field
    v[2, 3] = v[5, 17] = v[11, 0] = v[0, 19] = 1
    v[7, 7] = 2
    maps.append(("isolated", v, 2))
    v = np.zeros((9, 18), dtype=np.int64)                              # a patch between two fields of equal size: the lowest root wins
    v[:, 9:] = 1
    v[4, 8] = 2
    v[4, 9] = 2
    maps.append(("tie", v, 3))
    v = np.zeros((9, 9), dtype=np.int64)                               # a patch whose only neighbours are small patches: waits a round
    v[3:6, 3:6] = 1
    v[4, 4] = 2
    maps.append(("waits", v, 10))
    v = np.zeros((9, 9), dtype=np.int64)                               # a patch enclosed by dead pixels stays; -2 is preserved
    v[2:7, 2:7] = -2
    v[3:6, 3:6] = -1
    v[4, 4] = 7
    maps.append(("enclosed", v, 4))
    v = np.zeros((6, 40), dtype=np.int64)                              # across the tile border, and 8 against 4: a diagonal contact
    v[:, 20:] = 4
    v[2, 15:18] = 9
    v[3, 18] = 9
    v[1, 14] = 9
    maps.append(("diagonal_contact", v, 6))
    return maps
