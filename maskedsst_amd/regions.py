"""Connected regions of class maps: which pixels of a map hang together.  Connected-component labelling of an integer map on the
device, and one merge rule on top of it that serves two uses: the SIEVE (the minimum mapping unit of land-cover mapping, gdal_sieve: a
connected patch of a class with fewer than min_size pixels is merged into its largest neighbouring patch) and SLIC's CONNECTIVITY pass
(the orphan pieces of a superpixel are merged into a neighbouring superpixel).  It consumes what the other calls write: the [Bs, Hs,
Ws] int64 class maps of predict_scene, knn_predict_scene, probe_predict_scene, gaussian_predict_scene, cluster_scene, crf_refine and
superpixel_classify, and the label map of fit_superpixels.

    reg = label_regions(values, connectivity=4)          # Regions(labels, sizes, count, connectivity, error); no synchronisation
    ids, n = region_ids(reg)                             # dense ids [Bs, Hs, Ws] int64 per scene (-1 dead), n [Bs] int64
    res = sieve_classes(classes, min_size, connectivity=4, rounds=4)          # SieveResult(classes, regions, history)
    con = enforce_connectivity(superpixels, features=None, connectivity=4, rounds=4)   # ConnectedSuperpixels(superpixels, regions, history)

The contract:
    region      values is int64 [Bs, Hs, Ws]; a value < 0 is dead (-1 uncovered, -2 a Gaussian reject).  A region is a maximal set of
                live pixels of one scene with equal value, connected under `connectivity`: 4 (the cross) or 8 (the 3 x 3 square).
                Nothing crosses the scene border (the last pixel of a row and the first of the next are no neighbours); nothing passes
                between the scenes of a batch.
    labels      labels[b, y, x] = y0 Ws + x0 of the region's first pixel in raster order: the ROOT, the region's smallest linear index;
                -1 for a dead pixel.  sizes[b, y, x] (int32) = the region's pixel count at the root pixel, 0 everywhere else.  count[b]
                (int32) = the regions of scene b.  region_ids numbers the regions of a scene 0 .. n - 1 by ascending root.
    round       one merge round is SIMULTANEOUS: every decision is taken from the round's input.  A region is FLAGGED when its size is
                below min_size (sieve), or when it is not the kept piece of its superpixel id -- the piece of largest size, then lowest
                root (fragments; an id >= n_sp is treated as dead).  The candidates of a flagged region R are the live, unflagged
                regions T != R with a pixel next to a pixel of R under `connectivity`; for fragments only those whose id m is eligible:
                every cell (y // S, x // S) of R's pixels lies in the 3 x 3 cells around cell (m // gx, m % gx), so that a label stays
                in the 3 x 3 cells of its pixel and superpixel_pool and superpixel_classify stay valid on the result.  The winner is
                the candidate of largest size, then lowest root; every pixel of R takes its value.  A flagged region without a
                candidate keeps its value (a patch enclosed by dead pixels; a patch whose neighbours are all flagged waits a round).
                A dead pixel keeps its value: -1 stays -1, -2 stays -2.
    rounds      `rounds` times (label, merge), then one more label so that the returned regions describe the returned map.  history
                [rounds, 4] int64 on the CPU: live regions, flagged regions, merged regions and changed pixels of each round, summed
                over the batch.  After a round with 0 changed pixels every later round reproduces all outputs bit for bit.  ONE
                synchronisation, to read the history and the error word.
    error word  every device loop (the finds and unions of the labelling) follows strictly decreasing indices and so terminates; each
                still counts its turns against a cap derived from Hs Ws, and a loop that reaches it stops and raises an error word in
                device memory.  sieve_classes and enforce_connectivity read the word with the history and raise RuntimeError;
                label_regions does not synchronise and returns the word as Regions.error (int32 [1] on the device; check_regions reads
                it).  A bug shows as an error, never as a hung GPU.

Everything is integer arithmetic with integer atomics, and the root is the region's smallest index whatever order the atomics land in:
every output has the same bits in every call, and the same bits for a scene alone or inside a batch.  min_size = 1 or rounds = 0
returns the input classes bit for bit, with their regions.  enforce_connectivity leaves a superpixel that is in one piece untouched;
its counts are recounted (integer), its centroids are superpixel_pool(new, features) when a feature map is given and None otherwise,
its positions are None (they are not recomputed), step and grid are kept.  Limits: Hs, Ws <= 32768, Hs Ws < 2^31.  ValueError before
any device work for a wrong dtype (int64 only), shape or contiguity, a connectivity outside {4, 8}, a min_size that is no int >= 1,
rounds that is no int >= 0, sizes over the limits or a non-Superpixels argument; RuntimeError for CPU tensors.  There is no CPU or eager
fallback."""
import ctypes
from collections import namedtuple

import torch

from . import _lib
from .crf import _check_map
from .features import DIM, _is_int, _p, _stream, _require_cuda
from .superpixel import STEPS, Superpixels, superpixel_grid, superpixel_pool

MAX_SIDE = 32768
MODE_SIEVE, MODE_FRAGMENTS = 0, 1      # include/msst.h: msst_regions_merge's mode
ERR_BYTES = 16                         # the scratch starts with the error word

Regions = namedtuple("Regions", ["labels", "sizes", "count", "connectivity", "error"])
SieveResult = namedtuple("SieveResult", ["classes", "regions", "history"])
ConnectedSuperpixels = namedtuple("ConnectedSuperpixels", ["superpixels", "regions", "history"])


def _check_values(values, what="values"):
    if not torch.is_tensor(values) or values.dim() != 3 or values.dtype != torch.int64 or not values.is_contiguous() or values.numel() == 0:
        raise ValueError(f"{what} must be a contiguous int64 tensor [Bs, Hs, Ws], got "
                         f"{getattr(values, 'dtype', '')} {tuple(getattr(values, 'shape', ())) or type(values).__name__}")
    Bs, Hs, Ws = values.shape
    if Hs > MAX_SIDE or Ws > MAX_SIDE or Hs * Ws >= 2 ** 31 or _lib.load().msst_regions_scratch_bytes(Bs, Hs, Ws) <= 0:
        raise ValueError(f"{what} {tuple(values.shape)} is over the limits: Hs, Ws <= {MAX_SIDE}, Hs Ws < 2^31")


def _check_connectivity(connectivity):
    if not _is_int(connectivity) or connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity!r}")


def _check_rounds(rounds):
    if not _is_int(rounds) or rounds < 0:
        raise ValueError(f"rounds must be an integer >= 0, got {rounds!r}")


def _scratch(shape, device):
    """the scratch of both calls, its error word zeroed"""
    n = _lib.load().msst_regions_scratch_bytes(*shape)
    scratch = torch.empty((n + 3) // 4, dtype=torch.int32, device=device)
    scratch[:ERR_BYTES // 4].zero_()
    return scratch


def _label(values, connectivity, scratch):
    Bs, Hs, Ws = values.shape
    dev = values.device
    labels = torch.empty(Bs, Hs, Ws, dtype=torch.int64, device=dev)
    sizes = torch.empty(Bs, Hs, Ws, dtype=torch.int32, device=dev)
    count = torch.empty(Bs, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().msst_regions_label(_p(values), Bs, Hs, Ws, connectivity, _p(labels), _p(sizes), _p(count), _p(scratch),
                                              4 * scratch.numel(), _stream()), "msst_regions_label")
    return Regions(labels, sizes, count, connectivity, scratch[:1])


def _merge(values, reg, mode, min_size, step, history_row, scratch):
    Bs, Hs, Ws = values.shape
    out = torch.empty_like(values)
    _lib.check(_lib.load().msst_regions_merge(_p(values), _p(reg.labels), _p(reg.sizes), Bs, Hs, Ws, reg.connectivity, mode, min_size, step,
                                              _p(out), ctypes.c_void_p(history_row), _p(scratch), 4 * scratch.numel(), _stream()),
               "msst_regions_merge")
    return out


def _raise_on(error):
    if error:
        raise RuntimeError(f"maskedsst_amd.regions: a device loop of the labelling stopped at its iteration cap (error word {error}); "
                           "the outputs are not to be used")


def _rounds(values, connectivity, rounds, mode, min_size, step):
    """rounds x (label, merge) and a final label; ONE synchronisation: (values, Regions, history [rounds, 4] int64 on the CPU)"""
    dev = values.device
    scratch = _scratch(values.shape, dev)
    hist = torch.zeros(rounds * 4 + 1, dtype=torch.int32, device=dev)
    cur = values
    for t in range(rounds):
        reg = _label(cur, connectivity, scratch)
        cur = _merge(cur, reg, mode, min_size, step, hist.data_ptr() + 16 * t, scratch)
    reg = _label(cur, connectivity, scratch)
    hist[4 * rounds:] = scratch[:1]                    # the error word rides with the history
    host = hist.cpu().long()                           # the one synchronisation
    _raise_on(int(host[-1]))
    return cur, reg, host[:-1].reshape(rounds, 4)


def label_regions(values, connectivity=4):
    """The connected regions of an int64 map [Bs, Hs, Ws] (contiguous, on the device; a value < 0 is dead): Regions(labels [Bs, Hs, Ws]
    int64, the root y0 Ws + x0 of the pixel's region, -1 dead; sizes [Bs, Hs, Ws] int32, the pixel count at a root pixel, 0 elsewhere;
    count [Bs] int32; connectivity; error int32 [1] on the device, the error word -- check_regions reads it); see the module's
    contract.  Three launches, no synchronisation.  ValueError before any device work for a wrong dtype, shape, contiguity or
    connectivity or sizes over the limits; RuntimeError for a CPU tensor."""
    _check_values(values)
    _check_connectivity(connectivity)
    _require_cuda(values, "values")
    return _label(values, connectivity, _scratch(values.shape, values.device))


def _check_regions(reg):
    if not isinstance(reg, Regions):
        raise ValueError(f"regions must be a Regions (from label_regions), got {type(reg).__name__}")
    _check_values(reg.labels, "the regions' labels")
    if not torch.is_tensor(reg.sizes) or reg.sizes.dtype != torch.int32 or reg.sizes.shape != reg.labels.shape or not reg.sizes.is_contiguous():
        raise ValueError("the regions' sizes must be a contiguous int32 tensor of the labels' shape")
    _require_cuda(reg.labels, "the regions' labels")
    _require_cuda(reg.sizes, "the regions' sizes")


def check_regions(regions):
    """Read the error word of a label_regions result (one synchronisation): RuntimeError when a device loop stopped at its cap."""
    _check_regions(regions)
    _raise_on(int(regions.error.cpu()[0]))
    return regions


def region_ids(regions):
    """Dense region ids of a Regions: (ids [Bs, Hs, Ws] int64, the regions of a scene numbered 0 .. n - 1 by ascending root -- the
    raster order of their first pixels -- and -1 for a dead pixel; n [Bs] int64).  Index plumbing on the device (a cumulative sum
    over the root pixels and a gather), no synchronisation."""
    _check_regions(regions)
    Bs, Hs, Ws = regions.labels.shape
    roots = (regions.sizes > 0).view(Bs, -1)
    rank = torch.cumsum(roots, dim=1) - 1
    lab = regions.labels.view(Bs, -1)
    ids = torch.where(lab >= 0, rank.gather(1, lab.clamp(min=0)), lab.new_full((), -1))
    return ids.view(Bs, Hs, Ws), roots.sum(dim=1)


def sieve_classes(classes, min_size, connectivity=4, rounds=4):
    """The sieve (minimum mapping unit) of a class map [Bs, Hs, Ws] int64: `rounds` simultaneous rounds in which every region of fewer
    than min_size pixels is merged into its largest live neighbour of at least min_size pixels (then the lowest root); see the
    module's contract.  SieveResult(classes, regions: the Regions of the returned classes, history [rounds, 4] int64 on the CPU: live
    regions, flagged, merged, changed pixels per round).  min_size = 1 or rounds = 0 returns the input classes bit for bit.  A small
    patch whose neighbours are all small waits for a later round; one enclosed by dead pixels stays.  3 + 6 rounds launches and one
    synchronisation.  ValueError before any device work; RuntimeError for a CPU tensor or a raised error word."""
    _check_values(classes, "classes")
    if not _is_int(min_size) or min_size < 1 or min_size >= 2 ** 31:
        raise ValueError(f"min_size must be an integer >= 1 (and below 2^31), got {min_size!r}")
    _check_connectivity(connectivity)
    _check_rounds(rounds)
    _require_cuda(classes, "classes")
    out, reg, history = _rounds(classes, connectivity, rounds, MODE_SIEVE, min_size, 0)
    return SieveResult(out, reg, history)


def enforce_connectivity(superpixels, features=None, connectivity=4, rounds=4):
    """SLIC's connectivity pass on a Superpixels (from fit_superpixels): per superpixel id the largest piece (then the lowest root) is
    kept and every other piece is merged into the largest neighbouring kept piece whose id is eligible for it; see the module's
    contract.  ConnectedSuperpixels(superpixels: labels merged, counts recounted, centroids = superpixel_pool(new, features) for a
    feature map [Bs, 96, Hs, Ws] and None without one, positions None, history, step and grid kept; regions: the Regions of the new
    labels; history [rounds, 4] int64 on the CPU).  A piece without an eligible neighbour stays a fragment: history[-1] and regions
    say how many are left.  A superpixel that was in one piece is untouched.  ValueError before any device work; RuntimeError for CPU
    tensors or a raised error word."""
    if not isinstance(superpixels, Superpixels):
        raise ValueError(f"superpixels must be a Superpixels (from fit_superpixels), got {type(superpixels).__name__}")
    sp = superpixels
    if not _is_int(sp.step) or sp.step not in STEPS:
        raise ValueError(f"the superpixels' step must be one of {STEPS}, got {sp.step!r}")
    _check_values(sp.labels, "the superpixels' labels")
    Bs, Hs, Ws = sp.labels.shape
    if tuple(sp.grid) != superpixel_grid(Hs, Ws, sp.step):
        raise ValueError(f"the superpixels' grid {sp.grid!r} is not that of a {Hs} x {Ws} scene at step {sp.step}")
    if features is not None:
        _check_map(features, "features", DIM)
        if (features.shape[0],) + tuple(features.shape[2:]) != (Bs, Hs, Ws):
            raise ValueError(f"features {tuple(features.shape)} do not match the superpixels' Bs, Hs, Ws {(Bs, Hs, Ws)}")
    _check_connectivity(connectivity)
    _check_rounds(rounds)
    _require_cuda(sp.labels, "the superpixels' labels")
    if features is not None:
        _require_cuda(features, "features")
    labels, reg, history = _rounds(sp.labels, connectivity, rounds, MODE_FRAGMENTS, 1, sp.step)
    n_sp = sp.grid[0] * sp.grid[1]
    flat = labels.view(Bs, -1)
    live = (flat >= 0) & (flat < n_sp)
    counts = torch.zeros(Bs, n_sp, dtype=torch.int32, device=labels.device)
    counts.scatter_add_(1, torch.where(live, flat, torch.zeros_like(flat)), live.to(torch.int32))
    new = Superpixels(labels, None, None, counts, sp.history, sp.step, tuple(sp.grid))
    if features is not None:
        new = new._replace(centroids=superpixel_pool(new, features))
    return ConnectedSuperpixels(new, reg, history)
