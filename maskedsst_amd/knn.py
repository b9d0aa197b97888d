"""kNN evaluation of frozen per-pixel features: the weighted k-nearest-neighbour classifier over a bank of labelled features
(Wu et al. 2018; the protocol of the DINO and SimMIM papers), the standard way to judge a self-supervised encoder without
training anything -- and, on a sparsely labelled hyperspectral scene, the natural few-label classifier.

    bank = feature_bank(model, train_scenes, train_labels, per_class=2000)       # KnnBank: unit features [M, 96] + labels
    res = model.knn_predict_scene(scene, bank, k=20, temperature=0.07)           # KnnScene(classes, votes, cover)
    res = knn_classify(bank, features, k=20)                                     # KnnResult(classes, votes, index, sim)

Two launches of ``libmsst.so`` (``maskedsst_amd/csrc/msst_knn.hip``, ``include/msst.h``): ``msst_knn_topk`` computes the
similarities q . bank[m] on the fp32 matrix cores and selects each query's k neighbours behind them -- no [Q, M] score matrix
exists, and ``knn_predict_scene`` reads the ``encode_scene`` map [Bs, 96, Hs, Ws] in place, no permuted copy -- and
``msst_knn_vote`` sums the weights w_j = exp((s_j - s_1) / temperature) per class.  Neighbours are ranked by ONE total order,
similarity descending and then bank index ascending, so ties have a fixed answer and every output has the same bits in every
call, for every ``splits`` and for a query whatever batch it sits in.  There is no CPU or eager fallback.
"""
from collections import namedtuple

import torch

from . import _lib
from .features import DIM, MAX_CLASSES, KnnBank, _bank_from_scenes, _is_int, _p, _stream, _require_cuda, check_rows, on_scene_map  # noqa: F401

MAX_K = 64        # include/msst.h: msst_knn_topk
MAX_SPLITS = 64

# classes [Q] int64 (-1: a query without neighbours, i.e. one with a NaN channel), votes [Q, n_classes] fp32,
# index [Q, k] int32 bank rows in rank order (-1 past the bank's size), sim [Q, k] fp32 their similarities (-inf there)
KnnResult = namedtuple("KnnResult", ["classes", "votes", "index", "sim"])
# classes [Bs, Hs, Ws] int64 (-1 where no window covers the pixel), votes [Bs, n_classes, Hs, Ws] fp32, cover [Bs, Hs, Ws] int32
KnnScene = namedtuple("KnnScene", ["classes", "votes", "cover"])


def _check_bank(bank):
    if not isinstance(bank, KnnBank):
        raise ValueError(f"bank must be a KnnBank, got {type(bank).__name__}")


def _check_k(k, temperature, splits):
    if not _is_int(k) or not 1 <= k <= MAX_K:
        raise ValueError(f"k must be an integer in [1, {MAX_K}], got {k!r}")
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or not temperature >= 0:
        raise ValueError(f"temperature must be a number >= 0 (0: uniform weights), got {temperature!r}")
    if splits is not None and (not _is_int(splits) or not 1 <= splits <= MAX_SPLITS):
        raise ValueError(f"splits must be None or an integer in [1, {MAX_SPLITS}], got {splits!r}")


def knn_launch(bank, queries, q_layout, Q, plane, k, temperature, splits, votes, vote_layout, classes, index=None, sim=None):
    """The two launches on the current stream: queries is rows [Q, 96] (q_layout 0) or a map [Bs, 96, plane] (q_layout 1) read in
    place; votes and classes are written in vote_layout.  Returns (index [Q, k] int32, sim [Q, k])."""
    lib = _lib.load()
    dev = queries.device
    index = torch.empty(Q, k, dtype=torch.int32, device=dev) if index is None else index
    sim = torch.empty(Q, k, dtype=torch.float32, device=dev) if sim is None else sim
    sp = 0 if splits is None else splits
    nbytes = int(lib.msst_knn_scratch_bytes(Q, len(bank), k, sp))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
    st = _stream()
    _lib.check(lib.msst_knn_topk(_p(bank.features), len(bank), DIM, _p(queries), q_layout, Q, plane, k, sp, _p(index), _p(sim),
                                 _p(scratch), nbytes, st), "msst_knn_topk")
    _lib.check(lib.msst_knn_vote(_p(index), _p(sim), _p(bank.labels), Q, k, bank.n_classes, float(temperature), _p(votes),
                                 vote_layout, plane, _p(classes), st), "msst_knn_vote")
    return index, sim


def knn_classify(bank, queries, k=20, temperature=0.07, splits=None):
    """Classify queries [Q, 96] (fp32, contiguous, on the device) by the weighted vote of their k most similar bank rows:
    KnnResult(classes [Q] int64, votes [Q, n_classes], index [Q, k] int32, sim [Q, k]).  Neighbours come in rank order (similarity
    descending, ties by bank index ascending); with fewer than k bank rows the tail is index -1 / similarity -inf; a query with a
    NaN channel has no neighbours, zero votes and class -1.  temperature = 0: uniform weights (a plain majority vote, ties to the
    lowest class).  splits: bank slices walked by different workgroups (None: the library chooses from the sizes); the result has
    the same bits for every value.  ValueError, before any device work, for a wrong rank, width, dtype, k, temperature or splits;
    RuntimeError for CPU tensors."""
    _check_bank(bank)
    check_rows(queries, "queries", shape=f"[Q, {DIM}]")
    _check_k(k, temperature, splits)
    _require_cuda(queries, "queries")
    Q = queries.shape[0]
    votes = torch.empty(Q, bank.n_classes, dtype=torch.float32, device=queries.device)
    classes = torch.empty(Q, dtype=torch.int64, device=queries.device)
    index, sim = knn_launch(bank, queries, 0, Q, 1, k, temperature, splits, votes, 0, classes)
    return KnnResult(classes, votes, index, sim)


def knn_predict_scene(model, scene, bank, k=20, temperature=0.07, stride=None, max_windows=None):
    """See ViTSpatialSpectral.knn_predict_scene."""
    _check_bank(bank)
    _check_k(k, temperature, None)

    def launch(emb, Bs, Hs, Ws):
        dev = emb.features.device
        votes = torch.empty(Bs, bank.n_classes, Hs, Ws, dtype=torch.float32, device=dev)
        classes = torch.empty(Bs, Hs, Ws, dtype=torch.int64, device=dev)
        knn_launch(bank, emb.features, 1, Bs * Hs * Ws, Hs * Ws, k, temperature, None, votes, 1, classes)
        return KnnScene(classes, votes, emb.cover)

    return on_scene_map(model, scene, stride, True, max_windows, launch)


def feature_bank(model, scenes, labels, stride=None, ignored_label=-1, per_class=None, generator=None):
    """A KnnBank from labelled scenes: encode_scene(normalize=True) on scenes [Bs, bands, Hs, Ws], then the unit features of the
    pixels that a window covers and whose label in labels [Bs, Hs, Ws] is not ignored_label, in scene-major pixel order.
    per_class: at most that many rows per class, a random subset drawn with `generator` (a CPU torch.Generator; None: the global
    one), rows kept in pixel order.  n_classes is the model's num_classes.  ValueError for labels of the wrong shape or dtype, or
    when no pixel is left."""
    return _bank_from_scenes(model, scenes, labels, stride, ignored_label, per_class, generator, True)
