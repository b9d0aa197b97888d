"""What the three evaluators of frozen per-pixel features share (maskedsst_amd.knn, maskedsst_amd.probe, maskedsst_amd.cluster): the
feature width, the argument checks, the ctypes plumbing, the bank of labelled rows and the scene wrapper.  The kernels' shared pieces
live in ``maskedsst_amd/csrc/msst_feat.h``.
"""
import ctypes

import torch

DIM = 96          # the encoder's feature width: the only one the kernels take
MAX_CLASSES = 128


def _require_cuda(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"maskedsst_amd runs on an MI355X only ({what} is on {t.device}); there is no CPU fallback")


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _is_int(v):
    return not isinstance(v, bool) and isinstance(v, int)


def check_rows(t, what, min_rows=0, shape=f"[M, {DIM}]", few=None):
    """ValueError unless t is a contiguous float32 tensor [rows, 96] of at least min_rows rows.  `shape` is how the message writes the
    wanted shape; `few` is the message for too few rows (None: the shape message says it)."""
    if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] != DIM or (few is None and t.shape[0] < min_rows):
        raise ValueError(f"{what} must be a 2-D tensor {shape}, got {getattr(t, 'shape', type(t))}")
    if t.dtype != torch.float32:
        raise ValueError(f"{what} must be float32, got {t.dtype}")
    if t.shape[0] < min_rows:
        raise ValueError(few)
    if not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous")


class KnnBank:
    """A bank of labelled features: features [M, 96] fp32 contiguous on the device (unit length for cosine similarity; the
    kernels take any finite values), labels [M] integers in [0, n_classes).  One check at construction, with one read-back:
    ValueError for a label outside the range or a feature that is not finite.  CPU tensors raise RuntimeError."""

    def __init__(self, features, labels, n_classes):
        check_rows(features, "features", 1, few="the bank needs at least one row")
        if not torch.is_tensor(labels) or labels.dim() != 1 or labels.shape[0] != features.shape[0]:
            raise ValueError(f"labels must be a 1-D tensor [{features.shape[0]}], got {getattr(labels, 'shape', type(labels))}")
        if labels.dtype not in (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8):
            raise ValueError(f"labels must be integers, got {labels.dtype}")
        if not _is_int(n_classes) or not 1 <= n_classes <= MAX_CLASSES:
            raise ValueError(f"n_classes must be an integer in [1, {MAX_CLASSES}], got {n_classes!r}")
        _require_cuda(features, "the bank's features")
        _require_cuda(labels, "the bank's labels")
        bad = torch.stack([((labels < 0) | (labels >= n_classes)).any(), ~torch.isfinite(features).all()]).tolist()
        if bad[0]:
            raise ValueError(f"labels must lie in [0, {n_classes})")
        if bad[1]:
            raise ValueError("features must be finite (drop the uncovered pixels of encode_scene: cover == 0)")
        self.features = features
        self.labels = labels.to(torch.int32).contiguous()
        self.n_classes = n_classes

    def __len__(self):
        return self.features.shape[0]


def _bank_from_scenes(model, scenes, labels, stride, ignored_label, per_class, generator, normalize):
    """feature_bank (normalize=True) and maskedsst_amd.probe_bank (normalize=False: the raw features the head consumes)"""
    if not torch.is_tensor(scenes) or scenes.dim() != 4:
        raise ValueError(f"scenes must be a 4-D tensor [scenes, bands, H, W], got {getattr(scenes, 'shape', type(scenes))}")
    if not torch.is_tensor(labels) or labels.dim() != 3 or labels.shape != (scenes.shape[0],) + tuple(scenes.shape[2:]):
        raise ValueError(f"labels must be a 3-D tensor [scenes, H, W] matching the scenes, got {getattr(labels, 'shape', type(labels))}")
    if labels.dtype not in (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8):
        raise ValueError(f"labels must be integers, got {labels.dtype}")
    if per_class is not None and (not _is_int(per_class) or per_class < 1):
        raise ValueError(f"per_class must be None or a positive integer, got {per_class!r}")
    emb = model.encode_scene(scenes, stride=stride, normalize=normalize)
    labels = labels.to(emb.features.device)
    ok = (emb.cover > 0) & (labels != ignored_label)
    feats = emb.features.permute(0, 2, 3, 1)[ok].contiguous()
    labs = labels[ok].long()
    if per_class is not None and len(labs):
        lab_cpu = labs.cpu()
        keep = torch.zeros(len(lab_cpu), dtype=torch.bool)
        for c in torch.unique(lab_cpu).tolist():
            rows = torch.nonzero(lab_cpu == c).reshape(-1)
            if len(rows) > per_class:
                rows = rows[torch.randperm(len(rows), generator=generator)[:per_class]]
            keep[rows] = True
        keep = keep.to(feats.device)
        feats, labs = feats[keep].contiguous(), labs[keep]
    if len(labs) == 0:
        raise ValueError("no covered, labelled pixel to put into the bank")
    return KnnBank(feats, labs, int(model.num_classes))


def on_scene_map(model, scene, stride, normalize, max_windows, launch):
    """encode_scene, then launch(emb, Bs, Hs, Ws) on its map [Bs, 96, Hs, Ws], which the kernels read in place (layout 1, Bs Hs Ws
    rows, plane Hs Ws); returns what launch returns"""
    from .scene import encode_scene, SCENE_MAX_WINDOWS
    emb = encode_scene(model, scene, stride, normalize, SCENE_MAX_WINDOWS if max_windows is None else max_windows)
    Bs, _, Hs, Ws = emb.features.shape
    return launch(emb, Bs, Hs, Ws)
