#!/usr/bin/env python3
"""Scene report timing (GPU box): ``maskedsst_amd.scene.scene_report`` -- one pass of the extended HIP loss kernels (loss, counts and
confusion matrix) and two read-backs -- against an eager restatement of the same numbers in PyTorch: boolean-index compaction of the
counting pixels, ``torch.bincount`` of ``label * nc + argmax`` for the confusion matrix, ``F.cross_entropy`` on the compacted rows,
and ``confusion_report`` of the matrix on the host (the same function on both legs).  ``--weighted``: the eager leg's loss takes class
weights (``F.cross_entropy(weight=)``) and the fused leg is ``cross_entropy_stats(weight=, confusion=True, skip=classes)`` with the
same report.

Random logits and labels of ``--scenes`` 64 x 64 scenes with ``--classes`` classes, a border of 3 uncovered pixels (class -1), about
one label in nine ignored.  Both legs are warmed up, then alternated call by call in one process, each call between two HIP events
and ended by its own read-back; the result is the median of ``--calls`` calls per leg.  No speed claim rests on this tool: it records
what one box gave.  Prints ONE JSON line.

Run:  python tools/ce_ext_time.py [--scenes 4] [--classes 8] [--calls 20] [--warmup 5] [--weighted]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from maskedsst_amd.ops import confusion_report, cross_entropy_stats  # noqa: E402
from maskedsst_amd.scene import scene_report  # noqa: E402


def eager_report(logits, classes, labels, nc, weight=None):
    """the eager tail: -> (loss, confusion_report)"""
    valid = (classes != -1) & (labels != -1)
    lab = labels[valid]
    rows = logits.permute(0, 2, 3, 1)[valid]
    loss = F.cross_entropy(rows, lab, weight=weight)
    cm = torch.bincount(lab * nc + rows.argmax(dim=1), minlength=nc * nc).reshape(nc, nc)
    return float(loss), confusion_report(cm)


def fused_report(logits, classes, labels, nc, weight=None):
    if weight is None:
        r = scene_report(logits, classes, labels)
        return r.loss, r.report
    with torch.no_grad():
        _, stats = cross_entropy_stats(logits, labels, -1, skip=classes, weight=weight, confusion=True)
    h = stats.host()
    return h.loss, confusion_report(h.confusion)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=4)
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--weighted", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(5)
    nc = args.classes
    logits = torch.randn(args.scenes, nc, 64, 64, generator=gen).to(dev)
    labels = torch.randint(-1, nc, (args.scenes, 64, 64), generator=gen).to(dev)
    classes = logits.argmax(dim=1)
    for sl in ((slice(None), slice(0, 3)), (slice(None), slice(-3, None)), (slice(None), slice(None), slice(0, 3)),
               (slice(None), slice(None), slice(-3, None))):
        classes[sl] = -1
    weight = (torch.rand(nc, generator=gen) * 2.9 + 0.1).to(dev) if args.weighted else None
    legs = {"fused": fused_report, "eager": eager_report}
    out = {}
    for _ in range(args.warmup):
        for name, fn in legs.items():
            out[name] = fn(logits, classes, labels, nc, weight)
    (lf, rf), (le, re_) = out["fused"], out["eager"]
    agree = dict(loss_rel=abs(lf - le) / abs(le), oa=abs(rf.oa - re_.oa), kappa=abs(rf.kappa - re_.kappa), miou=abs(rf.mean_iou - re_.mean_iou),
                 pixels=[rf.total, re_.total])
    t = {name: [] for name in legs}
    for _ in range(args.calls):
        for name, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(logits, classes, labels, nc, weight)
            e1.record()
            e1.synchronize()
            t[name].append(e0.elapsed_time(e1))
    res = dict(tool="ce_ext_time", shape=dict(scenes=args.scenes, size=64, n_classes=nc), weighted=args.weighted, calls=args.calls,
               warmup=args.warmup, call_ms={k: round(statistics.median(v), 4) for k, v in t.items()},
               call_ms_min={k: round(min(v), 4) for k, v in t.items()}, call_ms_max={k: round(max(v), 4) for k, v in t.items()},
               legs_agree=agree)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
