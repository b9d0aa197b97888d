#!/usr/bin/env python3
"""Golden fixture of the shifting-window stacking: the reference's (HSG-AIML/MaskedSST) ``stack_image_batch`` (src/utils.py:451-474)
applied to small integer-valued tiles, captured as ``tests/golden/stack_image_batch.npz`` (tests/test_shifting_window_host.py
compares ``maskedsst_amd.utils.stack_image_batch`` against it bit for bit).

Cases: ``s8`` -- image_size 8, patch_sub 0 on 2 tiles of 3 bands, 16 x 16 (no cutoff, 4 windows per tile); ``s7`` -- image_size 8,
patch_sub 1 on 2 tiles of 3 bands, 23 x 23 (cutoff 2, 9 windows per tile).  Inputs: ``img[b, c, y, x] = ((b C + c) H + y) W + x``
(int32, every pixel its own value), ``label[b, y, x] = (b H + y) W + x`` (int32).  Stored per case: img, label, and the reference's
stacked img and label.

Run:  MSST_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_shifting_window.py
"""
import ast
import os
import types

import numpy as np
import torch
from einops import rearrange

REF = os.environ.get("MSST_REFERENCE", "")
if not os.path.isdir(os.path.join(REF, "src")):
    raise SystemExit("set MSST_REFERENCE to a checkout of the reference: nothing to generate")


def reference_function(path, name, namespace):
    """the function `name` of the reference file `path`, compiled from that file alone: src/utils.py imports its experiment tracker
    and the GeoTIFF readers at module level, none of which the function needs"""
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    node = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name)
    exec(compile(ast.Module([node], []), path, "exec"), namespace)
    return namespace[name]


stack_image_batch = reference_function(os.path.join(REF, "src", "utils.py"), "stack_image_batch", {"rearrange": rearrange})

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "stack_image_batch.npz")


def case(image_size, patch_sub, B, C, H, W):
    img = torch.arange(B * C * H * W, dtype=torch.int32).reshape(B, C, H, W)
    label = torch.arange(B * H * W, dtype=torch.int32).reshape(B, H, W)
    config = types.SimpleNamespace(image_size=image_size, patch_sub=patch_sub)
    simg, slabel = stack_image_batch(config, img, label)
    return img.numpy(), label.numpy(), simg.contiguous().numpy(), slabel.contiguous().numpy()


if __name__ == "__main__":
    out = {}
    for name, args in (("s8", (8, 0, 2, 3, 16, 16)), ("s7", (8, 1, 2, 3, 23, 23))):
        img, label, simg, slabel = case(*args)
        out.update({f"{name}_img": img, f"{name}_label": label, f"{name}_stacked_img": simg, f"{name}_stacked_label": slabel,
                    f"{name}_cfg": np.array(args[:2], dtype=np.int32)})
        print(name, img.shape, "->", simg.shape, slabel.shape)
    np.savez_compressed(OUT, **out)
