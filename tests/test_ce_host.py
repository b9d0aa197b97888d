"""Fused cross entropy, host side (no GPU needed): the C ABI of msst_ce_stats_fwd / msst_ce_bwd (additive under MSST_VERSION 109), their
argument checks (they run before any HIP call, so null buffers and no device are enough to see them), and the Python surface: no CPU
fallback, FusedCrossEntropy is no torch loss in disguise, and a torch criterion never reaches the new op."""
import re
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

BADARG, UNSUPPORTED = -3, -2   # include/msst.h: MSST_ERR_BADARG, MSST_ERR_UNSUPPORTED
CALLS = ("msst_ce_scratch_bytes", "msst_ce_stats_fwd", "msst_ce_bwd")


def test_c_abi_declares_and_exports_the_cross_entropy_calls():
    from maskedsst_amd import _lib
    header = open(_lib.HEADER_PATH).read()
    assert re.search(r"^long msst_ce_scratch_bytes\(", header, re.M)
    assert re.search(r"^int msst_ce_stats_fwd\(", header, re.M) and re.search(r"^int msst_ce_bwd\(", header, re.M)
    assert _lib.header_version() == 109   # additive: the revision does not move
    lib = _lib.load()                      # refuses a library that lacks a declared symbol
    assert lib.msst_version() == 109 and set(CALLS) <= set(_lib.declared_symbols())
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in CALLS:
        assert re.search(r" T %s$" % name, out, re.M), name
    # the record slots the binding uses are the header's
    for name, want in (("LOSS_SUM", _lib.CE_LOSS_SUM), ("N_VALID", _lib.CE_N_VALID), ("N_CORRECT", _lib.CE_N_CORRECT),
                       ("BAD_LABELS", _lib.CE_BAD_LABELS), ("NONFINITE", _lib.CE_NONFINITE), ("SUPPORT", _lib.CE_SUPPORT)):
        m = re.search(r"#define\s+MSST_CE_%s\s+(\d+)" % name, header)
        assert m and int(m.group(1)) == want, name
    names = [lib.msst_profile_name(i).decode() for i in range(lib.msst_profile_kernels())]
    assert "cross_entropy" in names and "?" not in names


def test_cross_entropy_calls_refuse_bad_arguments_before_launch():
    from maskedsst_amd import _lib
    lib = _lib.load()

    def fwd(R0, nc, M):
        return lib.msst_ce_stats_fwd(None, None, None, -1, None, None, None, None, R0, nc, M, None)

    def bwd(R0, nc, M):
        return lib.msst_ce_bwd(None, None, None, None, R0, nc, M, None)

    for shape in [(0, 8, 64), (4, 0, 64), (4, 8, 0), (-1, 8, 64), (4, -3, 1), (0, 0, 0)]:
        assert fwd(*shape) == BADARG and bwd(*shape) == BADARG, shape
        assert lib.msst_ce_scratch_bytes(*shape) == 0, shape
    assert b"msst_ce_bwd" in lib.msst_last_error()
    # 2^31 rows, or 2^31 logits: beyond the kernels' index range
    for shape in [(1 << 16, 8, 1 << 15), (1 << 20, 4096, 1), (3, 1 << 30, 1), (1 << 30, 1, 2)]:
        assert fwd(*shape) == UNSUPPORTED and bwd(*shape) == UNSUPPORTED, shape
        assert lib.msst_ce_scratch_bytes(*shape) == 0, shape
    assert fwd(0, 8, 1 << 30) == BADARG   # a size below 1 wins over a size beyond the kernels
    # shapes the kernels take, with null pointers: refused as bad arguments, nothing launched
    for shape in [(256, 8, 64), (1, 8, 1), (5, 1, 64), (2, 97, 5), (4, 8, 4096), (1, 5000, 1)]:
        assert fwd(*shape) == BADARG and bwd(*shape) == BADARG, shape
    # scratch: one fp32 loss partial and one int32 row [4 + 2 nc] per 256 rows
    assert lib.msst_ce_scratch_bytes(256, 8, 64) == 64 * (5 + 16) * 4
    assert lib.msst_ce_scratch_bytes(1, 8, 1) == (5 + 16) * 4
    assert lib.msst_ce_scratch_bytes(3, 97, 100) == 2 * (5 + 194) * 4


def test_cross_entropy_stats_has_no_cpu_fallback_and_checks_shapes():
    from maskedsst_amd.ops import cross_entropy_stats, FusedCrossEntropy
    logits, labels = torch.randn(2, 8, 4, 4), torch.randint(-1, 8, (2, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cross_entropy_stats(logits, labels)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FusedCrossEntropy(-1)(logits, labels)
    assert not issubclass(FusedCrossEntropy, torch.nn.CrossEntropyLoss) and isinstance(FusedCrossEntropy(), torch.nn.Module)
    assert not issubclass(FusedCrossEntropy, torch.nn.modules.loss._Loss)
    assert FusedCrossEntropy(ignore_index=-3).ignore_index == -3 and FusedCrossEntropy().ignore_index == -1


def test_finetune_loss_flag_and_criterion():
    import finetune
    ap = finetune.build_parser()
    assert ap.parse_args([]).loss == "torch" and ap.parse_args(["--loss", "fused"]).loss == "fused"
    with pytest.raises(SystemExit):
        ap.parse_args(["--loss", "focal"])
    crit = finetune.make_criterion("torch", -1)
    assert type(crit) is torch.nn.CrossEntropyLoss and crit.ignore_index == -1
    from maskedsst_amd.ops import FusedCrossEntropy
    crit = finetune.make_criterion("fused", -1)
    assert type(crit) is FusedCrossEntropy and crit.ignore_index == -1 and crit.fused_stats


TORCH_CRITERION_SCRIPT = r"""
import sys, torch
from maskedsst_amd.config import Dotdict
from maskedsst_amd.utils import train_step
import maskedsst_amd.utils as U

class Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.randn(5, 3))
    def forward(self, img):
        return torch.einsum("bchw,kc->bkhw", img, self.w)

torch.manual_seed(0)
model = Tiny()
opt = torch.optim.SGD(model.parameters(), lr=0.1)
cfg = Dotdict(dict(image_size=4, ignored_label=-1, pixelwise=False))
img, label = torch.randn(2, 3, 4, 4), torch.randint(-1, 5, (2, 4, 4))
called = []
U._fused_tail = lambda *a, **k: called.append(1)
crit = torch.nn.CrossEntropyLoss(ignore_index=-1)
before = model.w.detach().clone()
loss, acc, macro = train_step(img, label, model, cfg, "cpu", crit, opt)
want = torch.nn.functional.cross_entropy(torch.einsum("bchw,kc->bkhw", img, before), label, ignore_index=-1)
assert not called and torch.equal(loss.detach(), want) and float(macro) == float(acc)
assert not torch.equal(model.w.detach(), before)
assert "maskedsst_amd.ops" not in sys.modules, "a torch criterion imported the fused op"
print("ok")
"""


def test_train_step_with_a_torch_criterion_never_touches_the_fused_op():
    """in a fresh interpreter: the eager path of train_step (here on the CPU, with a stand-in model) gives torch's loss, steps the
    optimizer, does not enter the fused tail and does not even import maskedsst_amd.ops"""
    import os
    e = dict(os.environ)
    e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-c", TORCH_CRITERION_SCRIPT], cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), f"--- stdout\n{r.stdout[-3000:]}\n--- stderr\n{r.stderr[-3000:]}"
