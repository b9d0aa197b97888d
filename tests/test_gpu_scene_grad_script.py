"""GPU: finetune.py --val-saliency-scene end to end in a child process."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def child(cmd, timeout):
    """a script in a fresh child process under its own time limit.  A child that timed out or died of a signal (a GPU fault, an abort)
    ends the session: nothing more is started on the device after it."""
    e = dict(os.environ)
    e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
    try:
        r = subprocess.run(cmd, cwd=ROOT, env=e, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as t:
        pytest.exit(f"{' '.join(cmd)} timed out after {timeout} s: no further GPU work\n{(t.stderr or '')[-2000:]}", returncode=1)
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        pytest.exit(f"{' '.join(cmd)} ended with {r.returncode}: no further GPU work\n{r.stderr[-3000:]}", returncode=1)
    return r


def test_finetune_val_saliency_scene_script():
    """one more line per validation pass: five distinct bands of the 200, strongest first"""
    r = child([sys.executable, "finetune.py", "--steps", "2", "--batch-size", "2", "--val-scenes", "2", "--val-every", "1",
               "--val-saliency-scene"], 600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    sal = [l.split() for l in lines if l.startswith("val-saliency-scene step ")]
    assert [s[2] for s in sal] == ["1", "2"], r.stdout
    assert len([l for l in lines if l.startswith("val step ")]) == 2
    for s in sal:
        assert s[3:5] == ["top", "bands"] and s[-2:] == ["scenes", "2"]
        pairs = [p.split(":") for p in s[5:-2]]
        bands, values = [int(b) for b, _ in pairs], [float(v) for _, v in pairs]
        assert len(set(bands)) == 5 and all(0 <= b < 200 for b in bands)
        assert values == sorted(values, reverse=True) and values[-1] > 0.0


def test_finetune_val_saliency_scene_needs_val_scenes():
    r = child([sys.executable, "finetune.py", "--steps", "1", "--val-saliency-scene"], 600)
    assert r.returncode != 0 and "--val-scenes" in r.stderr
