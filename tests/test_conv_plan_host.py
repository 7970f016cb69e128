"""The conv launcher's decisions, held bit for bit to a recording.

tests/conv_plan_probe.cpp asks the library, through its public queries alone and without a device, what it decides for a
fixed list of descriptors under the cost model and under every pinned (configuration, split-K) request: GroupNorm mode
and row blocks, LayerNorm slots, return codes and message texts.  tests/golden/conv_plan.txt is that program's output at
the commit before the launcher was split into a planner and a launch step; any difference is a change of behaviour, to be
removed from the code and never re-recorded."""
import os
import shutil
import subprocess

import pytest

from upgpt_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


def test_conv_plan_matches_the_recording(tmp_path):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("no hipcc")
    _lib.load_library()  # (raises when the library has not been built)
    libdir, libname = os.path.split(os.path.abspath(_lib.LIB_PATH))
    exe = str(tmp_path / "conv_plan_probe")
    subprocess.run([hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1",
                    os.path.join(ROOT, "tests", "conv_plan_probe.cpp"), "-o", exe,
                    "-L" + libdir, "-l:" + libname, "-Wl,-rpath," + libdir], check=True, capture_output=True, text=True)
    got = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    want = open(os.path.join(ROOT, "tests", "golden", "conv_plan.txt")).read().splitlines()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w, "decision changed for " + w.split(" ")[0]
