"""scripts/kernel_identity.py, the proof tool of a refactor of the kernel files: a library against itself is identical and not empty; the shipped library
against the diagnosis library is not, and the instances only the diagnosis build has (the window-MLP timeline instances, the poison kernels) are listed as
such.  No GPU: the tool reads the code objects out of the libraries."""
import os
import subprocess
import sys

import pytest

from tests.util import CSRC_DIR

TOOL = os.path.normpath(os.path.join(CSRC_DIR, "..", "..", "scripts", "kernel_identity.py"))
SHIPPED, DIAG = (os.path.join(CSRC_DIR, n) for n in ("libfvit_hip.so", "libfvit_hip_diag.so"))
pytestmark = pytest.mark.skipif(not (os.path.isfile(SHIPPED) and os.path.isfile(DIAG)), reason="both libraries must be built")


def run(a, b):
    res = subprocess.run([sys.executable, TOOL, a, b], capture_output=True, text=True)
    assert res.stderr == "", res.stderr
    return res.returncode, res.stdout.splitlines()


def test_a_library_is_identical_to_itself():
    rc, out = run(SHIPPED, SHIPPED)
    assert rc == 0 and out[-1] == "only in A: 0, only in B: 0, differ: 0", out[-3:]
    n = int(out[-3].split(": ")[1].split()[0])
    assert n >= 2 * 52, out[-3]   # a kernel and its descriptor each; the conv and stem units alone hold 52 kernels


def test_the_diagnosis_library_differs_and_holds_the_timeline_instances():
    rc, out = run(SHIPPED, DIAG)
    assert rc != 0
    only_b = [l.split(": ", 1)[1] for l in out if l.startswith("only in B: ")]   # (the summary, the last line, starts with "only in A")
    assert not [l for l in out[:-1] if l.startswith("only in A: ")]
    # winmlp_kernel<_Float16, .., TS = true, ..> (fvit_debug_win_mlp_timeline) for C = 256 and C = 512, each with its descriptor
    timeline = [k for k in only_b if "winmlp_kernel" in k and "Lb1ELb0ELb0E" in k]
    assert len(timeline) == 4 and sum(k.endswith(".kd") for k in timeline) == 2, only_b
    assert out[-1].startswith("only in A: 0, only in B: %d, differ: " % len(only_b)) and not out[-1].endswith("differ: 0"), out[-1]
