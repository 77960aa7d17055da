"""The workspace carver (mpvae-1_amd/csrc/workspace.h) on the host: compiles
tests/host/workspace_check.cpp, which includes that header alone, and runs it.
The program checks the sizing pass against a real pass over a malloc'ed buffer,
0-count pieces, the refusals and two families' piece lists; it exits non-zero at
the first failed check."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_workspace_check(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ not found: the host library needs it too")
    exe = str(tmp_path / "workspace_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "mpvae-1_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "workspace_check.cpp"), "-o", exe],
                   check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
