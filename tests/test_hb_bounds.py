"""The builder of chain and lists in pieces touches no byte outside its arrays: tests/emu/hb_bounds_main.cpp, a program of its own on
the lane-emulated device code (plz4_amd/csrc/lz4hc_lists_device.inl), built with the address and undefined-behaviour sanitizers and
run as a child process (the sanitizers never enter this process; CPU only).  Every array is a heap allocation of exactly the size
the kernels' layouts give, the source has exactly n bytes; the program compares every array with hc12_build_lists's and the
definition's and exits non-zero on a wrong one; a bad access ends it with the sanitizer's report."""
import os
import subprocess

import pytest

from orclib import ROOT

SRC = os.path.join(ROOT, "tests", "emu", "hb_bounds_main.cpp")
EXE = os.path.join(ROOT, "tests", "emu", "_build", "hb_bounds")
# (the runtimes linked statically: the program stands alone, whatever else the environment has the loader bring in)
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def _sanitizers_link(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    return subprocess.run(["g++"] + SAN + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode == 0


def test_hb_stages_stay_inside_their_arrays(tmp_path):
    if not _sanitizers_link(tmp_path):
        pytest.skip("the sanitizer runtimes cannot be linked on this machine")
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DPLZ4_EMU", "-Wno-unused-parameter"] + SAN + ["-o", EXE, SRC])
    run = subprocess.run([EXE], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-6000:]
    assert "lists in pieces: no access outside a buffer, every array hc12_build_lists's and the definition's" in run.stdout
