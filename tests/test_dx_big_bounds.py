"""The few-block decoder's big path on hostile blocks of 5-6 MiB touches no byte outside its buffers and its workspaces:
tests/emu/dx_big_bounds_main.cpp, a program of its own on the lane-emulated device code, built with the address and
undefined-behaviour sanitizers and run as a child process (the sanitizers never enter this process; CPU only).  It allocates exactly
what launch_decode reserves for the path, checks every answer against the oracle and exits non-zero on a wrong one or on a run list
beyond its reserved count; a bad access ends it with the sanitizer's report."""
import os
import subprocess

import pytest

from orclib import ROOT

SRC = os.path.join(ROOT, "tests", "emu", "dx_big_bounds_main.cpp")
ORACLE = os.path.join(ROOT, "oracle", "plz4_oracle.c")
EXE = os.path.join(ROOT, "tests", "emu", "_build", "dx_big_bounds")
# (the runtimes linked statically: the program stands alone, whatever else the environment has the loader bring in)
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def _sanitizers_link(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    return subprocess.run(["g++"] + SAN + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode == 0


def test_big_path_stays_inside_its_buffers(tmp_path):
    if not _sanitizers_link(tmp_path):
        pytest.skip("the sanitizer runtimes cannot be linked on this machine")
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DPLZ4_EMU"] + SAN + ["-o", EXE, SRC, "-x", "c", ORACLE])
    run = subprocess.run([EXE], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-6000:]
    assert "no access outside a buffer" in run.stdout
