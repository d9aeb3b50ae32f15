"""The frame writer on hostile recOff tables touches no byte outside what the header lets it read and write:
tests/emu/frame_write_bounds_main.cpp, a program of its own on the lane-emulated device code, built with the address and
undefined-behaviour sanitizers and run as a child process (the sanitizers never enter this process; CPU only).  It checks every info
against a walk of its own, takes every written stream apart again and exits non-zero on a wrong one; a bad access ends it with the
sanitizer's report."""
import os
import subprocess

import pytest

from orclib import ROOT

SRC = os.path.join(ROOT, "tests", "emu", "frame_write_bounds_main.cpp")
EXE = os.path.join(ROOT, "tests", "emu", "_build", "frame_write_bounds")
# (the runtimes linked statically: the program stands alone, whatever else the environment has the loader bring in)
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def _sanitizers_link(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    return subprocess.run(["g++"] + SAN + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode == 0


def test_frame_write_stays_inside_its_buffers(tmp_path):
    if not _sanitizers_link(tmp_path):
        pytest.skip("the sanitizer runtimes cannot be linked on this machine")
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DPLZ4_EMU", "-Wno-unknown-pragmas"] + SAN + ["-o", EXE, SRC])
    run = subprocess.run([EXE], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-6000:]
    assert "no access outside a buffer" in run.stdout
