"""The few-block level-2 parse behind an external segment touches no byte outside its buffers: tests/emu/mxl_bounds_main.cpp, a
program of its own on the lane-emulated device code, built with the address and undefined-behaviour sanitizers and run as a child
process (the sanitizers never enter this process; CPU only).  The plaintext is exactly segment + block, every workspace array exactly
what piece_layout plans; per segment length the program checks every block's records against the unbroken hc_mid_parse<true> and
exits non-zero on a wrong one; a bad access ends it with the sanitizer's report."""
import os
import subprocess

import pytest

from orclib import ROOT

SRC = os.path.join(ROOT, "tests", "emu", "mxl_bounds_main.cpp")
EXE = os.path.join(ROOT, "tests", "emu", "_build", "mxl_bounds")
# (the runtimes linked statically: the program stands alone, whatever else the environment has the loader bring in)
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
SEGMENTS = (0, 3, 7, 8, 9, 100, 4096, 65535, 65536)


def _sanitizers_link(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    return subprocess.run(["g++"] + SAN + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode == 0


def test_mxl_rounds_stay_inside_their_buffers(tmp_path):
    if not _sanitizers_link(tmp_path):
        pytest.skip("the sanitizer runtimes cannot be linked on this machine")
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DPLZ4_EMU", "-Wno-unused-parameter"] + SAN + ["-o", EXE, SRC])
    run = subprocess.run([EXE], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-6000:]
    for seg in SEGMENTS:
        assert any(line.startswith("segment %d: " % seg) and line.endswith("0 wrong: no access outside a buffer, every block the unbroken walk's")
                   for line in run.stdout.splitlines()), seg
