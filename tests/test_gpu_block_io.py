"""Every kernel that shares the priming rule and the record writer of plz4_amd/csrc/lz4_block_io.inl, on the GPU: one list of blocks
(0 B, 13 B, 4096 B and 4097 B of text, 64 KiB of random bytes, 64 KiB of text; records of 64 KiB) through each of them, the route
forced as tests/test_gpu_routes.py forces it -- each case of tests/block_io_cases.py is a child process with the route's switches in
its environment.  (Two routes need more of the call's shape: the few-block route behind which k_fxl_small runs takes calls whose largest
block has at least 65547 bytes, so that case adds one such block and sizes its records to it; a call that is k_hcx's alone has no block
above 4 KiB, so that case takes the list's small blocks and 4 KiB of the random one.)  Block checksums on and off, the block API where the kernel has one.  Bytes and results must equal the oracle's /
the real liblz4's, the random block must be a stored record, and of the counters test_gpu_routes.py reads exactly the route's move."""
import json
import os
import subprocess
import sys

import pytest

import block_io_cases
from orclib import ROOT
from test_gpu_routes import COUNTED

pytestmark = pytest.mark.gpu
CHILD_TIMEOUT = 120
_stop = []                                                          # a child ended by a signal or its time limit: nothing more runs


@pytest.mark.parametrize("name", list(block_io_cases.CASES))
def test_gpu_block_io(name):
    if _stop:
        pytest.fail("not run: %s ended by a signal or its time limit" % _stop[0])
    _, _, switches, moves = block_io_cases.CASES[name]
    env = {k: v for k, v in os.environ.items() if not k.startswith("PLZ4HIP_")}
    env.update(switches)
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "block_io_cases.py"), name], env=env, capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _stop.append(name)
        raise
    if p.returncode < 0:
        _stop.append(name)
    assert p.returncode == 0, (name, p.returncode, p.stderr[-2000:])
    out = json.loads(p.stdout.strip().splitlines()[-1])
    print(name, {k: v for k, v in out["counters"].items() if v})
    assert out["failed"] == [], name
    assert out["stored"], name
    for k in COUNTED:
        assert (out["counters"][k] > 0) == (k in moves), (name, k, out["counters"])
