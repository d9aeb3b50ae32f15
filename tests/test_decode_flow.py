"""The control flow of the decoder's LDS-staged batch (wave_decode_lds_batch, plz4_amd/csrc/lz4_device.inl) on the lane-emulated
build of the same source: the caller primes the window and the staged tail, the token walk makes 22 hops without a test, the
chain cuts are mask arithmetic, and the batch says whether the next one may run.  Crafted blocks (tests/decflow_cases.py) and
seeded random ones decode to the oracle's bytes and return value through both builds of the vector path, at three capacities,
in both lane orders; the batch's counters show that each crafted block did what it is for; and on the bench's text the share of
windows that hold as many tokens as there are hops is what the unconditional walk rests on."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import decflow_cases
from emulib import SENTINEL, _check_guard, _guarded
from lz4blocks import make_block
from orclib import ROOT, _ptr, u8p
from plz4_amd import synth

SRC = os.path.join(ROOT, "tests", "emu", "emu_dec_flow.cpp")
BUILD = os.path.join(ROOT, "tests", "emu", "_build")
DEPS = [SRC] + [os.path.join(ROOT, "plz4_amd", "csrc", f) for f in ("lz4_device.inl", "wave.h")]
CNT = {"batches": 0, "full": 1, "rounds": 2, "coop": 3, "coop_mem": 4, "no_members": 5, "primes": 6, "members": 7}
N_HOPS = 22


class DfEmu:
    def __init__(self):
        so = os.path.join(BUILD, "libemu_df.so")
        newest = max(os.path.getmtime(p) for p in DEPS)
        if not os.path.exists(so) or os.path.getmtime(so) < newest:
            os.makedirs(BUILD, exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-parameter", "-o", so, SRC])
        L = self.L = C.CDLL(so)
        L.emu_df_decode.restype = C.c_int
        L.emu_df_decode.argtypes = [u8p, C.c_int, u8p, C.c_int, C.c_int]
        L.emu_df_set_descending.argtypes = [C.c_int]
        assert L.emu_df_hops() == N_HOPS

    def descending(self, d):
        self.L.emu_df_set_descending(int(d))

    def counters(self):
        """the batch's counters by name; reset on read"""
        cnt = (C.c_ulonglong * 8)()
        self.L.emu_df_counters(cnt)
        return {k: int(cnt[i]) for k, i in CNT.items()}

    def decode(self, comp, cap, lds):
        dst = _guarded(cap, 32)
        r = int(self.L.emu_df_decode(_ptr(comp), comp.size, _ptr(dst), cap, int(lds)))
        _check_guard(dst, cap, "emu_df_decode")
        return r, dst[:max(r, 0)]


@pytest.fixture(scope="module")
def df():
    e = DfEmu()
    yield e
    e.descending(0)


def _check(orc, df, comp, plain):
    """Oracle's bytes and return value through both builds, three capacities, both lane orders; returns the counters of the
    LDS-staged build in ascending order at capacity == size."""
    out = None
    for cap in (plain.size, plain.size + 100, plain.size - 1):
        want, wbytes = orc.decompress_safe(comp, cap)
        if cap >= plain.size:
            assert want == plain.size and np.array_equal(wbytes[:want], plain)
        for desc in (0, 1):
            df.descending(desc)
            for lds in (1, 0):
                df.counters()
                r, got = df.decode(comp, cap, lds)
                cnt = df.counters()
                assert r == want, (cap, desc, lds, r, want)
                assert want <= 0 or np.array_equal(got, wbytes[:want]), (cap, desc, lds)
                if lds == 0:
                    assert cnt["batches"] == 0                    # (the memory version is not the counted routine)
                elif cap == plain.size and desc == 0:
                    out = cnt
    df.descending(0)
    return out


@pytest.mark.parametrize("name", decflow_cases.NAMES)
def test_decode_flow_crafted(orc, df, name):
    comp, plain = decflow_cases.block(name)
    assert 2048 <= comp.size <= 65536
    cnt = _check(orc, df, comp, plain)
    print(name, cnt)
    # the vector path really took the site and the tail behind it, up to the last 1088 bytes of output room (the tail is
    # 220 sequences of 8 bytes: at least (1780 - 1088) / 8 = 86 of them are members)
    assert cnt["members"] >= 86 and cnt["batches"] >= 6, cnt
    assert cnt["primes"] >= 2 and cnt["no_members"] >= 1, cnt
    want = decflow_cases.CASES.get(name, (None, {}))[1]
    for k, v in want.items():
        assert cnt[k] == v, (name, k, cnt)
    if name == "start_below_32":
        # the first batch of the block runs at output position 0 (its matches copy their own literals: a near round)
        # (primed once there and once behind the long literal run, whose token is the one batch without members)
        assert cnt["rounds"] >= 1 and cnt["primes"] == 2 and cnt["no_members"] == 1, cnt
    if name == "input_room_first":
        assert cnt["primes"] == 2 and cnt["no_members"] == 1, cnt


def test_decode_flow_random_blocks(orc, df):
    rng = np.random.default_rng(4242)
    total = 0
    for i in range(200):
        comp, plain = make_block(rng, int(rng.integers(1, 300)))
        cnt = _check(orc, df, comp, plain)
        total += cnt["members"]
    assert total > 2000                                           # (the vector path took its share of them)


def test_decode_flow_hops_on_text_4mib(orc, df):
    """22 hops need no question because no window holds more than 22 tokens; on the bench's 4 MiB T block (the oracle encoder's
    output) this pins how rare even a full walk is, and the batching the figures of DESIGN 3.2 rest on."""
    bsz = 4 << 20
    src = np.ascontiguousarray(synth.make("T", bsz, bsz)[:bsz])
    rec = orc.block_record(src, bsz, True)
    comp = np.ascontiguousarray(rec[4:-4])
    df.descending(0)
    df.counters()
    r, got = df.decode(comp, bsz, 1)
    cnt = df.counters()
    print(cnt)
    assert r == bsz and np.array_equal(got, src)
    with_members = cnt["batches"] - cnt["no_members"]
    assert 25000 <= with_members <= 26000, cnt
    assert cnt["full"] / cnt["batches"] <= 0.02, cnt             # more than 21 tokens: under 2 % of the batches (more than 22: none can)
    assert 14.5 <= cnt["members"] / with_members <= 16.5, cnt
    assert 2.2 <= cnt["rounds"] / with_members <= 2.8, cnt
    # primed at the block's start and behind every sequential step that a batch without members left to (the last batches run
    # out of room instead); 818 sequential steps per block is the figure the cost of an empty pass was weighed with
    assert cnt["primes"] == cnt["no_members"] + 1 and 700 <= cnt["no_members"] <= 900, cnt
