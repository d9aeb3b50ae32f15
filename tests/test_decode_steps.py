"""The near steps of the decoder's LDS-staged batch (wave_decode_lds_batch, plz4_amd/csrc/lz4_device.inl) on the lane-emulated
build of the same source: near matches are copied one by one in sequence order, with no dependency rounds.  Crafted blocks
(tests/decsteps_cases.py) and seeded random ones whose matches are mostly near decode to the oracle's bytes and return value
through both builds of the vector path, at three capacities, in both lane orders; the step counters show that every crafted site
made one step per simple near match; and on the bench's text the steps per batch are the figure the step's form was chosen by."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import decsteps_cases
from emulib import _check_guard, _guarded
from orclib import ROOT, _ptr, u8p
from plz4_amd import synth

SRC = os.path.join(ROOT, "tests", "emu", "emu_dec_steps.cpp")
BUILD = os.path.join(ROOT, "tests", "emu", "_build")
DEPS = [SRC] + [os.path.join(ROOT, "plz4_amd", "csrc", f) for f in ("lz4_device.inl", "wave.h")]
CNT = {"batches": 0, "full": 1, "rounds": 2, "coop": 3, "coop_mem": 4, "no_members": 5, "primes": 6, "members": 7}
STEPS = {"steps": 0, "noop": 1, "max_steps": 2, "step_batches": 3}


class DsEmu:
    def __init__(self):
        so = os.path.join(BUILD, "libemu_ds.so")
        newest = max(os.path.getmtime(p) for p in DEPS)
        if not os.path.exists(so) or os.path.getmtime(so) < newest:
            os.makedirs(BUILD, exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-parameter", "-o", so, SRC])
        L = self.L = C.CDLL(so)
        L.emu_ds_decode.restype = C.c_int
        L.emu_ds_decode.argtypes = [u8p, C.c_int, u8p, C.c_int, C.c_int]
        L.emu_ds_set_descending.argtypes = [C.c_int]

    def descending(self, d):
        self.L.emu_ds_set_descending(int(d))

    def counters(self):
        """the batch's counters and the step counters by name; reset on read"""
        cnt = (C.c_ulonglong * 8)(); st = (C.c_ulonglong * 4)()
        self.L.emu_ds_counters(cnt, st)
        out = {k: int(cnt[i]) for k, i in CNT.items()}
        out.update({k: int(st[i]) for k, i in STEPS.items()})
        return out

    def decode(self, comp, cap, lds):
        dst = _guarded(cap, 32)
        r = int(self.L.emu_ds_decode(_ptr(comp), comp.size, _ptr(dst), cap, int(lds)))
        _check_guard(dst, cap, "emu_ds_decode")
        return r, dst[:max(r, 0)]


@pytest.fixture(scope="module")
def ds():
    e = DsEmu()
    yield e
    e.descending(0)


def _check(orc, ds, comp, plain):
    """Oracle's bytes and return value through both builds, three capacities, both lane orders; returns the counters of the
    LDS-staged build in ascending order at capacity == size."""
    out = None
    for cap in (plain.size, plain.size + 100, plain.size - 1):
        want, wbytes = orc.decompress_safe(comp, cap)
        if cap >= plain.size:
            assert want == plain.size and np.array_equal(wbytes[:want], plain)
        for desc in (0, 1):
            ds.descending(desc)
            for lds in (1, 0):
                ds.counters()
                r, got = ds.decode(comp, cap, lds)
                cnt = ds.counters()
                assert r == want, (cap, desc, lds, r, want)
                assert want <= 0 or np.array_equal(got, wbytes[:want]), (cap, desc, lds)
                if lds == 0:
                    assert cnt["batches"] == 0 and cnt["steps"] == 0 and cnt["noop"] == 0      # (the memory version makes no steps)
                elif cap == plain.size and desc == 0:
                    out = cnt
    ds.descending(0)
    return out


def _check_noops(ds, cnt):
    """Every step follows a question of its own (`while (run)`), so no step is made without a match."""
    assert cnt["noop"] == 0, cnt


@pytest.mark.parametrize("name", decsteps_cases.NAMES)
def test_decode_steps_crafted(orc, ds, name):
    comp, plain = decsteps_cases.block(name)
    assert 2048 <= comp.size <= 65536
    cnt = _check(orc, ds, comp, plain)
    print(name, cnt)
    site, near, coop = decsteps_cases.CASES[name]
    # the vector path really took the site and the tail behind it (tests/test_decode_flow.py: at least 86 of the tail's sequences)
    assert cnt["members"] >= 86 and cnt["batches"] >= 6, cnt
    assert cnt["steps"] == near and cnt["coop"] == coop, cnt
    if name == "own_12":                                              # (108 input bytes: the site is two batches)
        assert cnt["step_batches"] == 2 and 6 <= cnt["max_steps"] < near, cnt
    else:
        assert cnt["step_batches"] == (near > 0) and cnt["max_steps"] == near, cnt
    if name.startswith("chain_"):
        assert cnt["rounds"] == near, cnt                             # a chain: every near match was a round of its own
    if name in ("own_6", "fill_16"):
        # ... and so were these, although the six depend on nobody: the rounds' rule asked for a source that ends before the
        # first pending match's output, which a match that copies its own literals never has
        assert cnt["rounds"] == near, cnt
    _check_noops(ds, cnt)


def test_decode_steps_random_blocks(orc, ds):
    steps = members = 0
    for i in range(decsteps_cases.N_RANDOM):
        comp, plain = decsteps_cases.random_block(i)
        cnt = _check(orc, ds, comp, plain)
        _check_noops(ds, cnt)
        steps += cnt["steps"]; members += cnt["members"]
    print(steps, members)
    # HEAD and TAIL aside, most matches are near: 300 blocks of 210 site sequences on average, 11 in 12 of them short
    assert steps > 30000 and members > steps, (steps, members)


def test_decode_steps_on_text_4mib(orc, ds):
    """The bench's 4 MiB T block (the oracle encoder's output): 3.68 simple near matches per batch with members is the figure the
    step's estimate rests on (scripts/sim_decode_batches.py prints their histogram)."""
    bsz = 4 << 20
    src = np.ascontiguousarray(synth.make("T", bsz, bsz)[:bsz])
    rec = orc.block_record(src, bsz, True)
    comp = np.ascontiguousarray(rec[4:-4])
    ds.descending(0)
    ds.counters()
    r, got = ds.decode(comp, bsz, 1)
    cnt = ds.counters()
    print(cnt)
    assert r == bsz and np.array_equal(got, src)
    with_members = cnt["batches"] - cnt["no_members"]
    assert 25000 <= with_members <= 26000, cnt
    assert 3.4 <= cnt["steps"] / with_members <= 4.0, cnt
    assert cnt["max_steps"] <= 22, cnt                              # (a window holds no more than 22 tokens)
    _check_noops(ds, cnt)
