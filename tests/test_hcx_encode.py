"""The wave-wide HC parser for blocks of at most 4 KiB under a dictionary context (hcx_compress of
plz4_amd/csrc/lz4hcx_device.inl: the block's lists in LDS, the dictionary's lists of plz4hip_dict_create, one candidate per lane,
sequences written by all lanes) on the lane-emulated build of the same source.  Every case of tests/hcx_cases.py at every level the
parser is built for must be LZ4_compress_HC_continue's under the attached dictionary -- the real liblz4 -- byte for byte and
return value for return value, in both lane orders, and must agree with the one-thread restatement it replaces."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hcx_cases as hc
from emulib import ENC_SLACK, _check_guard, _guarded
from orclib import ROOT, _ptr, u8p

SRC = os.path.join(ROOT, "tests", "emu", "emu_hcx.cpp")
SO = os.path.join(ROOT, "tests", "emu", "_build", "libemu_hcx.so")
DEPS = [SRC] + [os.path.join(ROOT, "plz4_amd", "csrc", f) for f in
                ("lz4hcx_device.inl", "lz4hc_lazy_device.inl", "lz4hc12_device.inl", "lz4hc_device.inl", "lz4_seq_device.inl", "lz4_device.inl", "wave.h")]


class HcxEmu:
    def __init__(self):
        newest = max(os.path.getmtime(p) for p in DEPS)
        if not os.path.exists(SO) or os.path.getmtime(SO) < newest:
            os.makedirs(os.path.dirname(SO), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-parameter", "-o", SO, SRC])
        L = self.L = C.CDLL(SO)
        L.emu_hcx_compress.restype = C.c_int
        L.emu_hcx_compress.argtypes = [u8p, C.c_int, u8p, C.c_int, C.c_int, u8p, C.c_int]
        L.emu_hcx_set_descending.argtypes = [C.c_int]

    def compress(self, src, cap, level, dct, descending=False):
        dst = _guarded(cap, ENC_SLACK)
        nul = C.cast(None, u8p)
        self.L.emu_hcx_set_descending(int(descending))
        try:
            r = int(self.L.emu_hcx_compress(_ptr(src) if src.size else nul, src.size, _ptr(dst), cap, level, _ptr(dct) if dct.size else nul, dct.size))
        finally:
            self.L.emu_hcx_set_descending(0)
        _check_guard(dst, cap, "emu_hcx_compress")
        return r, dst[:max(r, 0)]


@pytest.fixture(scope="module")
def hcx():
    return HcxEmu()


@pytest.fixture(scope="module")
def emu():
    from emulib import Emu
    return Emu()


def test_hcx_levels_and_lds(hcx):
    """The levels the parser is built for are the ones the case list assumes; its LDS lets at least 8 waves share a CU's 160 KiB."""
    assert (hcx.L.emu_hcx_min_level(), hcx.L.emu_hcx_max_level()) == (hc.HCX_LEVELS[0], hc.HCX_LEVELS[-1])
    assert 8 * hcx.L.emu_hcx_lds_bytes() <= 160 << 10
    assert 7 * hcx.L.emu_hcx_mid_lds_bytes() <= 160 << 10               # (level 2's two tables: seven waves)


def _check(ref, hcx, emu, cases):
    streams = {}
    n_checked = 0
    for case in cases:
        d = hc.dict64(case.dct)
        for level in hc.levels_of(case):
            key = (case.dct.ctypes.data, case.dct.size, level)
            if key not in streams:
                keep, daddr = ref.new_dict_ctx_hc(d, level)
                streams[key] = (keep, ref.stream_ctx_hc(level, daddr))
            comp = streams[key][1]
            for cap in hc.caps_of(case):
                want = comp(case.block, cap)
                for desc in (False, True):
                    got = hcx.compress(case.block, cap, level, d, desc)
                    assert got[0] == want[0], (case.name, level, cap, desc, got[0], want[0])
                    assert np.array_equal(got[1], want[1]), (case.name, level, cap, desc)
                if emu is not None:
                    old = emu.compress_hc_dict(case.block, cap, level, d, 2)
                    assert old[0] == want[0] and np.array_equal(old[1], want[1]), (case.name, level, cap, "one-thread restatement")
                n_checked += 1
    return n_checked


def test_hcx_static_cases(ref, hcx, emu):
    assert _check(ref, hcx, emu, hc.static_cases()) > 0


def test_hcx_attempts_budget(ref, hcx, emu):
    """How deep the dictionary's chain is read follows the attempts the own walk took (the builder asserts, with the real
    liblz4, that the three members of a family have three different answers)."""
    assert _check(ref, hcx, emu, hc.budget_cases(ref)) == 9 * 3


def test_hcx_exact_capacities(ref, hcx, emu):
    assert _check(ref, hcx, emu, hc.exact_cap_cases(ref)) > 0


def test_hcx_fuzz(ref, hcx, emu):
    cases = hc.fuzz_cases()
    assert len(cases) == hc.FUZZ_BLOCKS
    assert _check(ref, hcx, emu, cases) >= hc.FUZZ_BLOCKS * len(hc.HCX_LEVELS)
