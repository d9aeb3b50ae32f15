"""The emit stage's LDS-free pieces (plz4_amd/csrc/lz4_device.inl) on the lane-emulated build of the same source:
wave_xxh32_x16 -- sixteen buffers' xxh32 chains in one wave, four lanes each, the loads pipelined in registers -- against the oracle's
xxh32, and wave_scan_lengths -- the one-wave scan behind k_scan / k_scan_from -- against numpy.cumsum.  Reads past a buffer's end are
the business of tests/emu/xxh16_bounds_main.cpp (a program of its own under the address sanitizer, scripts/README.md)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from orclib import ROOT, Oracle

SRC = os.path.join(ROOT, "tests", "emu", "emu_xxh16.cpp")
BUILD = os.path.join(ROOT, "tests", "emu", "_build")
DEPS = [SRC] + [os.path.join(ROOT, "plz4_amd", "csrc", f) for f in ("lz4_device.inl", "wave.h")]
# (2047 .. 2064: around twice the ring's depth of 64 stripes, where its refill loop first runs)
LENGTHS = [0, 1, 15, 16, 17, 31, 32, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 2063, 2064, 100003]
COUNTS = [1, 15, 16, 17, 33]


class X16Emu:
    def __init__(self):
        so = os.path.join(BUILD, "libemu_xxh16.so")
        newest = max(os.path.getmtime(p) for p in DEPS)
        if not os.path.exists(so) or os.path.getmtime(so) < newest:
            os.makedirs(BUILD, exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-parameter", "-o", so, SRC])
        L = self.L = C.CDLL(so)
        L.emu_x16_hash.restype = C.c_int
        L.emu_x16_hash.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_uint32)]
        L.emu_x16_scan.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.emu_x16_set_descending.argtypes = [C.c_int]

    def hash(self, bufs):
        """bufs: uint8 views (any start alignment); -> their digests, sixteen to an emulated wave"""
        k = len(bufs)
        ptrs = (C.c_void_p * k)(*[b.ctypes.data if b.size else None for b in bufs])
        lens = (C.c_int * k)(*[b.size for b in bufs])
        out = (C.c_uint32 * k)()
        waves = self.L.emu_x16_hash(ptrs, lens, k, out)
        assert waves == (k + 15) // 16
        return [int(v) for v in out]

    def scan(self, lens, first, clamp, start=0):
        n = lens.size
        off = np.full(n + 1, -77, dtype=np.int64)
        off[0] = start
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        self.L.emu_x16_scan(lens.ctypes.data if n else None, off.ctypes.data, n, first, clamp)
        return off


@pytest.fixture(scope="module")
def emu():
    e = X16Emu()
    yield e
    e.L.emu_x16_set_descending(0)


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.fixture(scope="module")
def pool():
    return np.random.default_rng(16).integers(0, 256, size=(1 << 20) + 64, dtype=np.uint8)


def _views(pool, lengths, align0):
    """one view per length, back to back in the pool from a start that is `align0` modulo 16 (records lie back to back in a body)"""
    base = (-pool.ctypes.data) % 16 + align0
    out, pos = [], base
    for n in lengths:
        out.append(pool[pos:pos + n])
        pos += n
    assert pos <= pool.size
    return out


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("descending", [0, 1])
def test_x16_against_oracle(emu, orc, pool, count, descending):
    emu.L.emu_x16_set_descending(descending)
    rng = np.random.default_rng(1000 + count)
    for align0 in range(16):
        # every length of the set shows up across the offsets; one long buffer beside short and empty ones in each wave
        lengths = [LENGTHS[(align0 + 5 * i) % len(LENGTHS)] for i in range(count)]
        if count >= 15:
            lengths[int(rng.integers(0, count))] = 100003
        bufs = _views(pool, lengths, align0)
        assert bufs[0].ctypes.data % 16 == align0 or bufs[0].size == 0
        got = emu.hash(bufs)
        want = [orc.xxh32(b) for b in bufs]
        assert got == want, (count, align0, lengths)


def test_x16_every_length_at_every_offset(emu, orc, pool):
    for align0 in range(16):
        bufs = _views(pool, LENGTHS, align0)                 # 22 buffers: two waves, the second with six groups
        assert emu.hash(bufs) == [orc.xxh32(b) for b in bufs]


def test_x16_same_length_everywhere(emu, orc, pool):
    # all sixteen groups leave every loop together
    for n in (0, 16, 1024, 2048, 2064, 4099):
        bufs = _views(pool, [n] * 16, 3)
        assert emu.hash(bufs) == [orc.xxh32(b) for b in bufs]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1025, 4097])
@pytest.mark.parametrize("first", [0, 1])
def test_scan_against_cumsum(emu, n, first):
    rng = np.random.default_rng(n * 2 + first)
    lens = rng.integers(1, 4 << 20, size=n, dtype=np.int64).astype(np.int32)
    if n:
        lens[rng.integers(0, n, size=max(1, n // 7))] = 0
        lens[rng.integers(0, n, size=max(1, n // 9))] = -7            # an engine failure code: counts as 0
    start = 0 if first else (1 << 33) + 12345                            # what the part before left in off[0]
    off = emu.scan(lens, first, 1, start=-5 if first else start)        # (first: off[0] is not read)
    want = np.zeros(n + 1, dtype=np.int64)
    want[1:] = np.cumsum(np.maximum(lens.astype(np.int64), 0))
    assert np.array_equal(off, want + start)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1025, 4097])
def test_scan_plain(emu, n):
    # k_scan: from 0, the lengths as they are; totals beyond 32 bits
    lens = np.random.default_rng(n).integers(0, 0x7E000000, size=n, dtype=np.int64).astype(np.int32)
    off = emu.scan(lens, 1, 0, start=-5)
    want = np.zeros(n + 1, dtype=np.int64)
    want[1:] = np.cumsum(lens.astype(np.int64))
    assert np.array_equal(off, want)
