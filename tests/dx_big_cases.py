"""Raw blocks above 4 MiB on the few-block decoder's big path: the shapes tests/test_dx_big_decode.py (lane-emulated,
tests/emu/emu_dx_big.cpp) and tests/test_gpu_dx_big_decode.py (through the C ABI) share, hand-built blocks that put the stitch's
group borders where they hurt, a hostile-block generator scaled to 5-6 MiB, and the ctypes loader of the emulation.  Test
infrastructure only."""
import ctypes as C
import os
import subprocess

import numpy as np

from lz4blocks import LL, ML, put_len
from orclib import ROOT
from plz4_amd import synth

SRC = os.path.join(ROOT, "tests", "emu", "emu_dx_big.cpp")
SO = os.path.join(ROOT, "tests", "emu", "_build", "libemu_dx_big.so")
DEPS = [SRC, os.path.join(ROOT, "tests", "emu", "dx_train.h")] + \
       [os.path.join(ROOT, "plz4_amd", "csrc", f) for f in ("lz4_dx_device.inl", "lz4_device.inl", "wave.h")]
u8p = C.POINTER(C.c_uint8)

LEFT, UNITS_DISAGREE, LIST_OVERRUN = -999999, -888888, -777777
SEG = 8192                                                   # kDxSeg
DX_MAX_OUT = (4 << 20) + 8                                   # kDxMaxOut

SHAPES = {
    "T4+9": lambda: synth.text(4194313),
    "T16": lambda: synth.text(16777221, seed=3),
    "Z16": lambda: synth.zeros(16777216),
    "R9": lambda: synth.random_bytes(9437185, seed=4),
    "M24": lambda: synth.mixed(24 << 20, 1 << 20),
    "T64": lambda: synth.text(64 << 20, seed=7),
}
_made = {}


def shape(orc, name):
    """(plaintext, compressed) of a named shape, made once per process"""
    if name not in _made:
        src = SHAPES[name]()
        c, comp = orc.compress_fast(src, orc.bound(src.size))
        _made[name] = (src, np.ascontiguousarray(comp[:c]).copy())
    return _made[name]


class DxBigEmu:
    def __init__(self):
        newest = max(os.path.getmtime(p) for p in DEPS)
        if not os.path.exists(SO) or os.path.getmtime(SO) < newest:
            os.makedirs(os.path.dirname(SO), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-parameter", "-o", SO, SRC])
        L = self.L = C.CDLL(SO)
        L.emu_dxb_decode.restype = C.c_int
        L.emu_dxb_decode.argtypes = [u8p, C.c_int, u8p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]

    def set_descending(self, d):
        self.L.emu_dxb_set_descending(int(d))

    def decode(self, comp, cap, group=0, thr=0):
        """-> (size or LEFT, output, {"launched", "taken", "runs", "groups", "room"})"""
        comp = np.ascontiguousarray(comp)
        dst = np.zeros(max(cap, 1), np.uint8)
        out = (C.c_int * 5)()
        r = int(self.L.emu_dxb_decode(comp.ctypes.data_as(u8p) if comp.size else C.cast(None, u8p), comp.size,
                                      dst.ctypes.data_as(u8p), cap, group, thr, out))
        assert r not in (UNITS_DISAGREE, LIST_OVERRUN), r
        return r, dst[:max(r, 0)], dict(zip(("launched", "taken", "runs", "groups", "room"), (int(v) for v in out)))


# ---- blocks built sequence by sequence -------------------------------------------------------------------------------------------
class Builder:
    """An LZ4 block sequence by sequence; the plaintext is kept beside it."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.comp = bytearray()
        self.buf = np.zeros(1 << 16, np.uint8)
        self.n = 0

    def _room(self, k):
        while self.n + k > self.buf.size:
            self.buf = np.concatenate([self.buf, np.zeros(self.buf.size, np.uint8)])

    def _lits(self, ll):
        v = self.rng.integers(0, 256, ll, dtype=np.uint8)
        self._room(ll)
        self.comp += v.tobytes(); self.buf[self.n:self.n + ll] = v; self.n += ll

    def seq(self, ll, ml, off):
        """a sequence of ll literals and a match of ml bytes at distance off (<= 65535, <= the plaintext so far + ll)"""
        self.comp.append((min(ll, 15) << 4) | min(ml - 4, 15))
        if ll >= 15:
            put_len(self.comp, ll - 15)
        self._lits(ll)
        assert 1 <= off <= min(self.n, 65535)
        self.comp += bytes([off & 0xFF, off >> 8])
        if ml - 4 >= 15:
            put_len(self.comp, ml - 4 - 15)
        self._room(ml)
        pat = self.buf[self.n - off:self.n][:ml]
        self.buf[self.n:self.n + ml] = np.tile(pat, ml // pat.size + 1)[:ml]
        self.n += ml

    def pad_to(self, at):
        """plain sequences (3 + ll bytes each) until the next sequence starts at input position `at` exactly"""
        while len(self.comp) < at:
            left = at - len(self.comp)
            assert left >= 3 and (left > 3 or self.n > 0), "cannot land on %d" % at
            ll = 4 if left >= 14 else left - 3
            self.seq(ll, 4 + int(self.rng.integers(0, 12)), 1 + int(self.rng.integers(0, min(self.n + ll, 300))))
        assert len(self.comp) == at

    def end(self, tail):
        """the closing literal run"""
        self.comp.append(min(tail, 15) << 4)
        if tail >= 15:
            put_len(self.comp, tail - 15)
        self._lits(tail)
        return np.frombuffer(bytes(self.comp), np.uint8).copy(), self.buf[:self.n].copy()


SLOW_ML = 19 + 255 * 40 + 7                                  # more length bytes than a table entry looks through (kDxExt = 32)


def slow_at_group_start(group):
    """the chain's first position in group 1 is the group's first position, and the sequence there is one the tables cannot tell"""
    b = Builder(41)
    b.pad_to(group * SEG)
    b.seq(3, SLOW_ML, 2)
    b.pad_to(4 * group * SEG + 100)
    return b.end(30)


def slow_behind_group_border(group):
    """a sequence straddles the border of groups 0 and 1; the first position behind it is slow"""
    b = Builder(42)
    b.pad_to(group * SEG - 5)
    b.seq(14, 9, 7)                                             # 17 bytes from 5 in front of the border
    assert len(b.comp) == group * SEG + 12
    b.seq(0, SLOW_ML, 1)
    b.pad_to(4 * group * SEG + 100)
    return b.end(30)


def early_tail_from_third_last(group):
    """three groups; the sequence that starts in the third-last segment is a literal run to the block's end (the tail unit starts
    there, in front of its own two segments)"""
    nseg = 2 * group + 3                                        # groups 0 and 1 whole, the third has one segment in front of the tail unit
    b = Builder(43)
    b.pad_to((nseg - 3) * SEG + 1000)
    comp, plain = b.end(2 * SEG)
    assert (comp.size + SEG - 1) // SEG == nseg, (comp.size, nseg)
    return comp, plain


def make_big_block(rng, target):
    """A valid block of about `target` plaintext bytes in the manner of lz4blocks.make_block -- lengths and offsets around the vector
    path's boundaries -- with literal runs and matches of up to several hundred KiB between them (the big path's run list)."""
    b = Builder(int(rng.integers(1, 1 << 30)))
    while b.n < target:
        for _ in range(200):
            ll = int(rng.choice(LL)) if rng.random() < 0.7 else int(rng.integers(0, 40))
            ml = int(rng.choice(ML)) if rng.random() < 0.6 else int(rng.integers(4, 40))
            if b.n == 0 and ll == 0:
                ll = 1
            have = b.n + ll
            kind = rng.random()
            cap = 8 if kind < 0.25 else (64 if kind < 0.55 else (2000 if kind < 0.8 else 65535))
            b.seq(ll, ml, int(rng.integers(1, min(have, cap) + 1)))
        k = rng.random()
        if k < 0.4:
            b.seq(int(rng.integers(60000, 400000)), 8, 3)
        elif k < 0.8:
            b.seq(2, int(rng.integers(60000, 700000)), int(rng.choice([1, 2, 7, 4000, 65535])) if b.n > 65535 else 1)
        else:
            b.seq(65536 + 15, 65536, 1)
    return b.end(int(rng.integers(12, 40)))


def damage(comp, rng, kind, at):
    """a damaged copy: kind 0 a bit flip, 1 a byte of 0xFF, 2 a zeroed offset-sized pair, 3 a truncation, near `at`"""
    i = min(max(at + int(rng.integers(0, 64)), 0), comp.size - 2)
    d = comp.copy()
    if kind == 0: d[i] ^= 1 << int(rng.integers(0, 8))
    elif kind == 1: d[i] = 0xFF
    elif kind == 2: d[i:i + 2] = 0
    else: d = d[:i].copy()
    return np.ascontiguousarray(d)
