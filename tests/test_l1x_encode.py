"""The bulk level-1 path for blocks with history outside the block (l1x_block of plz4_amd/csrc/lz4_fx_device.inl: the segment where
it lies, the starting table built in the wave's own table, one exact whole-block run of the kExt parse; then the kSeg emit stage) on
the lane-emulated build of the same source, over linked calls on CONTIGUOUS plaintext -- block i's segment is the tail of block
i - 1, in place.  Every block must be LZ4_compress_fast_continue's, byte for byte and return value for return value, as the oracle's
compress_linked restates it, in both lane orders, and the source must come back untouched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from emulib import ENC_SLACK, SENTINEL
from orclib import ROOT, _ptr, u8p
from plz4_amd import synth

SRC = os.path.join(ROOT, "tests", "emu", "emu_l1x.cpp")
SO = os.path.join(ROOT, "tests", "emu", "_build", "libemu_l1x.so")
DEPS = [SRC] + [os.path.join(ROOT, "plz4_amd", "csrc", f) for f in ("lz4_fx_device.inl", "lz4_seq_device.inl", "lz4_device.inl", "lz4_block_io.inl", "wave.h")]
PAD = 65536                                                            # the scratch in front of block 0
i32p = C.POINTER(C.c_int)


class L1xEmu:
    def __init__(self):
        newest = max(os.path.getmtime(p) for p in DEPS)
        if not os.path.exists(SO) or os.path.getmtime(SO) < newest:
            os.makedirs(os.path.dirname(SO), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-parameter", "-o", SO, SRC])
        L = self.L = C.CDLL(SO)
        L.emu_l1x_encode.restype = C.c_int
        L.emu_l1x_encode.argtypes = [C.c_void_p, C.c_longlong, C.c_int, u8p, C.c_int, C.c_void_p, C.c_int, u8p, C.c_int,
                                     u8p, C.c_longlong, i32p, C.c_int]
        L.emu_l1x_set_descending.argtypes = [C.c_int]

    def encode(self, buf, total, bsz, dct=None, dctx=None, prev_tail=None, order=0):
        """buf: PAD bytes of scratch, `total` bytes of plaintext, room to read past the end.  Returns the blocks' (ret, bytes)."""
        nb = -(-total // bsz)
        stride = bsz + ENC_SLACK                                         # block i's capacity is bsz: sentinel bytes behind it
        dst = np.full(max(nb, 1) * stride, SENTINEL, dtype=np.uint8)
        res = np.zeros(max(nb, 1), dtype=np.int32)
        d64 = None if dct is None else np.ascontiguousarray(dct[-65536:])
        null = C.cast(None, u8p)
        rc = self.L.emu_l1x_encode(buf.ctypes.data + PAD, total, bsz, null if d64 is None or not d64.size else _ptr(d64),
                                   0 if d64 is None else d64.size, None if dctx is None else C.cast(C.byref(dctx), C.c_void_p),
                                   int(dct is not None), null if prev_tail is None or not prev_tail.size else _ptr(prev_tail),
                                   -1 if prev_tail is None else prev_tail.size, _ptr(dst), stride, res.ctypes.data_as(i32p), order)
        assert rc == 0, rc
        for i in range(nb):
            assert np.all(dst[i * stride + bsz:(i + 1) * stride] == SENTINEL), "emu_l1x_encode wrote past block %d's capacity of %d" % (i, bsz)
        return [(int(res[i]), dst[i * stride:i * stride + max(int(res[i]), 0)].copy()) for i in range(nb)]


@pytest.fixture(scope="module")
def l1x():
    return L1xEmu()


_TEXT = {}


def _plain(kind, n, seed):
    key = (kind, seed)
    if key not in _TEXT:
        _TEXT[key] = synth.make(kind, (5 * 256 << 10) + 70000, 1 << 16, seed=seed)
    return _TEXT[key][70000:70000 + n]


def _want(orc, plain, bsz, dctx, prev_tail):
    out, prev = [], None
    for o in range(0, plain.size, bsz):
        b = plain[o:o + bsz].copy()
        tail = prev_tail if o == 0 else prev[-65536:].copy()
        out.append(orc.compress_linked(b, bsz, None if tail is None else tail.copy(), dctx if tail is None else None))
        prev = b
    return out


STARTS = ["fresh", "dict70000", "dict30000", "dict5", "tail0", "tail7", "tail8", "tail65536"]


def _start(orc, start):
    """(dct, dctx, prev_tail) of block 0."""
    user = synth.text(70000, seed=42)
    if start.startswith("dict"):
        dct = user[:int(start[4:])].copy()
        return dct, orc.dict_ctx(dct), None
    if start.startswith("tail"):
        n = int(start[4:])
        return None, None, np.ascontiguousarray(synth.make("M", 70000, 1 << 16, seed=5)[70000 - n:]).copy()
    return None, None, None


@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("bsz", [64 << 10, 256 << 10])
def test_l1x_linked_contiguous(orc, l1x, bsz, start):
    """1, 2 and 5 blocks, the last one of 1, 12, 13, 4097 and bsz bytes, behind every start of block 0, first block first in ascending
    lane order and last block first in descending lane order; the plaintext is the same afterwards."""
    dct, dctx, prev_tail = _start(orc, start)
    it = 0
    for nb in (1, 2, 5):
        for last in (1, 12, 13, 4097, bsz):
            total = (nb - 1) * bsz + last
            plain = _plain("TM"[it % 2], total, seed=11 + it % 3); it += 1
            want = _want(orc, plain, bsz, dctx, prev_tail)
            for order in (0, 1):
                buf = np.full(PAD + total + 256, 0xA7, dtype=np.uint8)
                buf[PAD:PAD + total] = plain
                l1x.L.emu_l1x_set_descending(order)
                try:
                    got = l1x.encode(buf, total, bsz, dct=dct, dctx=dctx, prev_tail=prev_tail, order=order)
                finally:
                    l1x.L.emu_l1x_set_descending(0)
                assert [g[0] for g in got] == [w[0] for w in want], (bsz, start, nb, last, order)
                for i, (g, w) in enumerate(zip(got, want)):
                    assert np.array_equal(g[1], w[1][:w[0]]), (bsz, start, nb, last, order, i)
                assert np.array_equal(buf[PAD:PAD + total], plain) and np.all(buf[PAD + total:] == 0xA7), (bsz, start, nb, last)
                if start in ("fresh", "dict5", "tail0", "tail7"):
                    assert np.all(buf[:PAD] == 0xA7)                     # (no segment: the scratch is not touched either)


def test_l1x_prev_tail_in_place(orc, l1x):
    """A call that continues one big buffer: prevTail is the 64 KiB in front of src, nothing is copied, the bytes are those of the
    whole buffer's blocks."""
    bsz = 64 << 10
    plain = _plain("T", 4 * bsz + 4097, seed=12)
    want = _want(orc, plain, bsz, None, None)
    buf = np.full(PAD + plain.size + 256, 0xA7, dtype=np.uint8)
    buf[PAD:PAD + plain.size] = plain
    k = 2
    view = buf[k * bsz:]                                                 # (its PAD bytes in front of block k are block k - 1's tail)
    got = l1x.encode(view, plain.size - k * bsz, bsz, prev_tail=view[PAD - 65536:PAD])
    assert [(g[0], g[1].tobytes()) for g in got] == [(w[0], w[1][:w[0]].tobytes()) for w in want[k:]]
    assert np.array_equal(buf[PAD:PAD + plain.size], plain) and np.all(buf[:PAD] == 0xA7)
