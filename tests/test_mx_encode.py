"""The few-block level-2 path (plz4_amd/csrc/lz4_mx_device.inl: a block's LZ4MID walk cut into pieces, rounds until every piece
starts from the exact state its predecessor ends in, the gather, the unchanged emit stage) on the lane-emulated build of the same
source: its blocks must be LZ4_compress_HC(level 2)'s of the real liblz4, byte for byte, whatever the piece size, warm-up and order
of the pieces.  Also the restart argument on the walk itself, the path's route function and its workspace layout."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import corpus
from emulib import ENC_SLACK, _check_guard, _guarded
from orclib import ROOT, _ptr, u8p
from plz4_amd import synth

SRC = os.path.join(ROOT, "tests", "emu", "emu_mx.cpp")
SO = os.path.join(ROOT, "tests", "emu", "_build", "libemu_mx.so")
DEPS = [SRC, os.path.join(ROOT, "tests", "emu", "piece_rounds.h")] + [os.path.join(ROOT, "plz4_amd", "csrc", f) for f in (
    "lz4_mx_device.inl", "lz4_fx_device.inl", "lz4_pieces_device.inl", "lz4hc_lazy_device.inl", "lz4_seq_device.inl", "lz4_device.inl", "wave.h", "ws_layout.h", "route.h")]
BSZ = 4 << 20


class MxEmu:
    def __init__(self):
        newest = max(os.path.getmtime(p) for p in DEPS)
        if not os.path.exists(SO) or os.path.getmtime(SO) < newest:
            os.makedirs(os.path.dirname(SO), exist_ok=True)
            tmp = "%s.%d.tmp" % (SO, os.getpid())                    # (several test processes may build at once: the last rename wins)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-parameter", "-o", tmp, SRC])
            os.replace(tmp, SO)
        L = self.L = C.CDLL(SO)
        L.emu_mx_encode.restype = C.c_int
        L.emu_mx_encode.argtypes = [u8p, C.c_int, u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong), C.c_void_p]
        L.emu_mx_whole.restype = C.c_int
        L.emu_mx_whole.argtypes = [u8p, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
        L.emu_mx_restart.restype = C.c_int
        L.emu_mx_restart.argtypes = [u8p, C.c_int, C.c_int]
        L.emu_mx_layout.restype = C.c_int
        L.emu_mx_layout.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong), C.c_int]
        L.emu_mx_route.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
        L.emu_mx_set_descending.argtypes = [C.c_int]

    def encode(self, src, cap, piece=128 << 10, warm=256 << 10, order=0, records=False):
        dst = _guarded(cap, ENC_SLACK)
        st = (C.c_longlong * 6)()
        seq = np.zeros(src.size // 4 + 64, dtype=np.uint64) if records else None
        r = int(self.L.emu_mx_encode(_ptr(src), src.size, _ptr(dst), cap, piece, warm, order, st, seq.ctypes.data if records else None))
        _check_guard(dst, cap, "emu_mx_encode")
        stats = {"rounds": st[0], "again": st[1], "pieces": st[2], "nseq": st[3], "chain": st[4], "walked": st[5]}
        return r, dst[:max(r, 0)], stats, (seq[:st[3]] if records and r >= 0 else None)

    def whole(self, src):
        out = np.zeros(src.size // 4 + 64, dtype=np.uint64)
        la = C.c_int(0)
        r = int(self.L.emu_mx_whole(_ptr(src), src.size, out.ctypes.data, C.byref(la)))
        return out[:r], la.value

    def route(self, env, level, nb, max_len, hc_ex=False, rider=False):
        out = (C.c_int * 7)()
        text = "".join("PLZ4HIP_%s=%s\n" % kv for kv in env.items()).encode()
        self.L.emu_mx_route(text, level, nb, max_len, int(hc_ex), int(rider), out)
        return {"mx": out[0], "piece": out[1], "warm": out[2], "P": out[3], "taken": out[4], "no_staged": out[5], "no_mx": out[6]}


@pytest.fixture(scope="module")
def mx():
    return MxEmu()


def _check(ref, mx, src, caps=None, **kw):
    n = src.size
    bound = n + n // 255 + 16
    st = None
    for cap in caps or (bound,):
        want, wcomp = ref.compress_hc(src, cap, 2)
        r, out, st, _ = mx.encode(src, cap, **kw)
        assert r == want, (n, cap, kw, r, want)
        assert np.array_equal(out, wcomp[:want]), (n, cap, kw)
    return st


def _kind(kind, n):
    return np.ascontiguousarray(synth.make(kind, n, min(max(n, 1), 1 << 16))[:n])


PIECE = 4096
LENGTHS = [0, 1, 12, 13, 14, PIECE - 1, PIECE, PIECE + 1, 8 * PIECE, 5 * PIECE + 7, 5 * PIECE + 11, 5 * PIECE + 12, 100003]


@pytest.mark.parametrize("kind", ["T", "R", "Z", "M"])
def test_mx_lengths_bytes_identical(ref, mx, kind):
    """One below / at kMinLength, around one piece, a multiple of the piece, a last piece shorter than 12 bytes (no search starts in
    it), odd lengths: LZ4_compress_HC's bytes at capacity bound, n and one byte below the compressed size (verdict 0)."""
    for n in LENGTHS:
        src = _kind(kind, n)
        c, _ = ref.compress_hc(src, n + n // 255 + 16, 2)
        caps = [n + n // 255 + 16] + ([n] if n else []) + ([c - 1] if c > 1 else [])
        st = _check(ref, mx, src, caps, piece=PIECE, warm=2 * PIECE)
        assert st["pieces"] == max(1, -(-n // PIECE)), (n, st)


def test_mx_twins(ref, mx):
    for name, src in corpus.twin_cases():
        _check(ref, mx, np.ascontiguousarray(src), piece=16 << 10, warm=16 << 10)


@pytest.mark.parametrize("kind", ["T", "R", "Z", "M"])
def test_mx_1mib(ref, mx, kind):
    src = _kind(kind, 1 << 20)
    c, _ = ref.compress_hc(src, (1 << 20) + 5000, 2)
    _check(ref, mx, src, [(1 << 20) + 5000, 1 << 20, c - 1], piece=32 << 10, warm=64 << 10)


def test_mx_4mib_at_the_defaults(ref, mx):
    """128 KiB pieces, 256 KiB warm-up: a plain restatement of LZ4MID's decision loop, run under the same round rule before the
    kernel code existed, needed two rounds for this kind of text; the kernel code may not need more."""
    st = _check(ref, mx, _kind("T", BSZ))
    assert st["pieces"] == 32 and 1 <= st["rounds"] <= 2, st


def test_mx_tiny_pieces_no_warmup(ref, mx):
    """4 KiB pieces started with no warm-up: nearly every piece walks again -- the same bytes, more rounds."""
    for kind in ("T", "M"):
        src = _kind(kind, 300000)
        st = _check(ref, mx, src, [300000 + 2000, 300000], piece=4096, warm=0)
        assert st["pieces"] == -(-300000 // 4096) and st["rounds"] > 1 and st["again"] > 0, st


def test_mx_piece_order_and_lane_order(ref, mx):
    src = _kind("T", 1 << 20)
    a = _check(ref, mx, src, piece=16 << 10, warm=16 << 10, order=0)
    b = _check(ref, mx, src, piece=16 << 10, warm=16 << 10, order=1)
    assert a == b
    mx.L.emu_mx_set_descending(1)
    try:
        for order in (0, 1):
            _check(ref, mx, corpus.structured(300000, 9), piece=8 << 10, warm=8 << 10, order=order)
    finally:
        mx.L.emu_mx_set_descending(0)


def test_mx_restart_from_saved_states_is_exact(mx):
    """From every saved boundary state a fresh walk gives the records of the unbroken hc_mid_parse."""
    for kind, n, stops in (("T", 256 << 10, 4096), ("T", 1 << 20, 65536 + 333), ("M", 256 << 10, 4096), ("S", 300000, 4096)):
        src = corpus.structured(n, 9) if kind == "S" else _kind(kind, n)
        tried = int(mx.L.emu_mx_restart(_ptr(src), n, stops))
        assert tried > 0, (kind, stops, tried)
        if kind == "T":          # (text has a match every dozen bytes: nearly every boundary has a state of its own)
            assert tried >= (n // stops) * 3 // 4, (kind, stops, tried)


def test_mx_records_are_the_unbroken_walks(mx):
    src = _kind("T", 512 << 10)
    whole, _ = mx.whole(src)
    r, _, st, seq = mx.encode(src, (512 << 10) + 5000, 8 << 10, 0, records=True)
    assert r > 0 and st["rounds"] > 1
    assert np.array_equal(seq, whole)


def test_mx_random_block_is_piece_0_alone(ref, mx):
    src = _kind("R", 1 << 20)
    st = _check(ref, mx, src, piece=64 << 10, warm=64 << 10)
    assert st["chain"] == 1 and st["rounds"] == 1 and st["nseq"] < 64, st


def test_mx_zeros_one_match_crosses_every_piece(ref, mx):
    src = np.zeros(1 << 20, dtype=np.uint8)
    for warm in (0, 64 << 10):
        st = _check(ref, mx, src, [(1 << 20) + 5000, 1 << 20], piece=64 << 10, warm=warm)
        assert st["nseq"] == 1 and st["pieces"] == 16, st


def test_mx_route_edges(mx):
    on = mx.route({}, 2, 512, BSZ)
    assert on == {"mx": 1, "piece": 128 << 10, "warm": 256 << 10, "P": 32, "taken": 1, "no_staged": 0, "no_mx": 0}
    assert mx.route({}, 2, 513, BSZ)["mx"] == 0                               # limit + 1 blocks
    assert mx.route({}, 2, 1, BSZ + 1)["mx"] == 0                             # 4 MiB + 1
    assert mx.route({}, 2, 1, 0)["mx"] == 0
    assert mx.route({}, 2, 1, 128 << 10)["mx"] == 0 and mx.route({}, 2, 1, (128 << 10) + 1)["P"] == 2      # nothing to cut / two pieces
    assert mx.route({}, 2, 4, BSZ, rider=True)["mx"] == 0
    assert mx.route({}, 2, 4, BSZ, hc_ex=True)["mx"] == 0
    assert mx.route({}, 1, 4, BSZ)["mx"] == 0 and mx.route({}, 3, 4, BSZ)["mx"] == 0
    assert mx.route({"MX_MAX_BLOCKS": "0"}, 2, 1, BSZ)["mx"] == 0             # the switch at 0
    two = mx.route({"MX_MAX_BLOCKS": "2", "MX_PIECE_KIB": "8", "MX_WARMUP_KIB": "16"}, 2, 2, 200 * 1024 + 13)
    assert two["mx"] == 1 and two["piece"] == 8192 and two["warm"] == 16384 and two["P"] == 26
    assert mx.route({"MX_MAX_BLOCKS": "2"}, 2, 3, BSZ)["mx"] == 0
    big = {"MX_MAX_BLOCKS": "100000"}                                         # (clamped to what one launch's grid holds)
    assert mx.route(big, 2, 65535, BSZ)["mx"] == 1 and mx.route(big, 2, 65536, BSZ)["mx"] == 0
    # values out of range keep the defaults; warm-up 0 is a value
    odd = mx.route({"MX_PIECE_KIB": "0", "MX_WARMUP_KIB": "5000"}, 2, 1, BSZ)
    assert odd["piece"] == 128 << 10 and odd["warm"] == 256 << 10
    assert mx.route({"MX_WARMUP_KIB": "0"}, 2, 1, BSZ)["warm"] == 0


def test_mx_layout_total_is_the_sum_of_its_parts(mx):
    for per, P, stride in ((1, 1, 1104), (3, 26, 2128), (128, 32, 32848)):
        out = (C.c_longlong * 16)()
        takes = int(mx.L.emu_mx_layout(per, P, stride, out, 16))
        assert takes == 4
        off_meta, off_in, off_out, off_rec, total = out[0:5]
        parts = [(out[5 + 2 * i], out[6 + 2 * i]) for i in range(4)]
        assert [p[0] for p in parts] == [off_meta, off_in, off_out, off_rec]
        nP = per * P
        assert [p[1] for p in parts] == [nP * 48,nP * 32768 * 4, 2 * nP * 32768 * 4, nP * stride * 8]
        end = 0
        for off, size in parts:                                               # in order, no overlap, every array inside the total
            assert off >= end and off + size <= total
            end = off + size
        assert total - end < 256
