"""The few-block level-1 path for blocks with history outside the block (the kExt flavour of plz4_amd/csrc/lz4_fx_device.inl:
fxl_prep -- the segment in front of the block, piece 0's entry table -- the rounds of piece parses, the gather, the emit stage with
the segment's catch-up room) on the lane-emulated build of the same source: every block must be LZ4_compress_fast_continue's, byte
for byte and return value for return value, as the oracle's compress_linked / compress_indie_dict restate it -- whatever the
segment, the piece size, the warm-up and the order of pieces and lanes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import corpus
from emulib import ENC_SLACK, _check_guard, _guarded
from orclib import ROOT, _ptr, u8p
from plz4_amd import synth

SRC = os.path.join(ROOT, "tests", "emu", "emu_fxl.cpp")
SO = os.path.join(ROOT, "tests", "emu", "_build", "libemu_fxl.so")
DEPS = [SRC, os.path.join(ROOT, "tests", "emu", "piece_rounds.h")] + [os.path.join(ROOT, "plz4_amd", "csrc", f) for f in (
    "lz4_fx_device.inl", "lz4_pieces_device.inl", "lz4_seq_device.inl", "lz4_device.inl", "wave.h", "ws_layout.h")]
FRESH, LOAD, CTX_COPY, CTX_LOOKUP, NONE = 0, 1, 2, 3, 4           # kDict* (lz4_device.inl)
SIZES = (65547, 65548, 100000, 262161, 1 << 20)


class FxlEmu:
    def __init__(self):
        newest = max(os.path.getmtime(p) for p in DEPS)
        if not os.path.exists(SO) or os.path.getmtime(SO) < newest:
            os.makedirs(os.path.dirname(SO), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-parameter", "-o", SO, SRC])
        L = self.L = C.CDLL(SO)
        L.emu_fxl_encode.restype = C.c_int
        L.emu_fxl_encode.argtypes = [u8p, C.c_int, u8p, C.c_int, C.c_int, C.c_void_p, u8p, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.POINTER(C.c_longlong)]
        L.emu_fxl_set_descending.argtypes = [C.c_int]

    def encode(self, src, cap, tail=None, dct=None, dctx=None, raw=False, piece_kib=64, warm_kib=64, order=0):
        """One block as the kernels prime it (k_encode_rec_dict / k_encode_raw_dict's decision, restated): after `tail` when there
        is one, else under the dictionary context, else a linked frame's first block (raw: the block API, no context)."""
        n = src.size
        seg, table = None, None
        if tail is not None:
            mode = LOAD if tail.size >= 8 else NONE
            seg = tail if mode == LOAD else None
        elif dct is not None:
            d64 = np.ascontiguousarray(dct[-65536:])
            mode = (CTX_COPY if n > 4096 else CTX_LOOKUP) if d64.size >= 8 else NONE
            if mode != NONE:
                seg, table = d64, C.cast(C.byref(dctx), C.c_void_p)
        else:
            mode = NONE if raw else FRESH
        dst = _guarded(cap, ENC_SLACK)
        st = (C.c_longlong * 5)()
        r = int(self.L.emu_fxl_encode(_ptr(src) if n else C.cast(None, u8p), n, _ptr(seg), 0 if seg is None else seg.size, mode, table,
                                      _ptr(dst), cap, piece_kib << 10, warm_kib << 10, order, st))
        _check_guard(dst, cap, "emu_fxl_encode")
        return r, dst[:max(r, 0)], {"rounds": st[0], "again": st[1], "pieces": st[2], "nseq": st[3], "path": st[4]}


@pytest.fixture(scope="module")
def fxl():
    return FxlEmu()


def _kind(kind, n, skip=0):
    return np.ascontiguousarray(synth.make(kind, n + skip, min(n + skip, 1 << 16))[skip:skip + n])


def _check(orc, fxl, src, caps=None, tail=None, dct=None, dctx=None, indie=False, **kw):
    """The block against the oracle at every capacity; caps None: bound, n and around the limitedOutput verdict."""
    n = src.size
    want_of = (lambda cap: orc.compress_indie_dict(src, cap, dctx)) if indie else (lambda cap: orc.compress_linked(src, cap, tail, dctx))
    bound = orc.bound(n)
    if caps is None:
        c, _ = want_of(bound)
        assert c > 0
        caps = [x for x in (bound, n, c - 40, c - 1, c, c + 1, c + 40) if x > 0]
    st = None
    for cap in caps:
        want, wcomp = want_of(cap)
        r, out, st = fxl.encode(src, cap, tail=tail, dct=dct, dctx=dctx, raw=indie, **kw)
        assert r == want, (n, cap, kw, r, want)
        assert np.array_equal(out, wcomp[:want]), (n, cap, kw)
    return st


def _tail_of(prev, ln):
    # (a copy: a tail that ends where the block begins in memory would make the oracle's stream take liblz4's prefix mode)
    return None if ln is None else prev[prev.size - ln:].copy()


@pytest.mark.parametrize("seg", [65536, 30000, 8, 7, None])
def test_fxl_segments_kinds_and_capacities(orc, fxl, seg):
    """Every segment -- full, dictSmall, just loaded, dropped, none -- in front of every size and kind, at the capacities around the
    limitedOutput verdict; the piece size and warm-up go round with the cases."""
    geo = [(64, 64), (16, 16), (4, 0), (1, 1), (16, 0), (4, 4), (1, 0), (64, 0)]
    it = 0
    for n in SIZES:
        for kind in ("T", "M", "Z", "R"):
            prev = _kind(kind, 70000)
            src = _kind(kind, n, 70000)
            pk, wk = geo[it % len(geo)]; it += 1
            if n == (1 << 20) and pk < 4:
                pk, wk = 16, 16
            caps = None if n <= 262161 else [orc.bound(n), n]
            st = _check(orc, fxl, src, caps, tail=_tail_of(prev, seg), piece_kib=pk, warm_kib=wk)
            assert st["path"] == 1 and st["rounds"] <= st["pieces"]


def test_fxl_structured_and_twins(orc, fxl):
    for i, n in enumerate(SIZES):
        whole = corpus.structured(n + 65536, i + 1)
        for seg in (65536, 30000):
            _check(orc, fxl, whole[65536:].copy(), tail=_tail_of(whole[:65536], seg), piece_kib=(1, 4, 16, 64, 16)[i],
                   warm_kib=(0, 4, 16, 64, 0)[i])
    for name, src in corpus.twin_cases():
        # (the block continues the segment's period: matches out of the segment from the block's first bytes on)
        cut = 65536 if name != "Tislands" else 40000
        _check(orc, fxl, src[cut:].copy(), [orc.bound(src.size - cut), src.size - cut], tail=src[:cut].copy(), piece_kib=16, warm_kib=16)


def test_fxl_dictionary_then_linked(orc, fxl):
    """Block 0 against the dictionary context (its table copied), block 1 against block 0's tail; dictionaries of 70 000 (its last
    64 KiB count), 30 000 and 5 bytes (dropped), blocks through the block API as well."""
    text = _kind("T", 70000 + 2 * 262161)
    for dlen in (70000, 30000, 5):
        dct = text[:dlen].copy()
        dctx = orc.dict_ctx(dct)
        b0 = text[70000:70000 + 262161].copy()
        b1 = text[70000 + 262161:].copy()
        for pk, wk in ((64, 64), (4, 0)):
            st = _check(orc, fxl, b0, dct=dct, dctx=dctx, piece_kib=pk, warm_kib=wk)
            assert st["path"] == 1
            _check(orc, fxl, b1, tail=_tail_of(b0, 65536), dct=dct, dctx=dctx, piece_kib=pk, warm_kib=wk)
            _check(orc, fxl, b0, dct=dct, dctx=dctx, indie=True, piece_kib=pk, warm_kib=wk)
        for n in (65547, 100000):
            _check(orc, fxl, np.ascontiguousarray(b0[:n]), dct=dct, dctx=dctx, indie=True, piece_kib=16, warm_kib=16)


def test_fxl_small_blocks_beside_large_ones(orc, fxl):
    """Blocks up to 4 KiB under a dictionary context are not the path's (two tables): they come out of wave_encode_block_dict behind
    the emit stage; every other short block is a block of one piece."""
    text = _kind("T", 400000)
    dct = text[:70000].copy()
    dctx = orc.dict_ctx(dct)
    for n in (0, 5, 12, 13, 4096, 4097, 65546, 200000):
        src = text[100000:100000 + n].copy()
        caps = [orc.bound(n), max(n, 1), max(n // 3, 1)]
        for indie in (False, True):
            st = _check(orc, fxl, src, caps, dct=dct, dctx=dctx, indie=indie, piece_kib=16, warm_kib=16)
            assert st["path"] == (0 if n <= 4096 else 1), (n, st)
        for tail in (_tail_of(text[:100000], 65536), _tail_of(text[:100000], 7), None):
            st = _check(orc, fxl, src, caps, tail=tail, piece_kib=16, warm_kib=16)
            assert st["path"] == 1 and st["pieces"] == max(1, -(-n // 16384))


def test_fxl_matches_out_of_the_segment_and_low_limit(orc, fxl):
    """A block that is a copy of the tail: its first pieces are one match out of the segment (offset > position, the catch-up room
    inside the segment).  A block that repeats its own start at a distance below 64 KiB right behind a segment that would extend
    that match backwards: a candidate in the block stops at the block's first byte (lowLimit)."""
    rnd = _kind("R", 65536)
    for seg in (65536, 30000):
        tail = _tail_of(rnd, seg)
        blk = np.ascontiguousarray(np.concatenate([tail, tail, _kind("T", 40000)]))
        for pk, wk in ((64, 64), (4, 4), (1, 0)):
            _check(orc, fxl, blk, tail=tail, piece_kib=pk, warm_kib=wk)
        # the catch-up: the match is found a few bytes late (its first bytes differ from what the table holds), then runs back
        blk2 = blk.copy(); blk2[:3] = [1, 2, 3]
        _check(orc, fxl, blk2, tail=tail, piece_kib=4, warm_kib=4)
    # lowLimit: segment = ...XYZ, block = A B A' where A' == A and the bytes before A' equal the segment's last bytes
    a = _kind("R", 20000, 7)
    seg = _kind("R", 65536, 123)
    gap = np.ascontiguousarray(np.concatenate([_kind("R", 10000, 999), seg[-64:]]))
    blk = np.ascontiguousarray(np.concatenate([a, gap, a, _kind("T", 30000)]))
    for pk, wk in ((64, 64), (4, 0)):
        _check(orc, fxl, blk, tail=seg, piece_kib=pk, warm_kib=wk)
        _check(orc, fxl, blk, tail=_tail_of(seg, 30000), piece_kib=pk, warm_kib=wk)


def test_fxl_piece_order_and_lane_order(orc, fxl):
    prev, src = _kind("T", 70000), _kind("T", 1 << 20, 70000)
    tail = _tail_of(prev, 65536)
    a = _check(orc, fxl, src, [orc.bound(src.size)], tail=tail, piece_kib=16, warm_kib=16, order=0)
    b = _check(orc, fxl, src, [orc.bound(src.size)], tail=tail, piece_kib=16, warm_kib=16, order=1)
    assert a == b
    fxl.L.emu_fxl_set_descending(1)
    try:
        whole = corpus.structured(300000 + 65536, 9)
        for order in (0, 1):
            _check(orc, fxl, whole[65536:].copy(), tail=_tail_of(whole[:65536], 65536), piece_kib=4, warm_kib=4, order=order)
            _check(orc, fxl, whole[65536:].copy(), tail=_tail_of(whole[:65536], 30000), piece_kib=1, warm_kib=0, order=order)
    finally:
        fxl.L.emu_fxl_set_descending(0)


def test_fxl_tiny_pieces_no_warmup(orc, fxl):
    prev = _kind("T", 70000)
    src = _kind("T", 300000, 70000)
    st = _check(orc, fxl, src, [orc.bound(src.size), src.size], tail=_tail_of(prev, 65536), piece_kib=1, warm_kib=0)
    assert st["pieces"] == (300000 + 1023) // 1024
    assert 2 < st["rounds"] <= st["pieces"] and st["again"] > 0, st


def test_fxl_4mib_behind_a_full_segment(orc, fxl):
    """One 4 MiB block of text behind 64 KiB at the default 64 / 64: indices above 2^22, the 9-bit tags and 22-bit record positions.
    DESIGN 3.10a quotes the rounds and the pieces parsed again from here."""
    prev = _kind("T", 70000)
    src = _kind("T", 4 << 20, 70000)
    st = _check(orc, fxl, src, [orc.bound(src.size), src.size], tail=_tail_of(prev, 65536))
    print("4 MiB T behind 64 KiB, 64 / 64:", st)
    assert st["pieces"] == 64 and st["rounds"] <= st["pieces"], st
    dct = np.ascontiguousarray(prev)
    st = _check(orc, fxl, src, [orc.bound(src.size)], dct=dct, dctx=orc.dict_ctx(dct))
    assert st["rounds"] <= st["pieces"], st


def test_fxl_fuzz_corpus_1mib_behind_a_segment(orc, fxl, monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "tests", "fuzz"))
    import fuzz_encode
    monkeypatch.setenv("FUZZ_MAXN", str(1 << 20))
    rng = np.random.default_rng(2025)
    for it in range(8):
        whole = np.ascontiguousarray(fuzz_encode.make(rng, it))
        seg = (65536, 30000, 8)[it % 3]
        src = whole[seg:].copy()
        _check(orc, fxl, src, [orc.bound(src.size), src.size], tail=whole[:seg].copy(), piece_kib=(4, 16, 64)[it % 3],
               warm_kib=(0, 8, 64)[it % 3])
