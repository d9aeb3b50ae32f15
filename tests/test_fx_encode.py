"""The few-block level-1 path (plz4_amd/csrc/lz4_fx_device.inl: a block's parse cut into pieces, rounds until every piece starts
from the exact state its predecessor ends in, the gather, the unchanged emit stage) on the lane-emulated build of the same source:
its blocks must be LZ4_compress_fast's, byte for byte, whatever the piece size, warm-up and order of the pieces.  Also the restart
argument itself, on a plain restatement of liblz4's byU32 parse: chained through saved post-match states it gives the unbroken
parse's sequences."""
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

SRC = os.path.join(ROOT, "tests", "emu", "emu_fx.cpp")
SO = os.path.join(ROOT, "tests", "emu", "_build", "libemu_fx.so")
DEPS = [SRC, os.path.join(ROOT, "tests", "emu", "piece_rounds.h")] + [os.path.join(ROOT, "plz4_amd", "csrc", f) for f in (
    "lz4_fx_device.inl", "lz4_pieces_device.inl", "lz4_seq_device.inl", "lz4_device.inl", "wave.h", "ws_layout.h")]
N_MIN = 65547          # liblz4's byU32 tables from here on (lz4.c:1389)


class FxEmu:
    def __init__(self):
        newest = max(os.path.getmtime(p) for p in DEPS)
        if not os.path.exists(SO) or os.path.getmtime(SO) < newest:
            os.makedirs(os.path.dirname(SO), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-parameter", "-o", SO, SRC])
        L = self.L = C.CDLL(SO)
        L.emu_fx_encode.restype = C.c_int
        L.emu_fx_encode.argtypes = [u8p, C.c_int, u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong), C.c_void_p]
        L.emu_fx_sim.restype = C.c_int
        L.emu_fx_sim.argtypes = [u8p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.emu_fx_set_descending.argtypes = [C.c_int]

    def encode(self, src, cap, piece_kib=64, warm_kib=64, order=0, records=False):
        dst = _guarded(cap, ENC_SLACK)
        st = (C.c_longlong * 4)()
        seq = np.zeros(src.size // 4 + 2, dtype=np.uint64) if records else None
        r = int(self.L.emu_fx_encode(_ptr(src), src.size, _ptr(dst), cap, piece_kib << 10, warm_kib << 10, order, st,
                                     seq.ctypes.data if records else None))
        _check_guard(dst, cap, "emu_fx_encode")
        stats = {"rounds": st[0], "again": st[1], "pieces": st[2], "nseq": st[3]}
        return r, dst[:max(r, 0)], stats, (seq[:st[3]] if records and r >= 0 else None)

    def sim(self, src, stops):
        out = np.zeros(src.size // 4 + 2, dtype=np.uint64)
        la = C.c_int(0)
        r = int(self.L.emu_fx_sim(_ptr(src), src.size, stops, out.ctypes.data, out.size, C.byref(la)))
        assert r >= 0
        return out[:r], la.value


@pytest.fixture(scope="module")
def fx():
    return FxEmu()


def _check(orc, fx, src, caps=None, **kw):
    n = src.size
    bound = orc.bound(n)
    c, comp = orc.compress_fast(src, bound)
    assert c > 0
    for cap in caps or (bound,):
        want, wcomp = orc.compress_fast(src, cap)
        r, out, st, _ = fx.encode(src, cap, **kw)
        assert r == want, (n, cap, kw, r, want)
        assert np.array_equal(out, wcomp[:want]), (n, cap, kw)
    return st


def _kind(kind, n):
    return np.ascontiguousarray(synth.make(kind, n, min(n, 1 << 16))[:n])


def test_fx_restart_from_saved_states_is_exact(fx):
    for kind in ("T", "M"):
        src = _kind(kind, 1 << 20)
        whole, la = fx.sim(src, 0)
        for stops in (1024, 16 << 10, 65536 + 333):
            chained, la2 = fx.sim(src, stops)
            assert la2 == la and np.array_equal(chained, whole), (kind, stops)


def test_fx_records_equal_the_simulated_parse(orc, fx):
    src = _kind("T", 1 << 20)
    whole, _ = fx.sim(src, 0)
    r, _, st, seq = fx.encode(src, orc.bound(src.size), 16, 16, records=True)
    assert r > 0 and st["rounds"] > 1
    # (the simulator keeps the probe position; the wave parser's records are the same triples)
    assert np.array_equal(seq, whole)


@pytest.mark.parametrize("n", [N_MIN, 1 << 20, 4 << 20])
def test_fx_kinds_bytes_identical(orc, fx, n):
    for kind in ("T", "M", "Z", "R"):
        src = _kind(kind, n)
        c, _ = orc.compress_fast(src, orc.bound(n))
        caps = [orc.bound(n), n]
        if n < (4 << 20):
            caps += [c - 40, c - 1, c, c + 1, c + 40]          # around the limitedOutput verdict
        _check(orc, fx, src, [x for x in caps if x > 0])


def test_fx_structured_and_twins(orc, fx):
    for n, seed in ((N_MIN, 1), (N_MIN + 1, 2), (100000, 3), (262144 + 17, 4), (1 << 20, 5)):
        src = corpus.structured(n, seed)
        c, _ = orc.compress_fast(src, orc.bound(n))
        _check(orc, fx, src, [orc.bound(n), n, c - 40, c + 40], piece_kib=16, warm_kib=16)
    for name, src in corpus.twin_cases():
        if src.size >= N_MIN:
            _check(orc, fx, np.ascontiguousarray(src), piece_kib=16, warm_kib=16)


def test_fx_piece_order_and_lane_order(orc, fx):
    src = _kind("T", 1 << 20)
    a = _check(orc, fx, src, piece_kib=16, warm_kib=16, order=0)
    b = _check(orc, fx, src, piece_kib=16, warm_kib=16, order=1)
    assert a == b
    fx.L.emu_fx_set_descending(1)
    try:
        _check(orc, fx, corpus.structured(300000, 9), piece_kib=8, warm_kib=8)
    finally:
        fx.L.emu_fx_set_descending(0)


def test_fx_tiny_pieces_no_warmup(orc, fx):
    """1 KiB pieces started with no warm-up: many rounds, pieces crossed by one search or one match (no post-match state of their
    own), guessed starts next to the block's end."""
    for kind in ("T", "M", "Z", "R"):
        src = _kind(kind, 300000)
        st = _check(orc, fx, src, [orc.bound(src.size), src.size], piece_kib=1, warm_kib=0)
        assert st["pieces"] == (300000 + 1023) // 1024
        if kind in ("T", "M"):
            assert st["rounds"] > 2 and st["again"] > 0
    st = _check(orc, fx, _kind("T", N_MIN), piece_kib=1, warm_kib=0)
    assert st["rounds"] > 2


def test_fx_rounds_on_4mib(orc, fx):
    """The round counts the defaults are chosen from (64 KiB pieces, 64 KiB warm-up): text converges in a few rounds, not in
    one per piece."""
    src = _kind("T", 4 << 20)
    st = _check(orc, fx, src)
    assert st["pieces"] == 64 and 2 <= st["rounds"] <= 12, st
    st = _check(orc, fx, _kind("R", 4 << 20))
    assert st["rounds"] == 1, st


def test_fx_fuzz_corpus_1mib(orc, fx, monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "tests", "fuzz"))
    import fuzz_encode
    monkeypatch.setenv("FUZZ_MAXN", str(1 << 20))
    rng = np.random.default_rng(2024)
    for it in range(8):
        src = np.ascontiguousarray(fuzz_encode.make(rng, it))
        if src.size < N_MIN:
            continue
        _check(orc, fx, src, [orc.bound(src.size), src.size], piece_kib=(4, 16, 64)[it % 3], warm_kib=(0, 8, 64)[it % 3])
