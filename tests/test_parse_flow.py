"""The level-1 parser's control flow (plz4_amd/csrc/lz4_seq_device.inl) on the lane-emulated build of the same source.  A grid batch
has one way out: it always runs to its end and hands back why the consecutive batch must not follow it -- given up (the generic
batch takes over), a match reached the block's last probe position (done), the search is past 64 misses, the next batch is not the
consecutive one (a long match), the block's last 224 bytes, a piece's boundary (the parser of pieces, lz4_fx_device.inl).  Each
input here drives batches out through one of those ways; the blocks must be LZ4_compress_fast's of the compiled reference, byte for
byte, in all three builds of the parser, both lane orders, with poison and with zeros, and the parser's counters must show that the
way out was really taken (a test that never leaves the steady state proves nothing about the ways out)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import corpus
import pwcases
from emulib import ENC_SLACK, _check_guard, _guarded
from orclib import ROOT, _ptr, u8p
from plz4_amd import synth

SRC = os.path.join(ROOT, "tests", "emu", "emu_parse_flow.cpp")
SO = os.path.join(ROOT, "tests", "emu", "_build", "libemu_pf.so")
DEPS = [SRC, os.path.join(ROOT, "tests", "emu", "piece_rounds.h")] + [os.path.join(ROOT, "plz4_amd", "csrc", f) for f in (
    "lz4_fx_device.inl", "lz4_pieces_device.inl", "lz4_seq_device.inl", "lz4_device.inl", "wave.h", "ws_layout.h")]
N_MIN = 65547          # liblz4's byU32 tables from here on (lz4.c:1389)
CNT = {"batches": 0, "primes": 1, "misorder": 2, "measured": 4, "second_round": 6, "no_regs": 7, "ext_loads": 10,
       "gave_up": 12, "done": 13, "missed": 14, "far": 15, "tail": 16, "piece": 17, "warmup": 18, "took36": 19}
MODES = [(0, 1), (0, 0), (1, 1), (1, 0)]            # (descending lane order, poison)


class PfEmu:
    def __init__(self):
        newest = max(os.path.getmtime(p) for p in DEPS)
        if not os.path.exists(SO) or os.path.getmtime(SO) < newest:
            os.makedirs(os.path.dirname(SO), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-parameter", "-o", SO, SRC])
        L = self.L = C.CDLL(SO)
        L.emu_pf_encode.restype = C.c_int
        L.emu_pf_encode.argtypes = [u8p, C.c_int, u8p, C.c_int, C.c_int]
        L.emu_pf_fx_encode.restype = C.c_int
        L.emu_pf_fx_encode.argtypes = [u8p, C.c_int, u8p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
        L.emu_pf_set_descending.argtypes = [C.c_int]
        L.emu_pf_set_poison.argtypes = [C.c_int]
        self.slots = int(L.emu_pf_slots())
        assert self.slots > max(CNT.values())

    def mode(self, descending, poison):
        self.L.emu_pf_set_descending(int(descending))
        self.L.emu_pf_set_poison(int(poison))

    def counters(self):
        out = (C.c_ulonglong * self.slots)()
        self.L.emu_pf_counters(out)
        return {k: int(out[i]) for k, i in CNT.items()}

    def encode(self, src, cap, win):
        dst = _guarded(cap, ENC_SLACK)
        r = int(self.L.emu_pf_encode(_ptr(src), src.size, _ptr(dst), cap, win))
        _check_guard(dst, cap, "emu_pf_encode")
        return r, dst[:max(r, 0)]

    def fx_encode(self, src, cap, piece_kib, warm_kib):
        dst = _guarded(cap, ENC_SLACK)
        rounds = C.c_int(0)
        r = int(self.L.emu_pf_fx_encode(_ptr(src), src.size, _ptr(dst), cap, piece_kib << 10, warm_kib << 10, C.byref(rounds)))
        _check_guard(dst, cap, "emu_pf_fx_encode")
        return r, dst[:max(r, 0)], rounds.value


@pytest.fixture(scope="module")
def pf():
    e = PfEmu()
    yield e
    e.mode(0, 1)


def _check(ref, pf, src, modes=MODES, wins=(0, 1, 2)):
    """Bytes against the reference in every mode and build; returns the counters of each (descending, poison, win)."""
    src = np.ascontiguousarray(src)
    n = src.size
    out = {}
    for cap in (n + n // 255 + 16, n):
        want, wcomp = ref.compress_fast(src, cap)
        for desc, poison in modes:
            pf.mode(desc, poison)
            for win in wins:
                pf.counters()
                r, got = pf.encode(src, cap, win)
                out[(desc, poison, win)] = pf.counters()
                assert r == want, (n, cap, desc, poison, win, r, want)
                assert np.array_equal(got, wcomp[:want]), (n, cap, desc, poison, win)
    pf.mode(0, 1)
    return out


def _all(cnt, key, modes=None):
    """every run (of the given lane orders) took the way out `key` at least once"""
    for (desc, poison, win), c in cnt.items():
        if modes is None or desc in modes:
            assert c[key] > 0, (key, desc, poison, win, c)


def test_flow_long_match_stops_and_primes_again(ref, pf):
    """600 bytes of text once more, 10 000 bytes on: the match ends several batches ahead, the batch that finds it hands back `far`
    and the pipeline is primed again at the match's end."""
    src = synth.text(200000, seed=41).copy()
    src[100000:100600] = src[90000:90600]
    cnt = _check(ref, pf, src)
    _all(cnt, "far")
    for c in cnt.values():
        assert c["primes"] > 1 and c["measured"] > 0, c


def test_flow_search_past_64_misses(ref, pf):
    """Text with random stretches in it: inside a stretch no match is found, the search runs past 64 misses -- where the parser's
    stride grows and the grid batch is left -- and the grid batches are entered again in the text behind it."""
    src = synth.text(300000, seed=43).copy()
    for at in (70000, 150000, 230000):
        src[at:at + 20000] = synth.random_bytes(20000, seed=at)
    cnt = _check(ref, pf, src)
    _all(cnt, "missed")
    for c in cnt.values():
        assert c["primes"] > 3, c


@pytest.mark.parametrize("n", [N_MIN, N_MIN + 63, 100000, 131072 + 223, 131072 + 224, 131072 + 225])
def test_flow_block_end(ref, pf, n):
    """The grid batches stop in front of the block's last 224 bytes; the generic batches finish the block."""
    src = synth.text(n, seed=44 + n % 7)
    cnt = _check(ref, pf, src)
    for c in cnt.values():
        assert c["tail"] + c["far"] + c["done"] + c["gave_up"] > 0, c
    if n == 100000:
        _all(cnt, "tail")


@pytest.mark.parametrize("back", [236, 300, 400, 1000])
def test_flow_match_reaches_last_probe_inside_a_grid_batch(ref, pf, back):
    """The block's last `back` bytes repeat earlier text up to the block's end: the match is found by a grid batch (more than 224
    bytes in front of the end), measured in a second round, and ends the parse there (lz4.c:1233): `done`."""
    n = 65536 + 8192
    buf = synth.text(n, seed=45 + back).copy()
    rng = np.random.Generator(np.random.PCG64(back))
    x = n - back
    pwcases._plant(buf, rng, x, back)                       # (the copies are equal up to the block's last byte)
    cnt = _check(ref, pf, np.ascontiguousarray(buf))
    _all(cnt, "done", modes=(0,))
    for c in cnt.values():
        assert c["done"] + c["gave_up"] > 0, c               # (descending lanes may give the batch up first: the generic batch ends it)


def test_flow_give_up_in_descending_lane_order(ref, pf):
    """Lanes of one slot that commit in descending order get back a position above their own: the batch takes its commits back,
    passes through its record and state steps as a batch that executed nothing, and the generic batch takes over from the state it
    found.  Ascending order never gives up for that reason."""
    src = synth.text(1 << 20, seed=46)
    cnt = _check(ref, pf, src)
    _all(cnt, "gave_up", modes=(1,))
    for (desc, poison, win), c in cnt.items():
        if desc:
            assert c["misorder"] > 0, c
        else:
            assert c["misorder"] == 0, c
    for name, blk in corpus.twin_cases():
        if blk.size >= N_MIN:
            _check(ref, pf, blk, modes=[(1, 1), (0, 0)])


@pytest.mark.parametrize("length", [24, 25, 35, 36, 40])
def test_flow_take36_batch(ref, pf, length):
    """A hit that fills its 20-byte window, executed by the first walk: the batch takes the 36-byte window and walks once more."""
    src, sites = pwcases.block_for_length(length)
    cnt = _check(ref, pf, src)
    _all(cnt, "took36", modes=(0,))
    for (desc, poison, win), c in cnt.items():
        if not desc:
            assert c["ext_loads"] >= 2 * len(sites), c


@pytest.mark.parametrize("piece_kib,warm_kib", [(16, 16), (64, 64), (4, 0), (1, 0)])
def test_flow_piece_boundary_and_warm_up(ref, pf, piece_kib, warm_kib):
    """The parser of pieces: grid batches stop in front of a piece's boundary (`piece`), and a piece that starts early from a guessed
    state passes its warm-up boundary, where its records start (`warmup`)."""
    for kind, n in (("T", 1 << 20), ("M", 300000)):
        src = np.ascontiguousarray(synth.make(kind, n, min(n, 1 << 16))[:n])
        want, wcomp = ref.compress_fast(src, n + n // 255 + 16)
        for desc in (0, 1):
            pf.mode(desc, 1)
            pf.counters()
            r, got, rounds = pf.fx_encode(src, n + n // 255 + 16, piece_kib, warm_kib)
            c = pf.counters()
            assert r == want and np.array_equal(got, wcomp[:want]), (kind, n, piece_kib, warm_kib, desc, r, want)
            assert rounds >= 1
            if kind == "T":
                assert c["piece"] > 0, c
                if warm_kib:
                    assert c["warmup"] > 0, c
        pf.mode(0, 1)


def test_flow_every_way_out_on_mixed_input(ref, pf):
    """One block with all of it: text, random stretches, long repeats, a repeat up to the block's end."""
    n = 1 << 20
    buf = synth.text(n, seed=47).copy()
    for at in (200000, 500000):
        buf[at:at + 30000] = synth.random_bytes(30000, seed=at)
    buf[700000:705000] = buf[660000:665000]
    rng = np.random.Generator(np.random.PCG64(47))
    pwcases._plant(buf, rng, n - 500, 500)
    cnt = _check(ref, pf, np.ascontiguousarray(buf))
    for key in ("far", "missed", "took36"):
        _all(cnt, key)
    _all(cnt, "gave_up", modes=(1,))
    _all(cnt, "done", modes=(0,))
