"""The level-1 parser's candidate windows (plz4_amd/csrc/lz4_seq_device.inl) on the lane-emulated build of the same source:
candidate windows are loaded only by the lanes that have a candidate (the others get poison, or zeros as on the hardware), and a
hit that fills its 20-byte window takes 16 bytes more when the batch's first walk executes it, before anything is committed.  Blocks must be LZ4_compress_fast's of the compiled
reference, byte for byte, in both lane orders, with poison and with zeros, in all three builds of the parser; the parser's counters
show that the crafted inputs did what they are for and what the two changes are worth in events."""
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

SRC = os.path.join(ROOT, "tests", "emu", "emu_parse_win.cpp")
BUILD = os.path.join(ROOT, "tests", "emu", "_build")
DEPS = [SRC] + [os.path.join(ROOT, "plz4_amd", "csrc", f) for f in ("lz4_seq_device.inl", "lz4_device.inl", "wave.h")]
N_MIN = 65547          # liblz4's byU32 tables from here on (lz4.c:1389)
CNT = {"batches": 0, "primes": 1, "misorder": 2, "long_only": 3, "measured": 4, "returned_other": 5, "second_round": 6, "no_regs": 7,
       "cand_loads": 8, "cand_lanes": 9, "ext_loads": 10, "first_full20": 11}


class PwEmu:
    """variant: None = the product's parser; 0 = -DPLZ4_PW=0, the parser as it was (every lane loads, 20-byte window)."""

    def __init__(self, variant=None):
        so = os.path.join(BUILD, "libemu_pw%s.so" % ("" if variant is None else "_v%d" % variant))
        newest = max(os.path.getmtime(p) for p in DEPS)
        if not os.path.exists(so) or os.path.getmtime(so) < newest:
            os.makedirs(BUILD, exist_ok=True)
            flags = [] if variant is None else ["-DPLZ4_PW=%d" % variant]
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-parameter"] + flags + ["-o", so, SRC])
        L = self.L = C.CDLL(so)
        L.emu_pw_encode.restype = C.c_int
        L.emu_pw_encode.argtypes = [u8p, C.c_int, u8p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
        L.emu_pw_set_descending.argtypes = [C.c_int]
        L.emu_pw_set_poison.argtypes = [C.c_int]
        assert L.emu_pw_variant() == (3 if variant is None else variant)

    def mode(self, descending, poison):
        self.L.emu_pw_set_descending(int(descending))
        self.L.emu_pw_set_poison(int(poison))

    def counters(self):
        out = (C.c_ulonglong * 16)()
        self.L.emu_pw_counters(out)
        return {k: int(out[i]) for k, i in CNT.items()}

    def encode(self, src, cap, win, records=False):
        dst = _guarded(cap, ENC_SLACK)
        seq = np.zeros(src.size // 4 + 3, dtype=np.uint64) if records else None
        ns = C.c_int(0)
        r = int(self.L.emu_pw_encode(_ptr(src) if src.size else C.cast(None, u8p), src.size, _ptr(dst), cap, win,
                                     seq.ctypes.data if records else None, C.byref(ns)))
        _check_guard(dst, cap, "emu_pw_encode")
        return r, dst[:max(r, 0)], (seq[:ns.value] if records else None)


@pytest.fixture(scope="module")
def pw():
    e = PwEmu()
    yield e
    e.mode(0, 1)


@pytest.fixture(scope="module")
def pw_old():
    return PwEmu(0)


MODES = [(0, 1), (0, 0), (1, 1), (1, 0)]            # (descending lane order, poison)


def _check(ref, pw, src, caps=None, modes=MODES, wins=(0, 1, 2)):
    src = np.ascontiguousarray(src)
    n = src.size
    bound = n + n // 255 + 16
    for cap in caps or (bound,):
        want, wcomp = ref.compress_fast(src, cap)
        for desc, poison in modes:
            pw.mode(desc, poison)
            for win in wins:
                r, out, _ = pw.encode(src, cap, win)
                assert r == want, (n, cap, desc, poison, win, r, want)
                assert np.array_equal(out, wcomp[:want]), (n, cap, desc, poison, win)
    pw.mode(0, 1)


def _kind(kind, n):
    return np.ascontiguousarray(synth.make(kind, n, min(n, 1 << 16))[:n])


def test_pw_corpus(ref, pw):
    for name, src in corpus.small_cases():
        n = src.size
        _check(ref, pw, src, [n + n // 255 + 16, n, max(n - 1, 0)], modes=[(0, 1), (1, 0)], wins=(0,))
    for name, src in corpus.block_cases_64k() + corpus.twin_cases():
        _check(ref, pw, src)
    for n, seed in ((N_MIN, 1), (100000, 3), (262144 + 17, 4), (1 << 20, 5)):
        _check(ref, pw, corpus.structured(n, seed))


@pytest.mark.parametrize("n", [N_MIN, 1 << 20, 4 << 20])
@pytest.mark.parametrize("kind", ["T", "R", "Z", "M"])
def test_pw_kinds(ref, pw, kind, n):
    src = _kind(kind, n)
    _check(ref, pw, src, [n + n // 255 + 16, n])


def _records(seq):
    pos = (seq & np.uint64(0x3FFFFF)).astype(np.int64)
    fwd = ((seq >> np.uint64(22)) & np.uint64(0x3FFFFF)).astype(np.int64)
    return dict(zip(pos.tolist(), fwd.tolist()))


@pytest.mark.parametrize("length", pwcases.LENGTHS)
def test_pw_crafted_lengths(ref, pw, pw_old, length):
    """A phrase that recurs with a total match length of `length`, starting at lanes 0, 27, 43, 63 and at the lane from which it
    ends exactly at a batch boundary: the records hold each of those matches with that length, the bytes are the reference's, and
    for lengths that fill the 20-byte window the first walk of a grid batch executed such a lane -- in the parser as it was, too."""
    src, sites = pwcases.block_for_length(length)
    _check(ref, pw, src)
    for emu in (pw, pw_old):
        emu.mode(0, 1)
        for win in (0, 1, 2):
            emu.counters()
            r, _, seq = emu.encode(src, src.size + src.size // 255 + 16, win, records=True)
            c = emu.counters()
            rec = _records(seq)
            for x in sites:
                assert rec.get(x) == length - 4, (length, x, x & 63, rec.get(x))
            assert (sites[-1] + length) % 64 == 0
            if length - 4 >= 16:
                assert c["first_full20"] >= len(sites), (length, win, c)
            if emu is pw:
                assert c["cand_loads"] == c["cand_lanes"] < 64 * (c["batches"] + c["primes"]), c
                # what the 36-byte window is for: only a match of 36 bytes or more is still measured in a second round
                if 20 <= length < 36:
                    assert c["ext_loads"] >= 2 * len(sites), (length, win, c)
    _check(ref, pw_old, src, modes=[(0, 1), (1, 1)])


@pytest.mark.parametrize("length", pwcases.LENGTHS)
def test_pw_crafted_match_limit(ref, pw, length):
    """The block's last match runs into matchLimit `length` bytes after it starts: the generic batches of a block's end."""
    src, x = pwcases.block_to_match_limit(length)
    _check(ref, pw, src)
    pw.mode(0, 1)
    _, _, seq = pw.encode(src, src.size + src.size // 255 + 16, 2, records=True)
    assert _records(seq).get(x) == length - 4, (length, x)


def test_pw_text_4mib_counts(ref, pw, pw_old):
    """The point of both changes on the bench's text, as exact event counts over the three builds of the parser: a candidate load
    is issued by the lanes that have a candidate (28.6 of 64 per batch), and a second round for no other reason than a match
    longer than the window is taken by 8.0 % of the batches with the 20-byte window and by fewer than 2.0 % with the 36-byte one."""
    src = _kind("T", 4 << 20)
    tot = {}
    for name, emu in (("new", pw), ("old", pw_old)):
        emu.mode(0, 1)
        emu.counters()
        for win in (0, 1, 2):
            r, _, _ = emu.encode(src, 4 << 20, win)
            assert r > 0
        tot[name] = emu.counters()
    new, old = tot["new"], tot["old"]
    print("new", new)
    print("old", old)
    assert old["batches"] == new["batches"] == 196602
    assert old["long_only"] == 15666 and abs(old["long_only"] / old["batches"] - 0.080) < 0.001
    assert new["long_only"] / new["batches"] < 0.020
    assert new["second_round"] < old["second_round"]
    assert old["cand_loads"] == 0                                   # (every lane loads there: not counted as candidate loads)
    lanes = new["cand_lanes"] / (new["batches"] + new["primes"])
    assert new["cand_loads"] == new["cand_lanes"] and 28.0 < lanes < 29.2, lanes
