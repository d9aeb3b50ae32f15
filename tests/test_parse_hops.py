"""The grid batch's scalar hop (plz4_amd/csrc/lz4_seq_device.inl, PLZ4_HOP) on the lane-emulated build of the same source: a match
without a successor is its own successor, so a hop has no test in it; a batch's first walk makes eight hops unconditionally and asks ONE question
for its two rare ways on (more matches than that; a lane that fills its 20-byte window was executed).  Blocks must be
LZ4_compress_fast's of the compiled reference, byte for byte, in both lane orders, with poison and with zeros, in all three builds
of the parser; the parser's counters and records show that each crafted input (tests/hopcases.py) did what it is for; and on the
bench's text the share of batches behind the question for more hops is what chose the eight."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hopcases
from emulib import ENC_SLACK, _check_guard, _guarded
from orclib import ROOT, _ptr, u8p
from plz4_amd import synth

SRC = os.path.join(ROOT, "tests", "emu", "emu_parse_hops.cpp")
BUILD = os.path.join(ROOT, "tests", "emu", "_build")
DEPS = [SRC] + [os.path.join(ROOT, "plz4_amd", "csrc", f) for f in ("lz4_seq_device.inl", "lz4_device.inl", "wave.h")]
CNT = {"batches": 0, "primes": 1, "second_round": 6, "took36": 19, "unfinished": 20, "unfinished_x36": 21, "guarded": 22, "from_lane0": 23}
MODES = [(0, 1), (0, 0), (1, 1), (1, 0)]            # (descending lane order, poison)
N_HOPS = 8


class PhEmu:
    """variant: None = the product's parser; 0 = -DPLZ4_HOP=0, the walk as it was."""

    def __init__(self, variant=None):
        so = os.path.join(BUILD, "libemu_ph%s.so" % ("" if variant is None else "_v%d" % variant))
        newest = max(os.path.getmtime(p) for p in DEPS)
        if not os.path.exists(so) or os.path.getmtime(so) < newest:
            os.makedirs(BUILD, exist_ok=True)
            flags = [] if variant is None else ["-DPLZ4_HOP=%d" % variant]
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-parameter"] + flags + ["-o", so, SRC])
        L = self.L = C.CDLL(so)
        L.emu_ph_encode.restype = C.c_int
        L.emu_ph_encode.argtypes = [u8p, C.c_int, u8p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
        L.emu_ph_set_descending.argtypes = [C.c_int]
        L.emu_ph_set_poison.argtypes = [C.c_int]
        assert L.emu_ph_variant() == (1 if variant is None else variant)
        assert L.emu_ph_hops() == (N_HOPS if variant is None else 6)

    def mode(self, descending, poison):
        self.L.emu_ph_set_descending(int(descending))
        self.L.emu_ph_set_poison(int(poison))

    def counters(self):
        """(the named counters, batches by the number of matches their first walk executed); reset on read"""
        cnt, hops = (C.c_ulonglong * 32)(), (C.c_ulonglong * 18)()
        self.L.emu_ph_counters(cnt, hops)
        return {k: int(cnt[i]) for k, i in CNT.items()}, [int(v) for v in hops]

    def encode(self, src, cap, win):
        dst = _guarded(cap, ENC_SLACK)
        seq = np.zeros(src.size // 4 + 3, dtype=np.uint64)
        ns = C.c_int(0)
        r = int(self.L.emu_ph_encode(_ptr(src), src.size, _ptr(dst), cap, win, seq.ctypes.data, C.byref(ns)))
        _check_guard(dst, cap, "emu_ph_encode")
        return r, dst[:max(r, 0)], seq[:ns.value]


@pytest.fixture(scope="module")
def ph():
    e = PhEmu()
    yield e
    e.mode(0, 1)


@pytest.fixture(scope="module")
def ph_old():
    e = PhEmu(0)
    yield e
    e.mode(0, 1)


def _records(seq):
    pos = (seq & np.uint64(0x3FFFFF)).astype(np.int64)
    fwd = ((seq >> np.uint64(22)) & np.uint64(0x3FFFFF)).astype(np.int64)
    return dict(zip(pos.tolist(), fwd.tolist()))


def _check(ref, emu, src):
    """Bytes against the reference in every mode and build; returns {(descending, poison, win): (counters, batches by matches,
    records)}."""
    n = src.size
    cap = n + n // 255 + 16
    want, wcomp = ref.compress_fast(src, cap)
    out = {}
    for desc, poison in MODES:
        emu.mode(desc, poison)
        for win in (0, 1, 2):
            emu.counters()
            r, got, seq = emu.encode(src, cap, win)
            cnt, hops = emu.counters()
            out[(desc, poison, win)] = (cnt, hops, _records(seq))
            assert r == want, (n, desc, poison, win, r, want)
            assert np.array_equal(got, wcomp[:want]), (n, desc, poison, win)
    emu.mode(0, 1)
    return out


def _site_matches(rec, x):
    return sorted(p for p in rec if x <= p < x + 64)


@pytest.fixture(scope="module")
def crafted():
    return {name: hopcases.block(name) for name in hopcases.NAMES}


@pytest.mark.parametrize("name", hopcases.NAMES)
def test_hops_crafted(ref, ph, ph_old, crafted, name):
    """Every crafted block: the reference's bytes in every mode and build, old walk and new; the records hold each site's matches
    with their lengths and nothing else in the site's batch; the ground has at most three matches in a batch, so the counters
    belong to the sites."""
    src, exp, xs = crafted[name]
    old = _check(ref, ph_old, src)
    new = _check(ref, ph, src)
    for key, (cnt, hops, rec) in new.items():
        desc = key[0]
        assert rec == old[key][2], key
        for site, x in zip(exp, xs):
            for p, ln in site:
                assert rec.get(p) == ln - 4, (name, key, p, ln, rec.get(p))
            if name != "wrap":
                assert _site_matches(rec, x) == [p for p, _ in site], (name, key, x)
        if desc:
            continue            # (descending lane order gives batches up for the generic parser: the counters below are the ascending order's)
        k = 1 if name == "wrap" else len(hopcases.CASES[name][1])
        if name == "wrap":
            # no executed match, lane 0 a hit with a successor below the first probe lane: only the first hop's guard keeps the walk out
            assert cnt["guarded"] >= hopcases.SITES, (key, cnt)
            for x in xs:
                assert _site_matches(rec, x) == [], (key, x)
        elif "x36" in name:
            # (the first walk takes the long match at its window's length and hops on inside it: it counts a match or two more)
            assert sum(hops[k:]) >= hopcases.SITES and sum(hops[4:k]) == 0, (name, key, hops)
            assert cnt["unfinished"] == sum(hops[N_HOPS + 1:]), (name, key, cnt, hops)
        else:
            assert hops[k] >= hopcases.SITES and sum(hops[4:]) == hops[k], (name, key, hops)
            assert cnt["unfinished"] == (hops[k] if k > N_HOPS else 0), (name, key, cnt, hops)
        if name == "first_at_lane0":
            assert cnt["from_lane0"] >= hopcases.SITES, (key, cnt)
        if name == "thirteen":
            assert hops[13] >= hopcases.SITES, (key, hops)
        if name in ("nine_then_x36", "x36_then_nine"):
            # both halves of the merged question true at once
            assert cnt["unfinished_x36"] >= hopcases.SITES and cnt["took36"] >= hopcases.SITES, (name, key, cnt)
        else:
            assert cnt["unfinished_x36"] == 0, (name, key, cnt)
        # the old walk counts its own question: more than six hops
        ocnt, ohops, _ = old[key]
        assert ohops == hops and ocnt["unfinished"] == sum(hops[7:]), (name, key, ocnt, hops)


def test_hops_text_4mib_share(ref, ph, ph_old):
    """The count that chose eight unconditional hops, on the bench's 4 MiB T block: at most 2 % of the grid batches are not
    finished after them (a third are after the old walk's six), and the old walk's records are the new one's."""
    src = np.ascontiguousarray(synth.make("T", 4 << 20, 1 << 16)[:4 << 20])
    want, wcomp = ref.compress_fast(src, 4 << 20)
    res = {}
    for name, emu in (("new", ph), ("old", ph_old)):
        emu.mode(0, 1)
        for win in (0, 1, 2):
            emu.counters()
            r, got, seq = emu.encode(src, 4 << 20, win)
            cnt, hops = emu.counters()
            assert r == want and np.array_equal(got, wcomp[:want]), (name, win)
            res[(name, win)] = (cnt, hops, seq)
    for win in (0, 1, 2):
        cnt, hops, seq = res[("new", win)]
        ocnt, ohops, oseq = res[("old", win)]
        print(win, "new", cnt, hops)
        print(win, "old", ocnt)
        assert np.array_equal(seq, oseq) and hops == ohops
        assert cnt["batches"] == ocnt["batches"] == 65534
        assert cnt["unfinished"] == sum(hops[N_HOPS + 1:]) and ocnt["unfinished"] == sum(hops[7:])
        assert cnt["unfinished"] / cnt["batches"] <= 0.02, cnt
        assert sum(hops[N_HOPS:]) / cnt["batches"] > 0.02            # (seven hops would not do)
        assert 0.30 < ocnt["unfinished"] / ocnt["batches"] < 0.40, ocnt
