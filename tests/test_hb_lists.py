"""Chain and lists built in pieces (plz4_amd/csrc/lz4hc_lists_device.inl: count, scan, fill, chain -- the kernels k_hb_count ..
k_hb_chain) on the lane-emulated build of the same source (tests/emu/emu_hb.cpp).  The staged builder, its pieces taken in ascending
and in descending order, must write exactly what hc12_build_lists fed by the histogram writes and what a loop written from the
definition (the last position per hash) gives: offsets, chain[0, nPad), rank of every inserted position, list[0, count) with its
flags -- in both lane orders.  Beside it: hb_want of route.h and HbLayout of ws_layout.h."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from orclib import ROOT
from plz4_amd import synth

SRC = os.path.join(ROOT, "tests", "emu", "emu_hb.cpp")
SO = os.path.join(ROOT, "tests", "emu", "_build", "libemu_hb.so")
CSRC = os.path.join(ROOT, "plz4_amd", "csrc")
u8p = C.POINTER(C.c_uint8)
PIECES = (256, 1024)
BIG = 200 * 1024 + 13
SEED_65535 = 7                                                             # (found with emu_hb_probe: see test_hb_far_predecessors)


class HbEmu:
    def __init__(self):
        deps = [SRC, os.path.join(ROOT, "tests", "emu", "hb_staged.h")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".inl", ".h"))]
        if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(p) for p in deps):
            os.makedirs(os.path.dirname(SO), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-parameter", "-o", SO, SRC])
        L = self.L = C.CDLL(SO)
        L.emu_hb_compare.argtypes = [u8p, C.c_int, C.c_int, C.c_int, C.c_int]
        L.emu_hb_probe.argtypes = [u8p, C.c_int, C.c_int, C.POINTER(C.c_int64)]
        L.emu_hb_want.argtypes = [C.c_char_p] + [C.c_int] * 6 + [C.POINTER(C.c_int64)]
        L.emu_hb_layout.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_int]
        L.emu_hb_set_descending.argtypes = [C.c_int]

    @staticmethod
    def _p(a):
        return (a if a.size else np.zeros(1, dtype=np.uint8)).ctypes.data_as(u8p)

    def compare(self, a, piece, skip=(0, 0), descending=False):
        a = np.ascontiguousarray(a, dtype=np.uint8)
        self.L.emu_hb_set_descending(int(descending))
        try:
            return int(self.L.emu_hb_compare(self._p(a), a.size, piece, skip[0], skip[1]))
        finally:
            self.L.emu_hb_set_descending(0)

    def probe(self, a, piece):
        out = (C.c_int64 * 3)()
        self.L.emu_hb_probe(self._p(a), a.size, piece, out)
        return [int(v) for v in out]

    def want(self, env, level, nb, max_len, span=None, segmented=True, overlap=False):
        out = (C.c_int64 * 5)()
        text = "".join("%s=%s\n" % kv for kv in env.items()).encode()
        self.L.emu_hb_want(text, level, nb, max_len, max_len if span is None else span, int(segmented), int(overlap), out)
        return dict(zip(("on", "piece", "P", "hbMax", "hbPieceKiB"), (int(v) for v in out)))

    def layout(self, per, P):
        out = (C.c_uint64 * 4)()
        takes = (C.c_uint64 * 32)()
        n = self.L.emu_hb_layout(per, P, out, takes, 8)
        return dict(zip(("offCnt", "offSlot", "total", "pieceStride"), (int(v) for v in out))), [tuple(int(takes[4 * i + j]) for j in range(4)) for i in range(n)]


@pytest.fixture(scope="module")
def hb():
    return HbEmu()


def _lengths(piece):
    return [0, 1, 3, 4, 5, 63, 64, 65, piece - 1, piece, piece + 1, piece + 3, piece + 4, 3 * piece + 17, BIG]


@pytest.fixture(scope="module")
def sources():
    """BIG bytes of each kind, cut to the lengths of a case -- computed once, never written to."""
    out = {"zeros": np.zeros(BIG, dtype=np.uint8), "text": np.ascontiguousarray(synth.text(BIG, seed=21)),
           "random": np.ascontiguousarray(synth.random_bytes(BIG, seed=22)), "mixed": np.ascontiguousarray(synth.make("M", BIG, 1 << 14, seed=23))}
    for a in out.values():
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("piece", PIECES)
def test_hb_staged_equals_one_wave_and_definition(hb, sources, piece, descending):
    """Zeros: every position has the same hash, and its one run crosses every piece."""
    for kind, data in sources.items():
        for n in _lengths(piece):
            if n == BIG and piece == 256 and kind in ("text", "random"):  # (800 pieces: the zeros and the mix; every kind at 1024)
                continue
            assert hb.compare(data[:n], piece, descending=descending) == 0, (kind, n, piece, descending)


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("piece", PIECES)
def test_hb_positions_never_inserted(hb, sources, piece, descending):
    """An external segment's last three positions [seg - 3, seg) in front of a block of every length; segments of piece - 1 and
    piece + 2 bytes put the range across a piece boundary."""
    for seg in (0, 2, 3, 4, piece - 1, piece + 2, 65536):
        skip = (max(seg - 3, 0), seg)
        for kind in ("text", "zeros"):
            for n in (_lengths(piece)[:-1] if seg <= piece + 2 else (5, 65, piece + 1, 3 * piece + 17)):
                assert hb.compare(sources[kind][:seg + n], piece, skip, descending) == 0, (kind, seg, n, piece, descending)
    assert hb.compare(sources["mixed"], piece, (piece - 2, piece + 1), descending) == 0   # (straddles the first boundary)
    assert hb.compare(sources["mixed"], piece, (2 * piece - 1, 2 * piece + 2), descending) == 0


@pytest.mark.parametrize("piece", PIECES)
def test_hb_far_predecessors(hb, piece):
    """One input that holds a predecessor exactly 65535 back (kept) and one exactly 65536 back (becomes "none") across piece
    boundaries, and positions whose predecessor lies two or more pieces back.  The seed was found by running the definition loop
    (emu_hb_probe) over seeds 0, 1, ...; that all three occur is asserted here."""
    data = np.random.default_rng(SEED_65535).integers(0, 256, BIG, dtype=np.uint8)
    at_65535, at_65536, far = hb.probe(data, piece)
    assert at_65535 >= 1 and at_65536 >= 1 and far >= 1, (at_65535, at_65536, far)
    for descending in (False, True):
        assert hb.compare(data, piece, descending=descending) == 0, (piece, descending)


SHAPE = dict(level=9, nb=1, max_len=4 << 20)


def test_hb_want_cases(hb):
    dflt = hb.want({}, **SHAPE)
    limit = dflt["hbMax"]
    assert dflt["on"] == 1 and limit >= 1 and dflt["piece"] == dflt["hbPieceKiB"] << 10 and dflt["P"] == -(-(4 << 20) // dflt["piece"])
    # the limit and limit + 1
    assert hb.want({}, 9, limit, 4 << 20)["on"] == 1 and hb.want({}, 9, limit + 1, 4 << 20)["on"] == 0
    assert hb.want({"PLZ4HIP_HB_MAX_BLOCKS": "2"}, 9, 2, 4 << 20)["on"] == 1 and hb.want({"PLZ4HIP_HB_MAX_BLOCKS": "2"}, 9, 3, 4 << 20)["on"] == 0
    assert hb.want({}, 9, 0, 4 << 20)["on"] == 0
    # off
    assert hb.want({"PLZ4HIP_HB_MAX_BLOCKS": "0"}, **SHAPE)["on"] == 0
    # the builder beside the walk, the other routes, the levels
    assert hb.want({}, overlap=True, **SHAPE)["on"] == 0
    assert hb.want({}, segmented=False, **SHAPE)["on"] == 0
    assert [hb.want({}, lv, 1, 4 << 20)["on"] for lv in (1, 2, 3, 11, 12, 13)] == [0, 0, 1, 1, 1, 0]
    # the largest segment + block at most one piece: nothing to cut; one byte more: two pieces
    p = dflt["piece"]
    assert hb.want({}, 9, 1, p)["on"] == 0
    w = hb.want({}, 9, 1, p + 1)
    assert w["on"] == 1 and w["P"] == 2
    w = hb.want({}, 9, 1, p - 65536 + 1, span=p + 1)                        # (the segment counts)
    assert w["on"] == 1 and w["P"] == 2
    # raw blocks above 4 MiB keep one wave per block
    assert hb.want({}, 12, 1, (4 << 20) + 1)["on"] == 0
    # the piece: KiB, clamped to 1 .. 4096
    w = hb.want({"PLZ4HIP_HB_PIECE_KIB": "8"}, 9, 3, 200 * 1024 + 13)
    assert w["on"] == 1 and w["piece"] == 8192 and w["P"] == 26
    assert hb.want({"PLZ4HIP_HB_PIECE_KIB": "0"}, **SHAPE)["hbPieceKiB"] == 1
    assert hb.want({"PLZ4HIP_HB_PIECE_KIB": "99999"}, **SHAPE)["hbPieceKiB"] == 4096
    assert hb.want({"PLZ4HIP_HB_MAX_BLOCKS": "-5"}, **SHAPE)["hbMax"] == 0
    assert hb.want({"PLZ4HIP_HB_MAX_BLOCKS": "999999"}, **SHAPE)["hbMax"] == 65535


def test_hb_layout_takes_do_not_overlap_and_sum_to_total(hb):
    for per, P in ((1, 1), (1, 65), (3, 26), (64, 65), (512, 4096)):
        L, takes = hb.layout(per, P)
        assert len(takes) == 2
        assert L["pieceStride"] == 32768
        spans = sorted((off, off + count * size) for off, count, size, _ in takes)
        assert spans[0][0] == 0
        for (_, end), (nxt, _) in zip(spans, spans[1:]):
            assert end <= nxt
        assert sum(end - off for off, end in spans) == L["total"] == spans[-1][1]           # (no padding: the arrays are multiples of 256)
        for off, count, size, align in takes:
            assert off % align == 0 and off % 256 == 0 and count == per * P * 32768 and size == 4
        assert {L["offCnt"], L["offSlot"]} == {s[0] for s in spans}
