"""The few-block level-2 path on blocks with history outside the block (plz4_amd/csrc/lz4_mx_device.inl, MxlFlavour: a block's
LZ4MID walk behind its external segment cut into pieces, rounds until every piece starts from the exact state its predecessor ends
in, the gather, the unchanged emit stage) on the lane-emulated build of the same source.  Its blocks must be those of the real
liblz4 driven as clz4.go drives it -- LZ4_loadDictHC(segment) + LZ4_compress_HC_continue for a linked block, an attached
LZ4_loadDictHC context for a block above 4 KiB under a dictionary -- byte for byte, whatever the segment's length, the piece size,
the warm-up and the order of the pieces.  Also the restart argument behind a segment, and the path's route function."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import corpus
from emulib import ENC_SLACK, _check_guard, _guarded
from orclib import ROOT, _ptr, u8p
from plz4_amd import synth

SRC = os.path.join(ROOT, "tests", "emu", "emu_mxl.cpp")
SO = os.path.join(ROOT, "tests", "emu", "_build", "libemu_mxl.so")
DEPS = [SRC, os.path.join(ROOT, "tests", "emu", "piece_rounds.h")] + [os.path.join(ROOT, "plz4_amd", "csrc", f) for f in (
    "lz4_mx_device.inl", "lz4_fx_device.inl", "lz4_pieces_device.inl", "lz4hc_lazy_device.inl", "lz4_seq_device.inl", "lz4_device.inl", "wave.h", "ws_layout.h", "route.h")]
BSZ = 4 << 20
NUL = np.zeros(1, dtype=np.uint8)


class MxlEmu:
    def __init__(self):
        newest = max(os.path.getmtime(p) for p in DEPS)
        if not os.path.exists(SO) or os.path.getmtime(SO) < newest:
            os.makedirs(os.path.dirname(SO), exist_ok=True)
            tmp = "%s.%d.tmp" % (SO, os.getpid())                    # (several test processes may build at once: the last rename wins)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-parameter", "-o", tmp, SRC])
            os.replace(tmp, SO)
        L = self.L = C.CDLL(SO)
        L.emu_mxl_encode.restype = C.c_int
        L.emu_mxl_encode.argtypes = [u8p, C.c_int, u8p, C.c_int, u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong), C.c_void_p]
        L.emu_mxl_whole.restype = C.c_int
        L.emu_mxl_whole.argtypes = [u8p, C.c_int, u8p, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
        L.emu_mxl_restart.restype = C.c_int
        L.emu_mxl_restart.argtypes = [u8p, C.c_int, u8p, C.c_int, C.c_int]
        L.emu_mxl_route.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
        L.emu_mxl_set_descending.argtypes = [C.c_int]

    def encode(self, seg, src, cap, piece=128 << 10, warm=256 << 10, order=0, records=False):
        dst = _guarded(cap, ENC_SLACK)
        st = (C.c_longlong * 6)()
        seq = np.zeros(src.size // 4 + 64, dtype=np.uint64) if records else None
        r = int(self.L.emu_mxl_encode(_ptr(seg if seg.size else NUL), seg.size, _ptr(src if src.size else NUL), src.size, _ptr(dst), cap,
                                      piece, warm, order, st, seq.ctypes.data if records else None))
        _check_guard(dst, cap, "emu_mxl_encode")
        stats = {"rounds": st[0], "again": st[1], "pieces": st[2], "nseq": st[3], "chain": st[4], "walked": st[5]}
        return r, dst[:max(r, 0)], stats, (seq[:st[3]] if records and r >= 0 else None)

    def whole(self, seg, src):
        out = np.zeros(src.size // 4 + 64, dtype=np.uint64)
        la = C.c_int(0)
        r = int(self.L.emu_mxl_whole(_ptr(seg if seg.size else NUL), seg.size, _ptr(src), src.size, out.ctypes.data, C.byref(la)))
        return out[:r], la.value

    def restart(self, seg, src, stops):
        return int(self.L.emu_mxl_restart(_ptr(seg if seg.size else NUL), seg.size, _ptr(src), src.size, stops))

    def route(self, env, level, nb, max_len, hc_ex=True, rider=False):
        out = (C.c_int * 9)()
        text = "".join("PLZ4HIP_%s=%s\n" % kv for kv in env.items()).encode()
        self.L.emu_mxl_route(text, level, nb, max_len, int(hc_ex), int(rider), out)
        return {"mxl": out[0], "piece": out[1], "warm": out[2], "P": out[3], "taken": out[4], "no_staged": out[5], "no_pieces": out[6],
                "mx": out[7], "default": out[8]}


@pytest.fixture(scope="module")
def mxl():
    return MxlEmu()


def _bound(n):
    return n + n // 255 + 16


def _ref_linked(ref, seg, src, cap):
    """A linked block behind the tail `seg`: clz4.StreamLinkedCtxHC -- LZ4_loadDictHC(tail), LZ4_compress_HC_continue."""
    return ref.stream_linked_ctx_hc(2)(src, cap, seg)


def _check(ref, mxl, seg, src, caps=None, refc=_ref_linked, **kw):
    """The emulated path's bytes and verdicts at every capacity against the reference's; the capacity one below the compressed
    size is added where there is one."""
    n = src.size
    want, _ = refc(ref, seg, src, _bound(n))
    caps = list(caps or (_bound(n),)) + ([want - 1] if want > 1 else [])
    st = None
    for cap in caps:
        want, wcomp = refc(ref, seg, src, cap)
        r, out, st, _ = mxl.encode(seg, src, cap, **kw)
        assert r == want, (seg.size, n, cap, kw, r, want)
        assert np.array_equal(out, wcomp[:want]), (seg.size, n, cap, kw)
    return st


def _pair(kind, seg_len, n, seed=synth.SEED):
    """A segment of seg_len bytes and a block of n bytes out of one stream of `kind`: they share their vocabulary."""
    data = np.ascontiguousarray(synth.make(kind, 65536 + n, 1 << 16, seed=seed))
    # (copies: a tail that lies right in front of the block in memory would be a prefix to liblz4, not an external segment)
    return data[65536 - seg_len:65536].copy(), data[65536:65536 + n].copy()


PIECE = 4096
SEGS = [0, 3, 7, 8, 9, 100, 4096, 65535, 65536]
LENGTHS = [0, 12, 13, 4097, PIECE - 1, PIECE, PIECE + 1, 8 * PIECE, 5 * PIECE + 7, 100003]


@pytest.mark.parametrize("seg_len", SEGS)
def test_mxl_segments_and_lengths_bytes_identical(ref, mxl, seg_len):
    """Every segment length around LZ4MID_fillHTable's thresholds, block lengths below / at kMinLength, around one piece, a multiple
    of the piece, a last piece shorter than 12 bytes, an odd length: the reference's bytes at capacity bound, n and one below the
    compressed size (verdict 0), at 4 KiB pieces with 8 KiB of warm-up."""
    for n in LENGTHS:
        seg, src = _pair("T", seg_len, n)
        st = _check(ref, mxl, seg, src, [_bound(n)] + ([n] if n else []), piece=PIECE, warm=2 * PIECE)
        assert st["pieces"] == max(1, -(-n // PIECE)), (n, st)
    seg, src = _pair("M", seg_len, 100003, seed=7)
    _check(ref, mxl, seg, src, [_bound(100003), 100003], piece=16 << 10, warm=16 << 10)


def test_mxl_user_dictionary_of_70000_bytes(ref, mxl):
    """Independent blocks above 4 KiB under a dictionary context (clz4.StreamCtxHC): the dictionary's last 64 KiB are the segment."""
    user = synth.text(70000, seed=42)
    d64 = np.ascontiguousarray(user[-65536:])
    keep, daddr = ref.new_dict_ctx_hc(d64, 2)
    comp = ref.stream_ctx_hc(2, daddr)
    refc = lambda ref_, seg, src, cap: comp(src, cap)
    for n in (4097, 5 * PIECE + 7, 100003):
        src = np.ascontiguousarray(synth.text(n, seed=43))
        _check(ref, mxl, d64, src, [_bound(n), n], refc=refc, piece=PIECE, warm=2 * PIECE)
        _check(ref, mxl, d64, src, refc=refc, piece=16 << 10, warm=16 << 10)


@pytest.mark.parametrize("kind", ["T", "R", "Z", "M"])
def test_mxl_1mib(ref, mxl, kind):
    seg, src = _pair(kind, 65536, 1 << 20)
    _check(ref, mxl, seg, src, [(1 << 20) + 5000, 1 << 20], piece=32 << 10, warm=64 << 10)


def twin_of_segment():
    """A 64 KiB text segment and a block that begins with a copy of the segment's last 60 KiB, then text of the same vocabulary:
    4 KiB pieces 1..16 find their matches inside the segment -- matches that end at the segment's end (safeLen), no look at ip + 1,
    no catch-up -- and a guessed start's zeroed tables lack the segment's live entries."""
    seg = np.ascontiguousarray(synth.text(65536, seed=11))
    rest = synth.text(140000, seed=11)[65536:]
    return seg, np.ascontiguousarray(np.concatenate([seg[-(60 << 10):], rest]))


def perturbed_twin():
    """twin_of_segment with one byte in 211 of the copy changed: not one long match but some three hundred, every one of them into
    the segment, in every 4 KiB piece of the first 60 KiB."""
    seg, src = twin_of_segment()
    src = src.copy()
    src[97:60 << 10:211] ^= 0x15
    return seg, src


def no_match_into_segment():
    """The twin: a block of text whose first 64 KiB (and everything else) has no match into its 64 KiB segment of random bytes."""
    return np.ascontiguousarray(synth.random_bytes(65536, seed=12)), np.ascontiguousarray(synth.text(60 * 1024 + 74464, seed=11))


def test_mxl_matches_inside_the_segment(ref, mxl):
    seg, src = twin_of_segment()
    for warm in (0, 2 * PIECE):
        for order in (0, 1):
            st = _check(ref, mxl, seg, src, [_bound(src.size), src.size], piece=PIECE, warm=warm, order=order)
        if warm == 0:
            assert st["again"] > 0 and st["rounds"] > 1, st           # (the repair rounds were exercised)
    _check(ref, mxl, seg, src, piece=16 << 10, warm=16 << 10)
    seg, src = perturbed_twin()
    for warm in (0, 2 * PIECE):
        st = _check(ref, mxl, seg, src, [_bound(src.size), src.size], piece=PIECE, warm=warm)
        if warm == 0:
            assert st["again"] > 0 and st["rounds"] > 1, st
    seg, src = no_match_into_segment()
    for warm in (0, 2 * PIECE):
        _check(ref, mxl, seg, src, [_bound(src.size), src.size], piece=PIECE, warm=warm)
    _check(ref, mxl, seg, src, piece=16 << 10, warm=16 << 10)


def test_mxl_twins(ref, mxl):
    seg = np.ascontiguousarray(synth.text(65536, seed=3))
    for name, src in corpus.twin_cases():
        _check(ref, mxl, seg, np.ascontiguousarray(src), piece=16 << 10, warm=16 << 10)


def test_mxl_restart_from_saved_states_is_exact(mxl):
    """From every saved boundary state a fresh walk gives the records of the unbroken hc_mid_parse<true>, behind a 64 KiB and a
    100-byte segment; the block that matches into its segment included."""
    cases = [("T", 65536, 256 << 10, 4096), ("T", 100, 256 << 10, 4096), ("T", 65536, 1 << 20, 65536 + 333), ("M", 65536, 256 << 10, 4096),
             ("M", 100, 256 << 10, 4096)]
    for kind, seg_len, n, stops in cases:
        seg, src = _pair(kind, seg_len, n)
        tried = mxl.restart(seg, src, stops)
        assert tried > 0, (kind, seg_len, stops, tried)
        if kind == "T":
            assert tried >= (n // stops) * 3 // 4, (kind, seg_len, stops, tried)
    seg, src = twin_of_segment()                       # (its first 60 KiB are a handful of matches: few boundaries have a state of their own)
    assert mxl.restart(seg, src, 4096) > 0
    assert mxl.restart(seg[-100:].copy(), src, 4096) > 0
    seg, src = perturbed_twin()
    assert mxl.restart(seg, src, 4096) >= (src.size // 4096) * 3 // 4


def test_mxl_records_are_the_unbroken_walks_any_order(mxl):
    """Piece order ascending and descending, lane order both ways: the records of the rounds are the unbroken walk's, with the same
    statistics either way."""
    for seg, src in (_pair("T", 65536, 512 << 10), twin_of_segment()):
        whole, _ = mxl.whole(seg, src)
        stats = []
        try:
            for lanes in (0, 1):
                mxl.L.emu_mxl_set_descending(lanes)
                for order in (0, 1):
                    r, _, st, seq = mxl.encode(seg, src, _bound(src.size), 8 << 10, 0, order=order, records=True)
                    assert r > 0 and st["rounds"] > 1
                    assert np.array_equal(seq, whole), (lanes, order)
                    stats.append(st)
        finally:
            mxl.L.emu_mxl_set_descending(0)
        assert all(s == stats[0] for s in stats), stats


def test_mxl_route_edges(mxl):
    limit = {"MXL_MAX_BLOCKS": "64"}
    on = mxl.route(limit, 2, 64, BSZ)
    assert {k: on[k] for k in ("mxl", "piece", "warm", "P", "taken", "no_staged", "no_pieces", "mx")} == {
        "mxl": 1, "piece": 128 << 10, "warm": 256 << 10, "P": 32, "taken": 1, "no_staged": 0, "no_pieces": 0, "mx": 0}
    assert mxl.route(limit, 2, 65, BSZ)["mxl"] == 0                            # limit + 1 blocks
    assert mxl.route(limit, 2, 0, BSZ)["mxl"] == 0
    assert mxl.route(limit, 2, 1, BSZ + 1)["mxl"] == 0                         # 4 MiB + 1
    assert mxl.route(limit, 2, 1, 128 << 10)["mxl"] == 0 and mxl.route(limit, 2, 1, (128 << 10) + 1)["P"] == 2   # one piece / one piece + 1
    assert mxl.route(limit, 2, 4, BSZ, rider=True)["mxl"] == 0
    assert mxl.route(limit, 2, 4, BSZ, hc_ex=False)["mxl"] == 0                # (an independent call is mx_want's ...)
    assert mxl.route(limit, 2, 4, BSZ, hc_ex=False)["mx"] == 1
    assert mxl.route(limit, 2, 4, BSZ)["mx"] == 0                              # (... and mx_want still answers 0 for hcEx)
    assert mxl.route(limit, 1, 4, BSZ)["mxl"] == 0 and mxl.route(limit, 3, 4, BSZ)["mxl"] == 0
    assert mxl.route({"MXL_MAX_BLOCKS": "0"}, 2, 1, BSZ)["mxl"] == 0           # the switch at 0
    assert mxl.route({"MX_MAX_BLOCKS": "0", "MXL_MAX_BLOCKS": "4"}, 2, 4, BSZ)["mxl"] == 1     # (the two limits are independent)
    # unset: the measured default (profiles/mxl_rate.json), the same bar as kMxMaxBlocks
    d = mxl.route({}, 2, 1, BSZ)["default"]
    assert mxl.route({}, 2, max(d, 1), BSZ)["mxl"] == (1 if d >= 1 else 0) and mxl.route({}, 2, d + 1, BSZ)["mxl"] == 0
    two = mxl.route({"MXL_MAX_BLOCKS": "2", "MX_PIECE_KIB": "8", "MX_WARMUP_KIB": "16"}, 2, 2, 200 * 1024 + 13)
    assert two["mxl"] == 1 and two["piece"] == 8192 and two["warm"] == 16384 and two["P"] == 26
    assert mxl.route({"MXL_MAX_BLOCKS": "2"}, 2, 3, BSZ)["mxl"] == 0
    big = {"MXL_MAX_BLOCKS": "100000"}                                         # (clamped to what one launch's grid holds)
    assert mxl.route(big, 2, 65535, BSZ)["mxl"] == 1 and mxl.route(big, 2, 65536, BSZ)["mxl"] == 0
    odd = mxl.route(dict(limit, MX_PIECE_KIB="0", MX_WARMUP_KIB="5000"), 2, 1, BSZ)    # out of range: the defaults stay
    assert odd["piece"] == 128 << 10 and odd["warm"] == 256 << 10
    assert mxl.route(dict(limit, MX_WARMUP_KIB="0"), 2, 1, BSZ)["warm"] == 0
