"""The frame writer on the lane-emulated build of its source (plz4_amd/csrc/lz4_frame_write_device.inl, the kernels behind
plz4hip_dev_write_frames): the stream, both tables and info, exactly, against the model of the header's table of rules in
frame_write_cases.py, in both lane orders, with canaries around `out`, both tables and info; the oracle's frame byte for byte for one
frame; the emulated stream index over `out` must list what the writer's tables say; the host layer's Reader -- an implementation of
its own -- must read the plaintext back.  CPU only; what the kernels read is the business of tests/emu/frame_write_bounds_main.cpp
(test_frame_write_bounds.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import frame_write_cases as fwc
import stream_index_cases as sic
from orclib import ROOT

SRC = os.path.join(ROOT, "tests", "emu", "emu_frame_write.cpp")
BUILD = os.path.join(ROOT, "tests", "emu", "_build")
DEPS = [SRC] + [os.path.join(ROOT, "plz4_amd", "csrc", f) for f in ("lz4_frame_write_device.inl", "lz4_frame_verify_device.inl",
                                                                    "lz4_stream_index_device.inl", "lz4_body_index_device.inl", "lz4_device.inl",
                                                                    "wave.h")]
CANARY = fwc.CANARY
GUARD = 0x5A5A5A5A5A5A5A5A
K64 = fwc.K64


class WriteEmu:
    def __init__(self):
        so = os.path.join(BUILD, "libemu_frame_write.so")
        newest = max(os.path.getmtime(p) for p in DEPS)
        if not os.path.exists(so) or os.path.getmtime(so) < newest:
            os.makedirs(BUILD, exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-parameter", "-Wno-unknown-pragmas", "-o", so, SRC])
        L = self.L = C.CDLL(so)
        vp = C.c_void_p
        L.emu_write_frames.restype = None
        L.emu_write_frames.argtypes = [vp, vp, C.c_int64, C.c_int64, vp, C.c_int64, vp, C.c_int, vp, C.c_int64, vp, vp, vp, C.c_int, C.c_int]
        L.emu_frame_write_index_stream.restype = None
        L.emu_frame_write_index_stream.argtypes = [vp, C.c_int64, C.c_int, C.c_int, vp, vp, vp]
        L.emu_frame_write_set_descending.argtypes = [C.c_int]

    def write(self, c):
        """-> dict(info, frames, out_rec_off, out): the raw tables (the caller knows from info which entries count) and out[0 .. outCap);
        the bytes around all four outputs must come back untouched"""
        g = fwc.geometry(c)
        n, nf = g["n"], g["nf"]
        out = np.full(c.out_cap + 128, CANARY, dtype=np.uint8)
        tab = np.full((nf + 2) * 64, CANARY, dtype=np.uint8)
        off = np.full(n + 1 + 16, GUARD, dtype=np.int64)
        inf = np.full(32 * 3, CANARY, dtype=np.uint8)
        words = fwc.opts_words(c.opts)
        addr = lambda a: a.ctypes.data if a.size else None
        self.L.emu_write_frames(words.ctypes.data, addr(c.src), c.src_bytes, c.stride, addr(c.body), c.body_bytes, c.rec_off.ctypes.data, c.k,
                                out[64:].ctypes.data, c.out_cap, tab[64:].ctypes.data, off[8:].ctypes.data, inf[32:].ctypes.data,
                                min(c.waves, 1 << 20), c.slices)
        assert (out[:64] == CANARY).all() and (out[64 + c.out_cap:] == CANARY).all(), (c.name, "a store outside [out, out + outCap)")
        assert (tab[:64] == CANARY).all() and (tab[64 * (1 + nf):] == CANARY).all(), (c.name, "a store outside frames[0 .. nFrames)")
        assert (off[:8] == GUARD).all() and (off[8 + n + 1:] == GUARD).all(), (c.name, "a store outside outRecOff[0 .. nBlocks]")
        assert (inf[:32] == CANARY).all() and (inf[64:] == CANARY).all(), (c.name, "a store outside info")
        return dict(info=fwc.info_of(inf[32:64].view(fwc.INFO_DTYPE)[0]), frames=tab[64:64 * (1 + nf)], out_rec_off=off[8:8 + n + 1],
                    out=out[64:64 + c.out_cap])

    def index(self, stream, max_frames, max_recs):
        tab = np.zeros(max(max_frames, 1) * 64, dtype=np.uint8)
        off = np.zeros(max_recs + 1, dtype=np.int64)
        inf = np.zeros(32, dtype=np.uint8)
        self.L.emu_frame_write_index_stream(stream.ctypes.data, stream.size, max_frames, max_recs, tab.ctypes.data, off.ctypes.data, inf.ctypes.data)
        info = sic.info_of(inf.view(sic.INFO_DTYPE)[0])
        return sic.frames_of(tab.view(sic.FRAME_DTYPE), info["nFrames"]), off, info


def check(c, got, want):
    """what the call left against the model's answer"""
    assert got["info"] == want["info"], (c.name, got["info"], want["info"])
    if want["frames"] is None:                                  # NO_ROOM: nothing but info is written
        assert (got["frames"] == CANARY).all() and (got["out_rec_off"] == GUARD).all() and (got["out"] == CANARY).all(), (c.name, "written without room")
        return
    frames = sic.frames_of(got["frames"].view(sic.FRAME_DTYPE), len(want["frames"]))
    assert frames == want["frames"], (c.name, [(j, g, w) for j, (g, w) in enumerate(zip(frames, want["frames"])) if g != w][:1])
    assert np.array_equal(got["out_rec_off"], want["out_rec_off"]), c.name
    if want["stream"] is not None:
        start, end = want["start"], want["info"]["end"]
        assert np.array_equal(got["out"][start:end], want["stream"]), (c.name, "the stream")
        assert (got["out"][:start] == CANARY).all() and (got["out"][end:] == CANARY).all(), (c.name, "a store in front of or behind the stream")


@pytest.fixture(scope="module")
def emu():
    return WriteEmu()


@pytest.fixture(scope="module")
def the_cases(orc):
    """([(case, the model's answer)] of the good cases, the same of the failure cases): computed once"""
    good, bad = fwc.cases(orc)
    return [(c, fwc.model(orc, c)) for c in good], [(c, fwc.model(orc, c)) for c in bad]


def test_the_cases(emu, the_cases):
    good, bad = the_cases
    for c, want in good:
        assert want["info"]["status"] == fwc.OK, c.name
        check(c, emu.write(c), want)
    seen = set()
    for c, want in bad:
        check(c, emu.write(c), want)
        seen.add(want["info"]["status"])
    assert seen == {fwc.NO_ROOM, fwc.RECORD}


def test_lane_order_does_not_matter(emu, the_cases):
    try:
        emu.L.emu_frame_write_set_descending(1)
        for c, want in the_cases[0] + the_cases[1]:
            check(c, emu.write(c), want)
    finally:
        emu.L.emu_frame_write_set_descending(0)


def test_the_cases_say_what_they_are_named_for(the_cases):
    """against the case list itself, without the kernels"""
    good, bad = the_cases
    by_name = {c.name: (c, want) for c, want in good + bad}
    assert len(by_name) == len(good) + len(bad)
    shapes = {(fwc.geometry(c)["H"], fwc.geometry(c)["T"], c.opts["linked"]) for c, _ in good}
    assert shapes == {(h, t, l) for h in (7, 11, 15, 19) for t in (4, 8) for l in (0, 1)}
    assert {c.opts["linked"] for c, _ in good if c.k} == {0}
    # every misalignment of a moved record: (where it lands) - (where it lay) mod 16
    c, want = by_name["17 frames, 1 waves"]
    assert {int(v) % 16 for v in want["out_rec_off"][:17] - c.rec_off[:17]} == set(range(16))
    # stored and compressed records, in one frame and as frames of their own
    for name in ("17 frames, 1 waves", "k 0, 1 blocks, stride %d" % K64, "k 2, 5 blocks, stride %d" % fwc.GAP):
        c, _ = by_name[name]
        stored = [int.from_bytes(bytes(c.body[a:a + 4]), "little") >> 31 for a in c.rec_off[:-1]]
        assert stored[0] == 0 and (len(stored) < 2 or stored[1] == 1), name
    assert {w["info"]["nFrames"] for c, w in good if c.k == 1} >= {15, 16, 17, 33, 49}
    assert {(c.waves, w["info"]["nFrames"]) for c, w in good} >= {(1, 49), (2, 33), (3, 33), (3, 49), (2, 17)}
    _, want = by_name["k 0, 0 blocks, stride %d" % K64]
    assert want["stream"].size == 15 + 8 and bytes(want["stream"][-4:]) == (0x02CC5D05).to_bytes(4, "little") and want["frames"][0]["nRecs"] == 0
    assert by_name["1 bytes"][1]["frames"][0]["contentSum"] != 0 and by_name["two blocks and 15 bytes, k 1"][1]["info"]["nFrames"] == 3
    # the failures: the lowest bad record
    first = lambda name: (by_name[name][1]["info"]["status"], by_name[name][1]["info"]["firstBadRec"], by_name[name][1]["info"]["end"] >= 0)
    assert first("record 2 takes no room") == (fwc.RECORD, 2, True)
    assert first("records 1 and 3 take no room") == (fwc.RECORD, 1, True)
    assert first("record 0 takes no room, one frame") == (fwc.RECORD, 0, True)
    assert first("record 4 takes no room, k 1") == (fwc.RECORD, 4, True)
    assert first("size word above bsz") == first("stored size word above bsz") == (fwc.RECORD, 1, True)
    assert first("size word of 0xFFFFFFFF in record 3, of 0 in record 4") == (fwc.RECORD, 3, True)
    assert first("size word one short") == (fwc.RECORD, 2, True)
    assert first("block checksums assumed but absent") == first("block checksums present, not assumed") == (fwc.RECORD, 0, True)
    assert first("the body overflowed its cap by one byte") == (fwc.RECORD, 4, False)
    assert first("the body overflowed its cap by two records") == (fwc.RECORD, 2, False)
    assert first("a negative offset") == (fwc.RECORD, 1, True) and first("a first offset of -1") == (fwc.RECORD, 0, True)
    assert first("an offset that steps back") == (fwc.RECORD, 2, True) and first("an offset of 2^62") == (fwc.RECORD, 0, True)
    assert first("a last offset of -2^63") == first("a last offset of 2^63 - 1") == (fwc.RECORD, 4, False)
    assert by_name["records 1 and 3 take no room"][1]["frames"][1]["status"] == -1 - 3          # frame 1 = records 2, 3: marked with its own
    c, want = by_name["a base above 2^32"]
    assert want["info"] == dict(end=5 * (15 + 4) + int(c.rec_off[5]), nFrames=5, nRecs=5, status=fwc.NO_ROOM, firstBadRec=-1) and want["info"]["end"] > 1 << 32
    assert sum(w["info"]["status"] == fwc.NO_ROOM for _, w in bad) == 5


def test_one_frame_is_the_oracles_frame(emu, orc):
    """k = 0 over level-1 independent blocks: byte for byte what the oracle's writer makes of the plaintext"""
    recs = fwc.Records(orc)
    for bck in (False, True):
        for cck in (False, True):
            for src_bytes in (0, 1, K64, 3 * K64 + 17):
                c = fwc.good_case(recs, "oracle", fwc.opts(bck, cck), src_bytes, 0)
                got = emu.write(c)
                assert got["info"]["status"] == fwc.OK
                assert np.array_equal(got["out"], orc.frame_encode(np.array(fwc.shared_plaintext()[:src_bytes]), 4, bck, cck)), (bck, cck, src_bytes)


def test_the_stream_index_lists_what_the_writer_listed(emu, the_cases):
    """wave_index_stream over out: the same table, field by field, and the same recOff with its padding"""
    for c, want in the_cases[0]:
        got = emu.write(c)
        n, nf = want["info"]["nRecs"], want["info"]["nFrames"]
        start = want["start"]                                   # (the index counts from the stream's first byte)
        frames, rec_off, info = emu.index(np.ascontiguousarray(got["out"][start:want["info"]["end"]]), nf, n)
        assert (info["status"], info["end"] + start, info["nFrames"], info["nRecs"], info["nSkippable"]) == (sic.END, want["info"]["end"], nf, n, 0), c.name
        for f in frames:
            for key in ("hdrOff", "bodyOff", "end"):
                f[key] += start
        assert frames == sic.frames_of(got["frames"].view(sic.FRAME_DTYPE), nf), c.name
        assert np.array_equal(rec_off + (start if n else 0), got["out_rec_off"]), c.name


def test_the_host_layers_reader_reads_the_plaintext_back(emu, the_cases):
    from hostengine import oracle_engine
    from plz4_amd import host
    eng = oracle_engine()
    try:
        n = 0
        for c, want in the_cases[0]:
            if n > 60 and want["info"]["nFrames"] > 17:         # (the long streams once each is enough)
                continue
            got = emu.write(c)
            size, plain, err = host.Reader(eng, got["out"][want["start"]:want["info"]["end"]].tobytes()).write_to()
            assert int(err) == host.OK and size == c.src_bytes and plain == c.plaintext().tobytes(), (c.name, int(err))
            n += 1
        assert n > 60
    finally:
        eng.close()
