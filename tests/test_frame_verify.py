"""The frame verdicts on the lane-emulated build of their source (plz4_amd/csrc/lz4_frame_verify_device.inl, the walk behind
plz4hip_dev_verify_frames): every verdict and the stream verdict, exactly, against the model of the header's table of rules in
frame_verify_cases.py, in both lane orders, with canaries around both outputs and in the entries behind nFrames; over real frames
from the oracle's writer, the first error of the host layer's Reader over the same bytes -- an implementation of its own -- must be
the same one.  CPU only; what the walk reads is the business of tests/emu/frame_verify_bounds_main.cpp (test_frame_verify_bounds.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import frame_verify_cases as fvc
import stream_index_cases as sic
from orclib import ROOT

SRC = os.path.join(ROOT, "tests", "emu", "emu_frame_verify.cpp")
BUILD = os.path.join(ROOT, "tests", "emu", "_build")
DEPS = [SRC] + [os.path.join(ROOT, "plz4_amd", "csrc", f) for f in ("lz4_frame_verify_device.inl", "lz4_stream_index_device.inl",
                                                                    "lz4_body_index_device.inl", "lz4_device.inl", "wave.h")]
CANARY = fvc.CANARY


class VerifyEmu:
    def __init__(self):
        so = os.path.join(BUILD, "libemu_frame_verify.so")
        newest = max(os.path.getmtime(p) for p in DEPS)
        if not os.path.exists(so) or os.path.getmtime(so) < newest:
            os.makedirs(BUILD, exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-parameter", "-o", so, SRC])
        L = self.L = C.CDLL(so)
        L.emu_verify_frames.restype = None
        L.emu_verify_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                        C.c_void_p, C.c_void_p, C.c_int]
        L.emu_frame_verify_set_descending.argtypes = [C.c_int]

    def verify(self, c):
        """-> (verdicts, sv) as the model gives them; the entries behind nFrames and the bytes around both outputs must come back
        untouched.  The grid: what plz4hip_dev_verify_frames launches, min(ceil(maxFrames / 16), the cap)."""
        mf = c.max_frames
        ver = np.full((mf + 2) * 32, CANARY, dtype=np.uint8)
        svb = np.full(32 * 3, CANARY, dtype=np.uint8)
        waves = min((mf + 15) // 16, c.waves or 1 << 20)
        addr = lambda a: a.ctypes.data if a.size else None
        self.L.emu_verify_frames(addr(c.frames), c.info.ctypes.data, mf, addr(c.dst), c.stride, c.cap, addr(c.result), addr(c.status),
                                 c.max_recs, ver[32:].ctypes.data, svb[32:].ctypes.data, waves)
        assert (svb[:32] == CANARY).all() and (svb[64:] == CANARY).all(), "a store outside sv"
        sv = fvc.sv_of(svb[32:64].view(fvc.SV_DTYPE)[0])
        nf = sv["nFrames"]
        assert 0 <= nf <= mf
        assert (ver[:32] == CANARY).all() and (ver[32 * (1 + nf):] == CANARY).all(), "a store behind verdicts[nFrames) or in front of them"
        return fvc.verdicts_of(ver[32:32 * (1 + mf)].view(fvc.VERDICT_DTYPE), nf), sv


@pytest.fixture(scope="module")
def emu():
    return VerifyEmu()


@pytest.fixture(scope="module")
def the_cases(orc):
    """[(case, the model's verdicts, the model's stream verdict)]: computed once"""
    return [(c,) + fvc.model(orc, c) for c in fvc.cases(orc)]


def _check(emu, c, want, want_sv):
    got, sv = emu.verify(c)
    assert sv == want_sv, (c.name, sv, want_sv)
    assert got == want, (c.name, [(j, g, w) for j, (g, w) in enumerate(zip(got, want)) if g != w][:1])


def test_the_cases(emu, the_cases):
    seen = set()
    for c, want, want_sv in the_cases:
        _check(emu, c, want, want_sv)
        seen |= {v["status"] for v in want}
    assert seen == set(range(7)), "a case list that never reaches status %s" % (set(range(7)) - seen)


def test_lane_order_does_not_matter(emu, the_cases):
    try:
        emu.L.emu_frame_verify_set_descending(1)
        for c, want, want_sv in the_cases:
            _check(emu, c, want, want_sv)
    finally:
        emu.L.emu_frame_verify_set_descending(0)


def test_the_cases_say_what_they_are_named_for(the_cases):
    """against the case list itself, without the kernel: the model's answers are the ones the cases were built for"""
    by_name = {c.name: (want, sv) for c, want, sv in the_cases}
    want, sv = by_name["every verdict"]
    S = fvc
    assert [v["status"] for v in want] == [S.SKIPPABLE, S.OK, S.BLOCK, S.SKIPPABLE, S.BLOCK, S.BLOCK, S.RANGE, S.RANGE, S.OK, S.CONTENT_HASH,
                                           S.CONTENT_SIZE, S.OK, S.OK, S.CONTENT_SIZE, S.OK, S.RANGE, S.RANGE, S.RANGE, S.RANGE, S.SKIPPABLE,
                                           S.BLOCK, S.RANGE, S.BLOCK, S.RANGE, S.CONTENT_HASH, S.SKIPPABLE, S.INCOMPLETE, S.SKIPPABLE]
    assert [(v["firstBad"], v["blockStatus"], v["contentSz"]) for v in want[2:8]] == [(3, 1, 0), (-1, 0, 0), (7, 3, 10), (11, 2, 30), (13, 0, 10),
                                                                                      (17, 0, 30)]
    assert (sv["firstBadFrame"], sv["status"], sv["contentBytes"], sv["nOk"], sv["nSkippable"]) == (2, S.BLOCK, 350, 5, 5)
    for v in want:                                              # every frame of 40 + 50 bytes that was walked to its end
        assert v["contentSz"] in (0, 10, 30, 40, 60, 90, 350, 600)
    assert want[26]["contentSum"] == 0 and want[26]["contentSz"] == 90
    want, sv = by_name["one record beyond maxRecs"]
    assert [v["status"] for v in want] == [S.OK, S.RANGE] and want[1]["firstBad"] == -1 and sv["contentBytes"] == 30
    want, sv = by_name["seventy frames, the 67th bad"]
    assert (sv["firstBadFrame"], sv["status"], sv["nOk"], sv["nSkippable"]) == (66, S.CONTENT_HASH, 54, 14)
    want, sv = by_name["every verdict, info->nFrames above maxFrames"]
    assert sv["nFrames"] == len(want) == 25
    for name in ("every verdict, info->nFrames negative", "every verdict, maxFrames 0", "no frames"):
        assert by_name[name] == ([], dict(contentBytes=0, firstBadFrame=-1, status=0, nFrames=0, nOk=0, nSkippable=0))
    assert by_name["17 frames, 1 waves"][1]["nOk"] == 17 and by_name["49 frames, 3 waves"][1]["nOk"] == 49
    empty = by_name["runs of tiny pieces, empty frames, totals below a stripe"][0]
    assert empty[8]["contentSum"] == 0x02CC5D05 and empty[8]["status"] == S.OK      # xxh32 of no bytes, seed 0


# the first error of the reference's reader, as the host layer restates it, and the stream verdict it corresponds to
def _status_of(host, err):
    return {host.OK: 0, host.ErrContentHash: fvc.CONTENT_HASH, host.ErrContentSize: fvc.CONTENT_SIZE}[int(err)]


def test_the_host_layers_reader_gives_the_same_verdict(emu, orc):
    from hostengine import oracle_engine
    from plz4_amd import host
    eng = oracle_engine()
    try:
        real = sic.oracle_frames(orc)
        # (the frames with a content size stand last: the reference's reader keeps a header's content size for the frames behind it
        # that carry none -- rdr.go:287-292 never clears it -- where the call compares a size only with its own frame's header)
        good = [real[2][0], sic.skippable(2, 9), real[3][0], real[1][0], real[4][0], real[6][0]]
        datas = [real[2][1], None, real[3][1], real[1][1], real[4][1], real[6][1]]
        seen = set()

        def run(parts, what, bad_frame):
            s = sic.cat(*parts)
            c, info = fvc.decoded_case(orc, s, what)
            assert info["status"] == sic.END and info["nFrames"] == len(parts)
            want, want_sv = fvc.model(orc, c)
            _check(emu, c, want, want_sv)
            n, plain, err = host.Reader(eng, s.tobytes()).write_to()
            assert want_sv["status"] == _status_of(host, err), (what, want_sv, int(err))
            assert want_sv["firstBadFrame"] == bad_frame, (what, want_sv)
            if bad_frame < 0:
                assert want_sv["contentBytes"] == n == sum(d.size for d in datas if d is not None)
                assert plain == b"".join(d.tobytes() for d in datas if d is not None)
                assert want_sv["nOk"] == len(parts) - 1 and want_sv["nSkippable"] == 1
                for v, d in zip(want, datas):
                    assert d is None or v["contentSz"] == d.size
            seen.add(want_sv["status"])

        run(good, "real frames", -1)
        # a stored content checksum flipped: frames 0, 2, 4, 5 store one
        for k in (0, 2, 4, 5):
            parts = [p.copy() for p in good]
            parts[k][-1] ^= 0x40
            run(parts, "checksum of frame %d flipped" % k, k)
        # a content size off by one: frames 4 and 5 carry one (header: FLG, BD, 8 bytes of size, [dict id,] the hash byte)
        for k, hlen in ((4, 15), (5, 19)):
            for delta in (1, -1):
                parts = [p.copy() for p in good]
                size = int.from_bytes(bytes(parts[k][6:14]), "little") + delta
                parts[k][6:14] = np.frombuffer(size.to_bytes(8, "little"), dtype=np.uint8)
                sic.rehash(parts[k], hlen)
                run(parts, "content size of frame %d off by %d" % (k, delta), k)
        # both at once: the hash is reported, as the reference does
        parts = [p.copy() for p in good]
        parts[4][-2] ^= 1
        parts[4][6] ^= 1
        sic.rehash(parts[4], 15)
        run(parts, "checksum and size of frame 4 wrong", 4)
        assert seen == {0, fvc.CONTENT_HASH, fvc.CONTENT_SIZE}
    finally:
        eng.close()
