"""The stream index on the lane-emulated build of its source (plz4_amd/csrc/lz4_stream_index_device.inl, the walk behind
plz4hip_dev_index_stream): info, every entry of the frame table, recOff with its padding and the untouched entries behind nFrames,
exactly, against the model of the header's table of steps in stream_index_cases.py; where every frame of a stream is a real one, the
first error of the host layer's Reader over the same bytes -- an implementation of its own -- must be the same verdict.  CPU only;
what the walk reads is the business of tests/emu/stream_index_bounds_main.cpp (test_stream_index_bounds.py)."""
import ctypes as C
import mmap
import os
import subprocess

import numpy as np
import pytest

import body_index_cases as bic
import stream_index_cases as sic
from orclib import ROOT

SRC = os.path.join(ROOT, "tests", "emu", "emu_stream_index.cpp")
BUILD = os.path.join(ROOT, "tests", "emu", "_build")
DEPS = [SRC] + [os.path.join(ROOT, "plz4_amd", "csrc", f) for f in ("lz4_stream_index_device.inl", "lz4_body_index_device.inl", "wave.h")]
GUARD = 0x5A5A5A5A5A5A5A5A
CANARY = 0xC7


class StreamEmu:
    def __init__(self):
        so = os.path.join(BUILD, "libemu_stream_index.so")
        newest = max(os.path.getmtime(p) for p in DEPS)
        if not os.path.exists(so) or os.path.getmtime(so) < newest:
            os.makedirs(BUILD, exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-parameter", "-o", so, SRC])
        L = self.L = C.CDLL(so)
        L.emu_index_stream.restype = None
        L.emu_index_stream.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.emu_stream_index_set_descending.argtypes = [C.c_int]

    def index(self, addr, n_bytes, max_frames, max_recs):
        """-> (frames, recOff[0 .. max_recs], info) as the model gives them; the entries behind nFrames, the entries around the
        table, around recOff and around info must come back untouched"""
        tab = np.full((max_frames + 2) * 64, CANARY, dtype=np.uint8)
        off = np.full(max_recs + 1 + 16, GUARD, dtype=np.int64)
        inf = np.full(32 * 3, CANARY, dtype=np.uint8)
        self.L.emu_index_stream(addr, n_bytes, max_frames, max_recs, tab[64:].ctypes.data, off[8:].ctypes.data, inf[32:].ctypes.data)
        assert (off[:8] == GUARD).all() and (off[8 + max_recs + 1:] == GUARD).all(), "a store outside recOff[0 .. maxRecs]"
        assert (inf[:32] == CANARY).all() and (inf[64:] == CANARY).all(), "a store outside info"
        info = sic.info_of(inf[32:64].view(sic.INFO_DTYPE)[0])
        nf = info["nFrames"]
        assert 0 <= nf <= max_frames
        assert (tab[:64] == CANARY).all() and (tab[64 * (1 + nf):] == CANARY).all(), "a store behind frames[nFrames) or in front of the table"
        return sic.frames_of(tab[64:64 * (1 + max_frames)].view(sic.FRAME_DTYPE), nf), off[8:8 + max_recs + 1].copy(), info


@pytest.fixture(scope="module")
def emu():
    return StreamEmu()


@pytest.fixture(scope="module")
def the_cases(orc):
    return sic.cases(orc)


def _check(emu, read, addr, n_bytes, max_frames, max_recs, what):
    want = sic.model(read, n_bytes, max_frames, max_recs)
    got = emu.index(addr, n_bytes, max_frames, max_recs)
    assert got[2] == want[2], (what, got[2], want[2])
    assert got[0] == want[0], (what, [(g, w) for g, w in zip(got[0], want[0]) if g != w][:1])
    assert np.array_equal(got[1], want[1]), what
    return got


def test_the_cases(emu, the_cases):
    seen = set()
    for c in the_cases:
        s = c.stream
        addr = s.ctypes.data if s.size else None
        frames, _, info = sic.model(sic.reader_of(s), s.size, *sic.ROOMY)
        assert info["nFrames"] < sic.ROOMY[0] and info["nRecs"] < sic.ROOMY[1], c.name
        for mf, mr in sic.sizes_of(c, frames, info):
            got = _check(emu, sic.reader_of(s), addr, s.size, mf, mr, (c.name, mf, mr))
            seen.add(got[2]["status"])
    assert seen == set(range(12)), "a case list that never reaches status %s" % (set(range(12)) - seen)


def test_the_headers_and_counts_are_what_the_cases_say(emu, the_cases, orc):
    """against the layout itself, without the model: the stream of all 128 headers lists 128 complete frames with the options they
    were written with, and the frames of 63, 1, 64, ... records list exactly those counts"""
    by_name = {c.name: c for c in the_cases}
    s = by_name["all 128 headers"].stream
    frames, rec_off, info = emu.index(s.ctypes.data, s.size, 130, 300)
    assert (info["status"], info["nFrames"], info["nRecs"], info["end"], info["nSkippable"]) == (sic.END, 128, 256, s.size, 0)
    assert info["maxBsz"] == 4 << 20 and info["flagsOr"] == 0x7D and info["flagsAnd"] == 0x40
    lens = set()
    for n, f in enumerate(frames):
        j, k = divmod(n, 32)
        linked, bck, cck, cs, did = sic.FLG_COMBOS[k]
        assert f["flags"] == 0x40 | (0 if linked else 0x20) | bck << 4 | cs << 3 | cck << 2 | did, n
        assert f["bsz"] == (64 << 10) << 2 * ((k + j) % 4) and f["blockDesc"] == (4 + (k + j) % 4) << 4
        assert f["contentSz"] == (0x0102030405060708 + k if cs else 0) and f["dictId"] == (0xA1B2C3D4 + k if did else 0)
        assert f["bodyOff"] - f["hdrOff"] == sic.header_len(cs, did) and (f["kind"], f["status"], f["nRecs"], f["firstRec"]) == (0, 0, 2, 2 * n)
        assert f["hdrOff"] == (frames[n - 1]["end"] if n else 0) and rec_off[2 * n] == f["bodyOff"]
        if cck:
            assert f["contentSum"] == int.from_bytes(bytes(s[f["end"] - 4:f["end"]]), "little")
        lens.add(f["bodyOff"] - f["hdrOff"])
    assert lens == {7, 11, 15, 19}
    s = by_name["frames of 63, 1, 64, 0, 65, 129, 0, 62 records"].stream
    frames, rec_off, info = emu.index(s.ctypes.data, s.size, 8, 384)
    assert [f["nRecs"] for f in frames] == [63, 1, 64, 0, 65, 129, 0, 62] and info["nRecs"] == 384 and info["status"] == sic.END
    assert [f["firstRec"] for f in frames] == [0, 63, 64, 128, 128, 193, 322, 322]
    assert (np.diff(rec_off[:384]) > 0).all() and rec_off[384] == frames[7]["end"] - 8          # end mark and trailer behind the last record


def test_lane_order_does_not_matter(emu, the_cases):
    try:
        emu.L.emu_stream_index_set_descending(1)
        for c in the_cases:
            if c.sizes is not None or c.name in ("all 128 headers", "seven real frames", "skippable in front, between and last"):
                s = c.stream
                frames, _, info = sic.model(sic.reader_of(s), s.size, *sic.ROOMY)
                for mf, mr in sic.sizes_of(c, frames, info):
                    _check(emu, sic.reader_of(s), s.ctypes.data if s.size else None, s.size, mf, mr, (c.name, mf, mr))
    finally:
        emu.L.emu_stream_index_set_descending(0)


def test_real_frames_list_the_oracles_records(emu, orc):
    """frames from the oracle's writer with skippable frames among them: every listed record is the oracle's record of its block,
    the content checksum the oracle's xxh32 of the plaintext, content size and dictionary id what the header was written with"""
    real = sic.oracle_frames(orc)
    parts, where = [], []
    for k, (f, data, _) in enumerate(real):
        if k % 2:
            parts.append(sic.skippable(k, 10 * k))
        where.append(sum(p.size for p in parts))
        parts.append(f)
    s = sic.cat(*parts)
    frames, rec_off, info = _check(emu, sic.reader_of(s), s.ctypes.data, s.size, 20, 40, "real frames")
    assert (info["status"], info["end"], info["nSkippable"], info["nFrames"]) == (sic.END, s.size, 3, len(real) + 3)
    lz4 = [f for f in frames if f["kind"] == 0]
    assert [f["hdrOff"] for f in lz4] == where
    for f, (raw, data, _) in zip(lz4, real):
        assert f["nRecs"] == 1 and f["status"] == bic.END_MARK and f["end"] == f["hdrOff"] + raw.size
        rec = orc.block_record(data, 64 << 10, bool(f["flags"] & 16))
        at = int(rec_off[f["firstRec"]])
        assert np.array_equal(s[at:at + rec.size], rec)
        if f["flags"] & 4:
            assert f["contentSum"] == orc.xxh32(data)
        if f["flags"] & 8:
            assert f["contentSz"] == data.size
    assert [f["dictId"] for f in lz4][-2:] == [77, 0xFFFFFFFF]


# the first error of the reference's reader, as the host layer restates it, and the verdict it corresponds to
def _verdict_of(host, err):
    return {host.OK: (sic.END, None), host.ErrHeaderRead: (sic.HEADER_READ, None), host.ErrMagic: (sic.MAGIC, None),
            host.ErrSkip: (sic.SKIP, None), host.ErrContentHashRead: (sic.CONTENT_HASH_READ, None),
            host.ErrBlockSizeRead: (sic.BODY, bic.TRUNCATED_WORD), host.ErrBlockRead: (sic.BODY, bic.TRUNCATED_BLOCK),
            host.ErrBlockSizeOverflow: (sic.BODY, bic.SIZE_OVERFLOW), host.ErrHeaderHash: (sic.HEADER_HASH, None),
            host.ErrVersion: (sic.VERSION, None), host.ErrReserveBitSet: (sic.RESERVED_BIT, None),
            host.ErrBlockDescriptor: (sic.BLOCK_DESCRIPTOR, None)}[int(err)]


def test_the_host_layers_reader_gives_the_same_verdict(emu, the_cases, orc):
    from hostengine import oracle_engine
    from plz4_amd import host
    eng = oracle_engine()
    try:
        n = 0
        seen = set()
        for c in the_cases:
            if not c.decodable:
                continue
            s = c.stream
            _, _, err = host.Reader(eng, s.tobytes()).write_to()
            frames, _, info = emu.index(s.ctypes.data if s.size else None, s.size, *sic.ROOMY)
            got = (info["status"], frames[-1]["status"] if info["status"] == sic.BODY else None)
            assert got == _verdict_of(host, err), (c.name, got, int(err))
            seen.add(got[0]); n += 1
        assert n > 60 and seen >= {sic.END, sic.HEADER_READ, sic.MAGIC, sic.SKIP, sic.CONTENT_HASH_READ, sic.BODY}
        # bad headers in front of a real block section: the reader stops at the header, as the walk does
        real = sic.oracle_frames(orc)[3][0]
        for at, value in ((0, 5), (4, real[4] & 0x3F), (4, real[4] | 0x80), (4, real[4] | 2), (5, 0x30), (5, 0xC0), (5, 0x41), (6, real[6] ^ 1)):
            s = real.copy(); s[at] = value
            _, _, err = host.Reader(eng, s.tobytes()).write_to()
            frames, _, info = emu.index(s.ctypes.data, s.size, *sic.ROOMY)
            assert (info["status"], None) == _verdict_of(host, err) and info["status"] not in (sic.END, sic.BODY), (at, value)
    finally:
        eng.close()


def test_offsets_beyond_4_gib(emu, orc):
    """a small frame, two skippable frames in a row of 3 GiB and 2.5 GiB, a small frame, in a sparse mapping that holds nothing
    but the frames and the two 8-byte headers: offsets pass 2^32 and stay exact; then the stream one byte short of the second
    skippable frame's end (PLZ4HIP_STREAM_SKIP beyond 2^32), and cut inside the last frame"""
    a, b = sic.made_frame(orc, 3, 4, bck=True, cck=True, seed=5), sic.made_frame(orc, 2, 7, cck=True, seed=6)
    s1, s2 = 3 << 30, (5 << 29) + 13
    at_s1, at_s2, at_b = a.size, a.size + 8 + s1, a.size + 16 + s1 + s2
    total = at_b + b.size
    assert total > (11 << 29) and at_s2 < 1 << 32 < at_b
    try:
        m = mmap.mmap(-1, total, flags=mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS | getattr(mmap, "MAP_NORESERVE", 0x4000))
    except (OSError, ValueError, OverflowError) as e:
        pytest.skip("a sparse mapping of %d bytes was refused: %s" % (total, e))
    try:
        m[0:a.size] = a.tobytes()
        m[at_s1:at_s1 + 8] = (0x184D2A5C).to_bytes(4, "little") + s1.to_bytes(4, "little")
        m[at_s2:at_s2 + 8] = (0x184D2A51).to_bytes(4, "little") + s2.to_bytes(4, "little")
        m[at_b:total] = b.tobytes()
        buf = (C.c_char * total).from_buffer(m)
        addr = C.addressof(buf)
        read = lambda off, n: m[off:off + n]
        for mf, mr in ((4, 5), (6, 80), (3, 5), (4, 4)):
            frames, rec_off, info = _check(emu, read, addr, total, mf, mr, ("sparse", mf, mr))
        frames, rec_off, info = _check(emu, read, addr, total, 4, 5, "sparse")
        assert (info["status"], info["end"], info["nFrames"], info["nSkippable"], info["nRecs"]) == (sic.END, total, 4, 2, 5)
        assert [(f["kind"], f["nibble"], f["hdrOff"], f["contentSz"]) for f in frames[1:3]] == [(1, 12, at_s1, s1), (1, 1, at_s2, s2)]
        assert frames[3]["hdrOff"] == at_b and frames[3]["firstRec"] == 3 and rec_off[3] == at_b + 7 and frames[3]["end"] == total
        frames, rec_off, info = _check(emu, read, addr, at_b - 1, 4, 5, "sparse, one byte short of the skippable frame")
        assert (info["status"], info["end"], info["nFrames"]) == (sic.SKIP, at_s2, 2) and (rec_off[3:] == frames[0]["end"] - 8).all()
        frames, rec_off, info = _check(emu, read, addr, total - 5, 4, 5, "sparse, cut in the end mark")
        assert (info["status"], frames[3]["status"], info["end"]) == (sic.BODY, bic.TRUNCATED_WORD, total - 8)
        del buf
    finally:
        try:
            m.close()
        except BufferError:
            pass
