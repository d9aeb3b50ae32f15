"""The frame-body index on the lane-emulated build of its source (plz4_amd/csrc/lz4_body_index_device.inl, the walk behind
plz4hip_dev_index_body): recOff[0 .. maxBlocks] and info, exactly, against the model of FrameReader._read in body_index_cases.py,
against the offsets the bodies were laid out with, and against frames from the oracle's frame writer.  CPU only; what the walk reads
is the business of tests/emu/body_index_bounds_main.cpp (test_body_index_bounds.py)."""
import ctypes as C
import mmap
import os
import subprocess

import numpy as np
import pytest

import body_index_cases as bic
from orclib import ROOT

SRC = os.path.join(ROOT, "tests", "emu", "emu_body_index.cpp")
BUILD = os.path.join(ROOT, "tests", "emu", "_build")
DEPS = [SRC] + [os.path.join(ROOT, "plz4_amd", "csrc", f) for f in ("lz4_body_index_device.inl", "wave.h")]
GUARD = 0x5A5A5A5A5A5A5A5A


class Info(C.Structure):
    _fields_ = [("end", C.c_int64), ("nBlocks", C.c_int32), ("status", C.c_int32)]


class IndexEmu:
    def __init__(self):
        so = os.path.join(BUILD, "libemu_body_index.so")
        newest = max(os.path.getmtime(p) for p in DEPS)
        if not os.path.exists(so) or os.path.getmtime(so) < newest:
            os.makedirs(BUILD, exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-parameter", "-o", so, SRC])
        L = self.L = C.CDLL(so)
        L.emu_index_body.restype = None
        L.emu_index_body.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.emu_body_index_set_descending.argtypes = [C.c_int]

    def index(self, body_addr, body_bytes, bsz, checksum, max_blocks):
        """-> (recOff[0 .. max_blocks], end, nBlocks, status); the entries around recOff must come back untouched"""
        off = np.full(max_blocks + 1 + 16, GUARD, dtype=np.int64)
        info = Info(-7, -7, -7)
        self.L.emu_index_body(body_addr, body_bytes, bsz, int(checksum), max_blocks, off[8:].ctypes.data, C.addressof(info))
        assert (off[:8] == GUARD).all() and (off[8 + max_blocks + 1:] == GUARD).all(), "a store outside recOff[0 .. maxBlocks]"
        return off[8:8 + max_blocks + 1].copy(), int(info.end), int(info.nBlocks), int(info.status)


@pytest.fixture(scope="module")
def emu():
    return IndexEmu()


def _check(emu, body, body_bytes, bsz, checksum, max_blocks, what):
    want = bic.model(bic.word_of(body), body_bytes, bsz, checksum, max_blocks)
    got = emu.index(body.ctypes.data if body.size else None, body_bytes, bsz, checksum, max_blocks)
    assert np.array_equal(got[0], want[0]), what
    assert got[1:] == want[1:], (what, got[1:], want[1:])
    return got


@pytest.mark.parametrize("checksum", [False, True])
@pytest.mark.parametrize("bsz", bic.BSZS)
@pytest.mark.parametrize("n", bic.COUNTS)
def test_well_formed_bodies(emu, n, bsz, checksum):
    sizes, stored = bic.record_sizes(n, bsz, 100 + n)
    if n >= 2:
        assert any(s == 0 and st for s, st in zip(sizes, stored)) and (n < 63 or bsz in sizes)
    for end_mark, trailing in ((False, 0), (True, 0), (True, 4)):
        body, off = bic.build_body(sizes, stored, checksum, end_mark, trailing, seed=n)
        for mb in bic.max_blocks_of(n):
            rec_off, end, nb, status = _check(emu, body, body.size, bsz, checksum, mb, (n, bsz, checksum, end_mark, trailing, mb))
            # ... and against the layout itself, without the model
            k = min(n, mb)
            assert nb == k and np.array_equal(rec_off[:k + 1], off[:k + 1]) and (rec_off[k:] == off[k]).all()
            if mb < n:
                assert status == bic.FULL and end == off[mb]
            elif end_mark:
                assert status == bic.END_MARK and end == off[n] + 4
            else:
                assert status == bic.END_OF_BYTES and end == off[n] == body.size


@pytest.mark.parametrize("checksum", [False, True])
@pytest.mark.parametrize("bsz", bic.BSZS)
def test_hostile_bodies(emu, bsz, checksum):
    seen = set()
    for name, body, body_bytes in bic.hostile(bsz, checksum):
        for mb in (0, 3, 5, 6, 80):
            seen.add(_check(emu, body, body_bytes, bsz, checksum, mb, (name, mb))[3])
    assert seen == {bic.END_MARK, bic.END_OF_BYTES, bic.FULL, bic.SIZE_OVERFLOW, bic.TRUNCATED_WORD, bic.TRUNCATED_BLOCK}


def test_lane_order_does_not_matter(emu):
    sizes, stored = bic.record_sizes(129, 1024, 9)
    body, off = bic.build_body(sizes, stored, True, True, 4, seed=9)
    try:
        emu.L.emu_body_index_set_descending(1)
        for mb in bic.max_blocks_of(129):
            _check(emu, body, body.size, 1024, True, mb, mb)
    finally:
        emu.L.emu_body_index_set_descending(0)


@pytest.mark.parametrize("content_checksum", [False, True])
@pytest.mark.parametrize("block_checksum", [False, True])
def test_oracle_frames(emu, orc, block_checksum, content_checksum):
    """a frame from the oracle's writer, the header skipped: the walk lists its records, stops at the end mark and leaves `end`
    where the content checksum starts"""
    from plz4_amd import synth
    bsz = 64 << 10
    data = synth.make("M", 5 * bsz + 1234, bsz)
    frame = orc.frame_encode(data, 4, block_checksum, content_checksum)
    hdr = len(orc.frame_header(4, block_checksum=block_checksum, content_checksum=content_checksum))
    body = np.ascontiguousarray(frame[hdr:])
    recs = [orc.block_record(data[o:o + bsz], bsz, block_checksum) for o in range(0, data.size, bsz)]
    want_off = np.concatenate([[0], np.cumsum([r.size for r in recs])]).astype(np.int64)
    rec_off, end, nb, status = _check(emu, body, body.size, bsz, block_checksum, 6 + 70, "oracle frame")
    assert nb == 6 and status == bic.END_MARK and np.array_equal(rec_off[:7], want_off)
    assert end == want_off[6] + 4 == body.size - (4 if content_checksum else 0)
    for i, r in enumerate(recs):
        assert np.array_equal(body[rec_off[i]:rec_off[i + 1]], r), i


def test_offsets_beyond_4_gib(emu):
    """five records of about 1.1 GiB each in a sparse mapping that holds nothing but their size words: offsets pass 2^32 and stay
    exact; then a word that claims more than the bytes that are left, and one above bsz"""
    bsz = 0x7FFFFFFF
    sizes = [0x46000000 + 13 * k for k in range(5)]
    total = sum(4 + s for s in sizes)
    assert total > 5 << 30
    try:
        m = mmap.mmap(-1, total, flags=mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS | getattr(mmap, "MAP_NORESERVE", 0x4000))
    except (OSError, ValueError, OverflowError) as e:
        pytest.skip("a sparse mapping of %d bytes was refused: %s" % (total, e))
    try:
        words, pos = {}, 0
        for k, s in enumerate(sizes):
            w = s | (0x80000000 if k == 2 else 0)
            m[pos:pos + 4] = int(w).to_bytes(4, "little"); words[pos] = w
            pos += 4 + s
        buf = (C.c_char * total).from_buffer(m)
        addr = C.addressof(buf)
        want_off = np.concatenate([[0], np.cumsum([4 + s for s in sizes])]).astype(np.int64)
        assert want_off[4] > 1 << 32
        for mb in (4, 5, 70):
            want = bic.model(lambda o: words[o], total, bsz, False, mb)
            got = emu.index(addr, total, bsz, False, mb)
            assert np.array_equal(got[0], want[0]) and got[1:] == want[1:]
            k = min(mb, 5)
            assert np.array_equal(got[0][:k + 1], want_off[:k + 1]) and got[2] == k
            assert got[3] == (bic.FULL if mb < 5 else bic.END_OF_BYTES)
        # one byte short: the last record does not fit (need > bodyBytes - off, beyond 2^32 on both sides)
        got = emu.index(addr, total - 1, bsz, False, 8)
        assert got[1:] == (int(want_off[4]), 4, bic.TRUNCATED_BLOCK) and (got[0][4:] == want_off[4]).all()
        # with block checksums every record is four bytes longer than the layout: the walk steps into zeros -- an end mark
        want = bic.model(lambda o: words.get(o, 0), total, bsz, True, 8)
        got = emu.index(addr, total, bsz, True, 8)
        assert np.array_equal(got[0], want[0]) and got[1:] == want[1:] and got[3] == bic.END_MARK
        # a smaller bsz: the first word is above it
        got = emu.index(addr, total, 0x40000000, False, 8)
        assert got[1:] == (0, 0, bic.SIZE_OVERFLOW) and (got[0] == 0).all()
        del buf
    finally:
        try:
            m.close()
        except BufferError:
            pass
