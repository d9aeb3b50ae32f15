"""The two frame-format rules every block encoder kernel shares (plz4_amd/csrc/lz4_block_io.inl) on the lane-emulated build of the
same source (tests/emu/emu_block_io.cpp).
(a) How block i of a call is primed -- hist_of, l1_prime, hc_prime, hc_pfx -- gives what the per-kernel copies it replaced gave:
tests/golden/prime_parent.json, written once by a program that carried those conditions verbatim (make_prime_golden.py); the table
itself covers every mode of both encoders and both sides of every threshold.
(b) The rule driving the emulated encoders over a list of blocks, laid out as the kernels find them, gives the reference's streams:
the oracle's compress_indie_dict / compress_linked at level 1, the real liblz4 (hcdict.ref_records' way) at levels 2, 3, 9, 12.
(c) The record writer, wave_finish_record, gives Oracle.block_record's bytes and length, in both lane orders."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import hcdict
from orclib import ROOT, Ref, _ptr, u8p
from plz4_amd import synth

SRC = os.path.join(ROOT, "tests", "emu", "emu_block_io.cpp")
SO = os.path.join(ROOT, "tests", "emu", "_build", "libemu_block_io.so")
DEPS = [SRC] + [os.path.join(ROOT, "plz4_amd", "csrc", f) for f in ("lz4_block_io.inl", "lz4_device.inl", "lz4hc_device.inl", "wave.h")]
GOLDEN = os.path.join(ROOT, "tests", "golden", "prime_parent.json")
PAD = 65536                                                            # the scratch in front of every block
SENTINEL = 0xA5
i32p = C.POINTER(C.c_int32)
NULL = C.cast(None, u8p)

# the enums of lz4_device.inl / lz4hc_device.inl
L1_MODES = {"kDictFreshPrefix": 0, "kDictLoad": 1, "kDictCtxCopy": 2, "kDictCtxLookup": 3, "kDictNonePrefix": 4}
HC_MODES = {"kHcNone": 0, "kHcExt": 1, "kHcCtx": 2}


class BlockIo:
    def __init__(self):
        if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(p) for p in DEPS):
            os.makedirs(os.path.dirname(SO), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-parameter", "-o", SO, SRC])
        L = self.L = C.CDLL(SO)
        L.bio_prime_row.argtypes = [C.c_int] * 7 + [C.POINTER(C.c_longlong)]
        L.bio_encode.argtypes = [C.c_void_p, C.c_longlong, i32p, C.c_int, C.c_int, C.c_int, C.c_int, u8p, C.c_int, u8p, C.c_int, C.c_void_p,
                                 u8p, C.c_longlong, C.c_int, i32p, C.c_int]
        L.bio_block_record.argtypes = [u8p, C.c_int, C.c_int, C.c_int, u8p, i32p]
        L.bio_finish_record.argtypes = [u8p, u8p, C.c_int, C.c_int, C.c_int]

    def prime_row(self, inputs):
        out = (C.c_longlong * 10)()
        assert self.L.bio_prime_row(*inputs, out) == 0, inputs
        return list(out)

    def encode(self, blocks, cap, level, raw=False, linked=False, prev_tail=None, dct=None, table=None, order=0):
        """The blocks' (return value, bytes).  Every block gets PAD bytes of scratch in front of it and sentinel bytes behind its
        capacity; the plaintext must come back untouched."""
        nb = len(blocks)
        stride = PAD + max(b.size for b in blocks) + 256
        src = np.full(nb * stride + 256, 0xA7, dtype=np.uint8)
        for i, b in enumerate(blocks):
            src[i * stride + PAD:i * stride + PAD + b.size] = b
        lens = np.array([b.size for b in blocks], dtype=np.int32)
        dstride = cap + 64
        dst = np.full(nb * dstride, SENTINEL, dtype=np.uint8)
        res = np.zeros(nb, dtype=np.int32)
        d64 = None if dct is None else np.concatenate([dct[-65536:], np.zeros(64, dtype=np.uint8)])     # (the encoders read words)
        self.L.bio_set_descending(order)
        try:
            rc = self.L.bio_encode(src.ctypes.data + PAD, stride, lens.ctypes.data_as(i32p), nb, level, int(raw), int(linked),
                                   NULL if prev_tail is None or not prev_tail.size else _ptr(prev_tail), -1 if prev_tail is None else prev_tail.size,
                                   NULL if d64 is None else _ptr(d64), -1 if d64 is None else d64.size - 64,
                                   None if table is None else C.cast(C.byref(table), C.c_void_p), _ptr(dst), dstride, cap, res.ctypes.data_as(i32p), order)
        finally:
            self.L.bio_set_descending(0)
        assert rc == 0
        for i, b in enumerate(blocks):
            assert np.array_equal(src[i * stride + PAD:i * stride + PAD + b.size], b), "block %d's plaintext changed" % i
            assert np.all(dst[i * dstride + cap:(i + 1) * dstride] == SENTINEL), "block %d: bytes behind its capacity" % i
        return [(int(res[i]), dst[i * dstride:i * dstride + max(int(res[i]), 0)].copy()) for i in range(nb)]


@pytest.fixture(scope="module")
def bio():
    return BlockIo()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    g["in"], g["out"] = g["in"].split(), g["out"].split()
    return g


# ---------------------------------------------------------------------------------------------------------------- (a) the table
def test_same_answers_as_the_copies_it_replaced(bio, golden):
    n_in = len(golden["in"])
    assert golden["in"] == "raw linked i prevTailLen dictLen prevLen n".split()
    for row in golden["cases"]:
        assert len(row) == n_in + len(golden["out"])
        inputs = [5 if v is None else v for v in row[:n_in]]             # (null: the rule does not read block i - 1's length)
        got = bio.prime_row(inputs)
        assert got == row[n_in:], (dict(zip(golden["in"], row[:n_in])), dict(zip(golden["out"], got)), dict(zip(golden["out"], row[n_in:])))
        if row[5] is None:                                               # ... and does not read it indeed
            inputs[5] = 70000
            assert bio.prime_row(inputs) == row[n_in:], row


def test_table_covers_every_mode_and_both_sides_of_every_threshold(bio, golden):
    rows = [dict(zip(golden["in"] + golden["out"], r)) for r in golden["cases"]]
    assert 2000 <= len(rows) <= 5000

    def some(**kv):
        return any(all(r[k] == v for k, v in kv.items()) for r in rows)

    for raw in (0, 1):
        for name, m in L1_MODES.items():
            if not (raw and name in ("kDictFreshPrefix", "kDictLoad")):   # (the block API has no linked mode and no fresh stream)
                assert some(raw=raw, l1Mode=m), (raw, name)
        for name, m in HC_MODES.items():
            assert some(raw=raw, hcMode=m), (raw, name)
        assert not some(raw=raw, l1Mode=L1_MODES["kDictFreshPrefix"]) or not raw
        # the dictionary: none / attached and empty / dropped (7) / kept (8); the 4 KiB bar on both sides, at levels 1 and 2..12
        assert some(raw=raw, dictLen=-1, hcMode=0, isCtx=0) and some(raw=raw, dictLen=0, hcMode=2, hcLen=0, isCtx=1, hcPfx=-1)
        assert some(raw=raw, dictLen=0, n=4097, hcMode=1, hcLen=0, hcPfx=0)
        assert some(raw=raw, dictLen=7, l1Mode=4, l1Size=0) and some(raw=raw, dictLen=7, hcMode=1, hcLen=7, hcBytes=2)
        assert some(raw=raw, dictLen=8, n=4096, l1Mode=3, l1Size=8, l1Bytes=2, isCtx=1) and some(raw=raw, dictLen=8, n=4097, l1Mode=2, l1Bytes=2, isCtx=0, hcPfx=8)
    assert bio.L.bio_ctx_max_block() == 4096
    # linked: prevTail of -1 / 0 / 7 / 8 bytes in front of block 0, with and without a dictionary behind it
    assert some(raw=0, linked=1, i=0, prevTailLen=-1, dictLen=-1, l1Mode=0, hcMode=0, hcPfx=0)
    assert some(raw=0, linked=1, i=0, prevTailLen=-1, dictLen=65536, n=4096, l1Mode=3, hcMode=2)
    for dl in (-1, 65536):
        assert some(raw=0, linked=1, i=0, prevTailLen=0, dictLen=dl, l1Mode=4, hcMode=1, hcLen=0, hcBytes=1, isCtx=0)
        assert some(raw=0, linked=1, i=0, prevTailLen=7, dictLen=dl, l1Mode=4, l1Bytes=0, hcMode=1, hcLen=7)
        assert some(raw=0, linked=1, i=0, prevTailLen=8, dictLen=dl, l1Mode=1, l1Size=8, l1Bytes=1, hcLen=8)
    # ... the tail of the block before: all of a short one, the last 64 KiB of a long one
    for i in (1, 2):
        for pl, size, off in ((0, 0, None), (7, 0, None), (8, 8, 0), (65535, 65535, 0), (65536, 65536, 0), (70000, 65536, 4464)):
            kv = dict(raw=0, linked=1, i=i, prevLen=pl, l1Size=size, hcLen=min(pl, 65536), hcBytes=3, hcOff=max(pl - 65536, 0))
            if off is not None:
                kv.update(l1Mode=1, l1Bytes=3, l1Off=off)
            assert some(**kv), kv
    assert [bio.L.bio_tail_len(pl) for pl in (0, 7, 65535, 65536, 65537, 70000)] == [0, 7, 65535, 65536, 65536, 65536]
    # the block API sees no linked mode, independent records no tail
    assert not some(raw=1, l1Mode=1) and not some(raw=1, hcBytes=1) and not some(raw=1, hcBytes=3)
    assert not some(linked=0, l1Mode=1) and not some(linked=0, hcBytes=3)


# --------------------------------------------------------------------------------------------- (b) the rule, end to end
SIZES = (0, 13, 4096, 4097, 70000)
CAP = 70000                                                             # records: capacity == block size
# (dictionary bytes or None, linked, bytes of prevTail or None)
CALLS = [(d, False, None) for d in (65536, 7)] + [(d, True, t) for d in (None, 65536, 7) for t in (None, 0, 7, 8)]


@pytest.fixture(scope="module")
def blocks():
    text = synth.text(sum(SIZES) + 70000, seed=43)
    out, at = [], 0
    for n in SIZES:
        out.append(np.ascontiguousarray(text[at:at + n])); at += n
    return out


def _call(d, t):
    user = synth.text(70000, seed=42)                                   # (shares vocabulary with the blocks)
    dct = None if d is None else np.ascontiguousarray(user[70000 - d:])
    tail = None if t is None else np.ascontiguousarray(synth.text(70000, seed=44)[70000 - t:])
    return dct, tail


@pytest.mark.parametrize("d,linked,t", CALLS)
def test_level1_streams_are_the_oracles(orc, bio, blocks, d, linked, t):
    dct, tail = _call(d, t)
    dctx = None if dct is None else orc.dict_ctx(dct)
    want = []
    for i, b in enumerate(blocks):
        if not linked:
            want.append(orc.compress_indie_dict(b, CAP, dctx))
        else:
            prev = tail if i == 0 else blocks[i - 1][-65536:].copy()
            want.append(orc.compress_linked(b, CAP, prev, dctx if prev is None else None))
    for order in (0, 1):
        got = bio.encode(blocks, CAP, 1, linked=linked, prev_tail=tail, dct=dct, table=dctx, order=order)
        assert [g[0] for g in got] == [w[0] for w in want], (d, linked, t, order)
        for i, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(g[1], w[1][:w[0]]), (d, linked, t, order, i)
    if not linked:                                                      # the block API under the same dictionary: the same blocks
        got = bio.encode(blocks, CAP, 1, raw=True, dct=dct, table=dctx)
        assert [(g[0], g[1].tobytes()) for g in got] == [(w[0], w[1][:w[0]].tobytes()) for w in want]


@pytest.mark.skipif(not Ref.available(), reason="the reference's liblz4 is not built")
@pytest.mark.parametrize("level", (2, 3, 9, 12))
@pytest.mark.parametrize("d,linked,t", CALLS)
def test_hc_streams_are_liblz4s(ref, orc, bio, blocks, d, linked, t, level):
    dct, tail = _call(d, t)
    if tail is None:
        recs, rets = hcdict.ref_records(ref, orc, blocks, CAP, level, linked, dct, checksum=False)
        want = [(r, np.frombuffer(rec, dtype=np.uint8)[4:]) for r, rec in zip(rets, recs)]
    else:                                                               # ref_records' linked loop with a window in front of block 0
        daddr = None
        if dct is not None:
            keep, daddr = ref.new_dict_ctx_hc(dct, level)
        comp = ref.stream_linked_ctx_hc(level, daddr)
        want, prev = [], tail
        for b in blocks:
            want.append(comp(b, CAP, prev.copy())); prev = b[-65536:]
    got = bio.encode(blocks, CAP, level, linked=linked, prev_tail=tail, dct=dct)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0], (level, d, linked, t, i)
        if w[0]:
            assert np.array_equal(g[1], w[1][:w[0]]), (level, d, linked, t, i)


# ------------------------------------------------------------------------------------------------------ (c) the record writer
def _payloads():
    rng = np.random.default_rng(7)
    for n in (0, 1, 13, 65536):
        yield "text", np.ascontiguousarray(synth.text(65536, seed=3)[:n])
        yield "zeros", np.zeros(n, dtype=np.uint8)
        yield "random", rng.integers(0, 256, n, dtype=np.uint8)


@pytest.mark.parametrize("order", (0, 1))
@pytest.mark.parametrize("checksum", (False, True))
def test_finish_record_is_the_oracles_record(orc, bio, checksum, order):
    bsz = 65536
    bio.L.bio_set_descending(order)
    try:
        for kind, src in _payloads():
            want = orc.block_record(src if src.size else np.zeros(1, dtype=np.uint8)[:0], bsz, checksum)
            rec = np.full(bsz + 8 + 64, SENTINEL, dtype=np.uint8)
            c = C.c_int32(-1)
            n = bio.L.bio_block_record(_ptr(src) if src.size else NULL, src.size, bsz, int(checksum), _ptr(rec), C.byref(c))
            assert n == want.size and np.array_equal(rec[:n], want), (kind, src.size, checksum, order)
            assert np.all(rec[n:] == SENTINEL), (kind, src.size)
            stored = bool(rec[3] & 0x80)
            assert stored == (c.value == 0)
            if kind == "random" and src.size == 65536:
                assert stored and n == 4 + src.size + (4 if checksum else 0)
            if kind == "zeros" and src.size == 65536:
                assert not stored
    finally:
        bio.L.bio_set_descending(0)
