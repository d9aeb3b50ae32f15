"""The frame-body index (plz4hip_dev_index_body) for the CPU and the GPU tests: a model of FrameReader._read's size-word walk
(internal/pkg/blk/frame.go:54-98), written from the table of rules in include/plz4hip.h and from nothing else, the bodies the tests
walk, and the hostile set.  Test infrastructure only."""
from __future__ import annotations

import numpy as np

END_MARK, END_OF_BYTES, FULL, SIZE_OVERFLOW, TRUNCATED_WORD, TRUNCATED_BLOCK = 0, 1, 2, 3, 4, 5

COUNTS = [0, 1, 2, 63, 64, 65, 128, 129, 200]          # records: on the edges of the 64-entry store groups
BSZS = [1024, 65536]


def word_of(body: np.ndarray):
    """the LE32 at an offset of a uint8 array"""
    return lambda off: int(body[off]) | int(body[off + 1]) << 8 | int(body[off + 2]) << 16 | int(body[off + 3]) << 24


def model(read_word, body_bytes: int, bsz: int, checksum: bool, max_blocks: int):
    """-> (recOff[0 .. max_blocks] as int64, end, nBlocks, status).  read_word(off): the LE32 at off; it is asked only where
    body_bytes - off >= 4."""
    off, i, listed = 0, 0, []
    while True:
        end = off
        if off == body_bytes:
            status = END_OF_BYTES; break
        if body_bytes - off < 4:
            status = TRUNCATED_WORD; break
        word = read_word(off)
        if word == 0:
            status = END_MARK; end = off + 4; break
        if i == max_blocks:
            status = FULL; break
        size = word & 0x7FFFFFFF
        if size > bsz:
            status = SIZE_OVERFLOW; break
        need = 4 + size + (4 if checksum else 0)
        if need > body_bytes - off:
            status = TRUNCATED_BLOCK; break
        listed.append(off)
        off += need; i += 1
    rec_off = np.array(listed + [off] * (max_blocks + 1 - i), dtype=np.int64)
    return rec_off, end, i, status


def le32(v: int) -> np.ndarray:
    return np.frombuffer(np.uint32(v).tobytes(), dtype=np.uint8)


def build_body(sizes, stored, checksum: bool, end_mark: bool, trailing: int = 0, seed: int = 1):
    """A well-formed block section: record k = [LE32 sizes[k] | bit 31 if stored[k]][sizes[k] payload bytes][4 checksum bytes?],
    then an end mark and `trailing` bytes behind it if asked for.  Payload, checksum and trailing bytes are 0x01..0xFF noise: a walk
    that took one of them for a size word would stop with the wrong answer.  -> (body, the records' offsets + the section's end)"""
    rng = np.random.default_rng(seed)
    parts, off, pos = [], [], 0
    for n, st in zip(sizes, stored):
        off.append(pos)
        parts.append(le32(int(n) | (0x80000000 if st else 0)))
        parts.append(rng.integers(1, 256, size=int(n) + (4 if checksum else 0), dtype=np.uint8))
        pos += 4 + int(n) + (4 if checksum else 0)
    off.append(pos)
    if end_mark:
        parts.append(le32(0))
        parts.append(rng.integers(1, 256, size=trailing, dtype=np.uint8))
    body = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
    return np.ascontiguousarray(body), np.array(off, dtype=np.int64)


def record_sizes(n: int, bsz: int, seed: int):
    """n records: mostly short, a few of exactly bsz, stored ones among them, a stored record of size 0 (the word 0x80000000) when
    there are two or more, and a short last record"""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(1, 200, size=n)
    stored = rng.integers(0, 4, size=n) == 0
    if n:
        sizes[rng.integers(0, n, size=max(1, n // 16))] = bsz
        sizes[n - 1] = 3
    if n >= 2:
        k = int(rng.integers(0, n - 1))
        sizes[k] = 0; stored[k] = True
    return [int(x) for x in sizes], [bool(x) for x in stored]


def max_blocks_of(n: int):
    """0, n - 1 (the index is full), n, n + 1, n + 70 (padding over more than one store group)"""
    return sorted({0, max(n - 1, 0), n, n + 1, n + 70})


def hostile(bsz: int, checksum: bool):
    """[(name, body, bodyBytes)]: bodies of 0..3 bytes, a body cut at each of its last 12 byte positions, and the size words
    0x7FFFFFFF, 0xFFFFFFFF and bsz + 1 (with and without the stored bit) as the first, a middle and the last record's word"""
    out = []
    for k in range(4):
        out.append(("bytes%d" % k, np.full(k, 0x41, dtype=np.uint8), k))
        out.append(("zeros%d" % k, np.zeros(k, dtype=np.uint8), k))
    sizes, stored = record_sizes(5, bsz, 77)
    sizes[4] = 9                                          # the cut passes through payload, checksum, the size word and a record's end
    for end_mark in (False, True):
        body, off = build_body(sizes, stored, checksum, end_mark, 0, seed=5)
        for cut in range(1, 13):
            out.append(("cut%d%s" % (cut, "m" if end_mark else ""), body, body.size - cut))
    body, off = build_body(sizes, stored, checksum, True, 4, seed=6)
    for word in (0x7FFFFFFF, 0xFFFFFFFF, bsz + 1, 0x80000000 | (bsz + 1), 0):        # (0: an end mark in front of records)
        for k in (0, 2, 4):
            b = body.copy()
            b[off[k]:off[k] + 4] = le32(word)
            out.append(("word%08x@%d" % (word, k), b, b.size))
    return out
