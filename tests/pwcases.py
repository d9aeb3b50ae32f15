"""Crafted level-1 inputs for the parser's candidate windows (tests/test_parse_window.py, tests/test_gpu_parse_window.py): text in
which a phrase recurs with a chosen total match length, the recurrence starting at a chosen lane of a 64-position batch.

A site is   [guard 4][A 8][B 8][A again][u1][phrase, L bytes][d][B again][u2][phrase again at X][e] ...   (all bytes drawn at random)
The parser stops probing every position once a search has missed 64 times, so a short match in front of each copy of the phrase
starts the search anew: "A again" is found as a match of 8 bytes that ends at u1, so the first copy of the phrase is probed and
entered into the table; "B again" likewise ends at u2, so X is probed, and the match found there is exactly L bytes (LZ4's minimum
match of 4 plus L - 4 forward bytes; d and e differ from what follows the other copy).  The table has 4096 slots: the site is
drawn again until no position between a first copy and its second one hashes to the second one's slot."""
from __future__ import annotations

import numpy as np

from plz4_amd import synth

LENGTHS = tuple(range(19, 42)) + (51, 52, 53)          # total match lengths: forward lengths 15..37 and 47..49
LANES = (0, 27, 43, 63)
STRIDE = 1024                                          # bytes of text per site


def hash5(buf: np.ndarray, pos) -> np.ndarray:
    """LZ4_hash5 (12 bits) of the positions `pos` of `buf`."""
    pos = np.atleast_1d(np.asarray(pos, dtype=np.int64))
    v = np.zeros(pos.size, dtype=np.uint64)
    for k in range(5):
        v |= buf[pos + k].astype(np.uint64) << np.uint64(8 * k)
    with np.errstate(over="ignore"):
        return ((v << np.uint64(24)) * np.uint64(889523592379)) >> np.uint64(52)


def _plant(buf, rng, x, length):
    """The second copy at x, the first copy and what surrounds them (see the module's text)."""
    s = x - 10 - 1 - length                                    # first copy
    g = s - 29                                                 # guard
    hi = min(buf.size, x + length + 8)
    for _ in range(256):
        buf[g:hi] = rng.integers(0, 256, size=hi - g, dtype=np.uint8)
        a, b, a2, u1, d, b2, u2 = g + 4, g + 12, g + 20, g + 28, s + length, s + length + 1, x - 1
        buf[a2:a2 + 8] = buf[a:a + 8]
        buf[u1] = buf[b] ^ 0x33                                # the match at a2 ends after 8 bytes
        buf[b2:b2 + 8] = buf[b:b + 8]
        buf[u2] = buf[a2] ^ 0x33                               # the match at b2 ends after 8 bytes
        buf[x:x + length] = buf[s:s + length]
        if x + length < buf.size:
            buf[d] = buf[x + length] ^ 0x55                    # both copies end after `length` bytes
        ok = True
        for src, dst in ((a, a2), (b, b2), (s, x)):
            ok = ok and not np.any(hash5(buf, np.arange(src + 1, dst)) == hash5(buf, dst)[0])
        if ok:
            return
    raise AssertionError("no site without a collision")


def block_for_length(length: int, seed: int = 0):
    """Text with one site per lane of LANES plus the lane at which the match ends exactly at a batch boundary.
    Returns (block, [positions of the second copies])."""
    lanes = LANES + ((-length) % 64,)
    n = 65536 + 2048 + STRIDE * len(lanes) + 4096
    buf = synth.text(n, seed=1000 + length + 97 * seed).copy()
    rng = np.random.Generator(np.random.PCG64(length * 131 + seed))
    sites = []
    for i, lane in enumerate(lanes):
        x = ((65536 + 2048 + STRIDE * i + 512) & ~63) + lane
        _plant(buf, rng, x, length)
        sites.append(x)
    return np.ascontiguousarray(buf), sites


def block_to_match_limit(length: int, seed: int = 0):
    """Text whose last match is found `length` bytes in front of matchLimit (n - 5) and runs on to the block's end: the parser
    must stop it at matchLimit (the generic batches of a block's last 224 bytes)."""
    n = 65536 + 4096 + 11 + length
    buf = synth.text(n, seed=2000 + length + 97 * seed).copy()
    rng = np.random.Generator(np.random.PCG64(length * 733 + seed))
    x = n - 5 - length
    _plant(buf, rng, x, length + 5)                            # (the copies are equal up to the block's last byte)
    return np.ascontiguousarray(buf[:n]), x
