"""Crafted level-1 inputs for the grid batch's scalar hop (tests/test_parse_hops.py, tests/test_gpu_parse_hops.py): blocks in which
chosen 64-position batches hold a chosen number of executed matches at chosen lanes, in bytes that have no other match near them.

The ground is random bytes with a keep-alive every 40 bytes -- 8 bytes, 8 others, the first 8 again: a match of 8 -- because the
parser stops probing every position once a search has missed 64 times, and a batch is a grid batch only while it does.  So the
ground has one or two matches per batch and nothing else, and the counters of a block say what its sites did.

A site for the batch at X (a multiple of 64) is
    [keep-alive][source, first half][keep-alive][source, second half][keep-alive][random, < 40][copies, from X + lane0][random up to X + 64 ...]
The copies are `units`: unit k is some bytes of the source, followed by a byte that differs from what follows them there, so the
match found at its first byte is exactly as long as the unit.  The copies stand in the reverse of the sources' order and all units
start with different bytes, so neighbouring copies do not continue each other.  A unit has at least 5 bytes: LZ4 hashes five
bytes, and with this hash two positions whose first four bytes are equal and whose fifth differ never share a slot (the fifth
byte, times the multiplier's odd low byte, lands in the product's top eight bits, which are part of the slot number) -- so the
parser never finds a match of exactly four bytes, and a batch holds at most 13 executed matches (lanes 0, 5, ... 60), not 16."""
from __future__ import annotations

import numpy as np

from pwcases import hash5

PERIOD = 40            # of the ground's keep-alives
HALF = 40              # bytes of source between two keep-alives
N_BLOCK = 128 << 10
SITE_STRIDE = 4096
FIRST_SITE = 66 << 10  # (beyond 64 KiB: liblz4's byU32 tables, the grid batches)


def _ka(rng) -> np.ndarray:
    x = rng.integers(0, 256, size=24, dtype=np.uint8)
    x[16:24] = x[0:8]
    x[8] = x[0] ^ 0x5A                                     # (not a run)
    return x


def ground(n: int, seed: int) -> np.ndarray:
    rng = np.random.Generator(np.random.PCG64(seed))
    buf = rng.integers(0, 256, size=n, dtype=np.uint8)
    at = np.arange(64, n - 64, PERIOD)
    ka = rng.integers(0, 256, size=(at.size, 24), dtype=np.uint8)
    ka[:, 16:24] = ka[:, 0:8]
    ka[:, 8] = ka[:, 0] ^ 0x5A                             # (not a run)
    buf[at[:, None] + np.arange(24)] = ka
    return buf


def _found(buf, sp, p) -> bool:
    """The table still holds sp when p is probed: no position in between hashes to the same slot."""
    return not np.any(hash5(buf, np.arange(sp + 1, p)) == hash5(buf, p)[0])


def _units(rng, lengths):
    """One unit of random bytes per length, all with different first bytes."""
    firsts = rng.permutation(256)[:len(lengths)]
    units = []
    for ln, f in zip(lengths, firsts):
        assert ln >= 5
        u = rng.integers(0, 256, size=ln, dtype=np.uint8)
        u[0] = f
        units.append(u)
    return units


def _place(buf, rng, x, lane0, halves, copy):
    """Writes a site for the batch at x; returns the position of the first source half."""
    assert len(halves) == 2 and all(h.size <= HALF for h in halves)
    at = x + lane0
    lead = 24 + halves[0].size + 24 + halves[1].size + 24
    s = 64 + (at - lead - 64) // PERIOD * PERIOD              # in step with the ground's keep-alives
    pad = at - (s + lead)
    assert 0 <= pad < PERIOD
    end = max(x + 64, at + copy.size) + 8
    buf[s:end] = rng.integers(0, 256, size=end - s, dtype=np.uint8)
    p = s
    for h in halves:
        buf[p:p + 24] = _ka(rng); p += 24
        buf[p:p + h.size] = h; p += h.size
    buf[p:p + 24] = _ka(rng)
    buf[at:at + copy.size] = copy
    for q in range(64 + (end - 64 + PERIOD - 1) // PERIOD * PERIOD, end + 2 * PERIOD, PERIOD):
        buf[q:q + 24] = _ka(rng)                               # (the ground's keep-alives that the site's end may have cut)
    return s + 24


def site_units(buf, rng, x, lane0, lengths):
    """A batch at x with one executed match per unit, the first at lane0.  Returns [(position, match length)]."""
    for _ in range(64):
        units = _units(rng, lengths)
        halves, cur = [], []
        for u in reversed(units):                              # sources in the reverse of the copies' order
            if sum(c.size for c in cur) + u.size > HALF:
                halves.append(cur); cur = []
            cur.append(u)
        halves.append(cur)
        while len(halves) < 2:
            halves.append([])
        assert len(halves) == 2, "the units do not fit two halves"
        halves = [np.concatenate(h + [rng.integers(0, 256, size=HALF - sum(c.size for c in h), dtype=np.uint8)]) for h in halves]
        _place(buf, rng, x, lane0, halves, np.concatenate(units))
        # every match ends where its unit ends: the byte behind the copy differs from the byte behind the source's same bytes
        out, p, ok = [], x + lane0, True
        whole = buf[x - 512:x + lane0].tobytes()
        for u in units:
            sp = whole.rfind(u.tobytes())
            sp = sp + x - 512 if sp >= 0 else sp
            ok = ok and sp >= 0 and buf[sp + u.size] != buf[p + u.size] and _found(buf, sp, p)
            out.append((p, int(u.size))); p += u.size
        if ok:
            return out
    raise AssertionError("no site")


def site_wrap(buf, rng, x, cover):
    """The batch at x starts inside a match from the batch before that covers its lanes 0 .. cover-1 (every one of them a hit, since
    the match's source was probed position by position), and has no hit from there on.  Returns [(position, match length)]."""
    for _ in range(64):
        a = rng.integers(0, 256, size=28, dtype=np.uint8)
        b = rng.integers(0, 256, size=28, dtype=np.uint8)
        copy = np.zeros(80, dtype=np.uint8)                    # (filled once the keep-alive between the halves is known)
        src0 = _place(buf, rng, x, cover - 80, [a, b], copy)
        buf[x + cover - 80:x + cover] = buf[src0:src0 + 80]
        if buf[x + cover] != buf[src0 + 80] and _found(buf, src0, x + cover - 80):
            return [(x + cover - 80, 80)]
    raise AssertionError("no site")


# name -> (lane of the first unit, the units' match lengths); N = 8 unconditional hops
CASES = {
    "first_at_lane0": (0, [5, 6, 5, 7, 5]),
    "exactly_8":      (3, [5, 5, 6, 5, 5, 7, 5, 5]),
    "exactly_9":      (3, [5, 5, 6, 5, 5, 7, 5, 5, 5]),
    "thirteen":       (0, [5] * 13),                       # the most a batch can hold: two turns of the loop behind the question
    "nine_then_x36":  (0, [5] * 9 + [28]),                 # the lane that fills its 20-byte window is the 10th match: found behind the question
    "x36_then_nine":  (0, [20] + [5] * 9),                 # ... is the first match: both halves of the question known at once
}
WRAP_COVER = 40
SITES = 4


def block(name: str, seed: int = 0):
    """One block of N_BLOCK bytes with SITES sites of the case.  Returns (block, [[(position, match length)] per site], [x per site])."""
    buf = ground(N_BLOCK, 7000 + seed)
    rng = np.random.Generator(np.random.PCG64([seed, sum(name.encode())]))
    exp, xs = [], []
    for i in range(SITES):
        x = FIRST_SITE + SITE_STRIDE * i
        if name == "wrap":
            exp.append(site_wrap(buf, rng, x, WRAP_COVER))
        else:
            lane0, lengths = CASES[name]
            exp.append(site_units(buf, rng, x, lane0, lengths))
        xs.append(x)
    return np.ascontiguousarray(buf), exp, xs


NAMES = ("wrap",) + tuple(CASES)
