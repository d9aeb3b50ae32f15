"""Inputs for the encoders' capacity verdict (tests/test_encode_capacity.py on the lane emulation, tests/test_gpu_encode_capacity.py
on the kernels): blocks built from sequence specs whose run and match lengths sit on the edges of the length encoding and of liblz4's
end-of-block rules, so that the compressed size lands on every residue an encoder's "does the block fit dstCap" arithmetic can get
wrong; blocks spliced from a dictionary for the routes with history outside the block; and blocks tuned to a given compressed size
for the stored/compressed flip of a record.  Test infrastructure."""
import numpy as np

import corpus
from plz4_amd import synth

# run and match lengths: the token's nibble (15 / 19), the first and second length byte (270 / 274, 525 / 529), liblz4's
# MFLIMIT / LASTLITERALS / MINMATCH (12, 5, 4) and their neighbours
EDGE_LENS = (0, 1, 4, 5, 11, 12, 13, 14, 15, 16, 18, 19, 20, 254, 255, 256, 269, 270, 271, 273, 274, 524, 525, 529, 530)
TAILS = (0, 1, 4, 5, 6, 11, 12, 13)
WIDTH = 8                                                   # capacities swept: [full - WIDTH, full + WIDTH)


def bound(n):
    return n + n // 255 + 16


def _len(rng):
    return int(EDGE_LENS[int(rng.integers(0, len(EDGE_LENS)))]) if rng.random() < 0.8 else int(rng.integers(0, 600))


def spec_block(rng):
    """1..7 times a literal run of random bytes and a copy of `ml` bytes from `off` back (overlapping like a decoder's), then a
    tail of literals."""
    out = bytearray()
    for _ in range(int(rng.integers(1, 8))):
        ll = _len(rng)
        if not out:
            ll = max(ll, 1)
        out += rng.integers(0, 256, size=ll, dtype=np.uint8).tobytes()
        ml = _len(rng)
        pick = int(rng.integers(0, 4))
        off = (1, 2, len(out), int(rng.integers(1, len(out) + 1)))[pick]
        off = min(off, len(out), 65535)
        for _ in range(ml):
            out.append(out[-off])
    out += rng.integers(0, 256, size=TAILS[int(rng.integers(0, len(TAILS)))], dtype=np.uint8).tobytes()
    return np.frombuffer(bytes(out), dtype=np.uint8).copy()


def spec_blocks(count, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return [spec_block(rng) for _ in range(count)]


def corpus_blocks():
    """A few of the shared corpus with 13 <= n <= 20000."""
    out = [np.ascontiguousarray(corpus.structured(n, seed)) for n, seed in ((13, 1), (300, 2), (4097, 3), (20000, 4))]
    for n in (13, 39, 65, 271, 4096):                       # the T and S members of corpus.small_cases() at these sizes
        out += [np.ascontiguousarray(synth.text(n, seed=n + 1)[:n]), np.ascontiguousarray(corpus.structured(n, seed=n + 3)[:n])]
    return out


def big_blocks():
    """65 536, 65 547 (liblz4's byU32 tables begin, and with them the few-block level-1 path) and about 70 000 bytes."""
    return [np.ascontiguousarray(corpus.structured(n, seed)) for n, seed in ((65536, 11), (65547, 12), (70001, 13))]


# ---- blocks with history outside them
HIST_SIZES = (13, 100, 4095, 4096, 4097, 9000, 70000)
_T = synth.text(70000 + 90000, seed=177)
DICT_USER = np.ascontiguousarray(_T[:70000])                # the user's dictionary; its last 64 KiB are kept
DICT64 = np.ascontiguousarray(DICT_USER[-65536:])
DICT1000 = np.ascontiguousarray(DICT_USER[-1000:])


def hist_block(n, seed, dct):
    """`n` bytes spliced from text of the dictionary's vocabulary, pieces of `dct`, noise and repeats of the block's own bytes,
    the piece lengths from EDGE_LENS."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = bytearray()
    t_at = 0
    while len(out) < n:
        kind = int(rng.integers(0, 4))
        ln = max(_len(rng), 1)
        if kind == 0:
            out += rng.integers(0, 256, size=min(ln, 40), dtype=np.uint8).tobytes()
        elif kind == 1 and dct.size > ln:
            o = int(rng.integers(0, dct.size - ln))
            out += dct[o:o + ln].tobytes()
        elif kind == 2 and len(out) >= 8:
            off = int(rng.integers(1, min(len(out), 65535) + 1))
            for _ in range(ln):
                out.append(out[-off])
        else:
            out += _T[70000 + t_at:70000 + t_at + ln].tobytes(); t_at = (t_at + ln) % 80000
    return np.frombuffer(bytes(out[:n]), dtype=np.uint8).copy()


def hist_blocks(dct):
    return [hist_block(n, 1000 + n, dct) for n in HIST_SIZES]


# ---- a block of a given compressed size
def tight_block(size_fn, n, target, seed=0):
    """`n` random bytes with src[0:L] copied to a later place that does not overlap it and, where that one knob steps over the
    target, a second short repeat elsewhere, searched until size_fn(block) == target.  Both repeats lie in the block's first 4 KiB,
    where level 1's table still holds their sources.  Raises if no such block is found: a caller never goes without a size."""
    rng = np.random.Generator(np.random.PCG64(0x7161 + seed))
    base = rng.integers(0, 256, size=n, dtype=np.uint8)
    at1 = 1024                                              # the first repeat: src[0:L] -> src[at1:at1 + L], L < 1024
    src2, at2 = 2048, 3072                                  # the second: src[src2:src2 + M] -> src[at2:at2 + M]
    assert n >= 4096

    def build(L, M):
        b = base.copy()
        b[at1:at1 + L] = b[0:L]
        if M:
            b[at2:at2 + M] = b[src2:src2 + M]
        return b

    # a repeat of L bytes saves a little less than L bytes: start just below the saving wanted
    size0 = size_fn(build(0, 0))
    guess = size0 - target
    assert 0 <= guess < 900, (n, target, size0)
    for M in (0,) + tuple(range(4, 24)):                    # (one knob first: most sizes need no second repeat)
        for L in range(max(guess - M - 2, 0), guess + 24):
            b = build(L, M)
            if size_fn(b) == target:
                return b
    raise AssertionError("tight_block: no block of %d bytes compresses to %d (from %d)" % (n, target, size0))
