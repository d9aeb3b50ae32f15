"""The cases of the wave-wide HC parser for blocks of at most 4 KiB under a dictionary context (plz4_amd/csrc/lz4hcx_device.inl),
shared by tests/test_hcx_encode.py (lane emulation) and tests/test_gpu_hcx_encode.py (the kernels): the smallest shapes at which
that code can go wrong.  A case is (name, dictionary as the user gives it, block, levels or None for every level, capacities or
None for the default three).  Test infrastructure."""
from collections import namedtuple

import numpy as np

import corpus
from plz4_amd import synth

Case = namedtuple("Case", "name dct block levels caps")

ALL_LEVELS = tuple(range(2, 13))
# the levels the wave-wide parser is built for (kHcxMinLevel .. kHcxMaxLevel of lz4hcx_device.inl): every HC level
HCX_LEVELS = tuple(range(2, 13))
SIZES = (0, 1, 4, 5, 12, 13, 64, 65, 1000, 4095, 4096)
DICT_LENS = (0, 3, 4, 8, 9, 30000, 70000)                   # 70000: the last 64 KiB are taken
FUZZ_SEED = 0x48435831
FUZZ_BLOCKS = 150

_T = synth.text(70000 + 3 * 4096 + 5000, seed=77)           # dictionary and blocks out of one generator: shared vocabulary
TEXT_DICT = np.ascontiguousarray(_T[:70000])
_TEXT_BLOCKS = _T[70000:]


def dict64(dct):
    """What plz4 keeps of a user dictionary (compress/dict.go:43-56)."""
    return np.ascontiguousarray(dct[-65536:] if dct.size > 65536 else dct)


def bound(n):
    return n + n // 255 + 16


def default_caps(n):
    return [bound(n), n, n // 3]


def sequences(comp):
    """The (position, match length, offset) of every sequence of an LZ4 block."""
    b = bytes(comp)
    i, pos, out = 0, 0, []
    while i < len(b):
        tok = b[i]; i += 1
        ll = tok >> 4
        if ll == 15:
            while True:
                v = b[i]; i += 1; ll += v
                if v != 255: break
        i += ll; pos += ll
        if i >= len(b): break
        off = b[i] | (b[i + 1] << 8); i += 2
        ml = (tok & 15) + 4
        if (tok & 15) == 15:
            while True:
                v = b[i]; i += 1; ml += v
                if v != 255: break
        out.append((pos, ml, off))
        pos += ml
    return out


def text_block(n, k=0):
    return np.ascontiguousarray(_TEXT_BLOCKS[k * 4096:k * 4096 + n])


def static_cases():
    out = []
    for n in SIZES:                                         # every size under the full dictionary ...
        out.append(Case(f"text-{n}", TEXT_DICT, text_block(n), None, None))
    for dl in DICT_LENS:                                    # ... and every dictionary length under two sizes
        for n in (65, 4096):
            out.append(Case(f"dict{dl}-text-{n}", np.ascontiguousarray(TEXT_DICT[:dl]), text_block(n, 1), None, None))
    d = dict64(TEXT_DICT)
    # the distance boundary: a candidate at the block's own phase is 65536 away (out of range) / 65535 away (in range)
    out.append(Case("dist-65536", TEXT_DICT, np.ascontiguousarray(d[0:4096]), None, None))
    out.append(Case("dist-65535", TEXT_DICT, np.ascontiguousarray(d[1:4097]), None, None))
    # matches that run into the dictionary's end and stop there
    out.append(Case("dict-end", TEXT_DICT, np.ascontiguousarray(np.concatenate([d[-300:], text_block(3000, 2)])), None, None))
    # ... and behind them zeros, which is what the emulation harness keeps behind its copy of the dictionary: a count that does not
    # stop at the dictionary's end goes on there
    out.append(Case("dict-end-zeros", TEXT_DICT, np.ascontiguousarray(np.concatenate([d[-300:], np.zeros(200, np.uint8), text_block(1000, 2)])), None, None))
    # pattern analysis in the own chain, then the dictionary
    pat = np.tile(np.frombuffer(b"abcabcab", np.uint8), 9000)
    for n in (65, 1000, 4096):
        out.append(Case(f"periodic-{n}", np.ascontiguousarray(pat[:50001]), np.ascontiguousarray(pat[50001:50001 + n]), (9, 10, 12), None))
    out.append(Case("periodic-text-dict", TEXT_DICT, np.ascontiguousarray(pat[3:3 + 4096]), (9, 10, 12), None))
    out.append(Case("zeros", np.zeros(5000, np.uint8), np.zeros(4096, np.uint8), None, None))
    out.append(Case("structured", corpus.structured(30000, 3), np.ascontiguousarray(corpus.structured(100000, 3)[50000:54096]), None, None))
    out.append(Case("structured-1000", corpus.structured(30000, 3), np.ascontiguousarray(corpus.structured(100000, 3)[70000:71000]), None, None))
    for n in (100, 4096):                                   # incompressible: a stored record, result 0 at n // 3
        out.append(Case(f"noise-{n}", TEXT_DICT, synth.random_bytes(n, seed=5 + n), None, None))
    return out


# ---- the attempts budget: how deep the dictionary's chain is read depends on how many attempts the own walk took
_PHRASE = np.frombuffer(b"Qz7#kW2@pL9!xV4$", np.uint8)       # 16 bytes, no 4-byte window repeats inside
BUDGET_LEVELS = (3, 4, 5)                                   # 4, 8, 16 attempts


def _noise(rng, n):
    return rng.integers(128, 254, size=n, dtype=np.uint8)   # (never the phrase's bytes, nor the two bytes in front of the dictionary's phrases)


def budget_case(level, k):
    """k copies of the phrase in front of the searched position, each followed by noise, the oldest one by 2 bytes of the
    continuation first; the dictionary holds the phrase with 4 bytes of the continuation at depth 1 of its chain and with 6 at
    depth 2.  The searched position lies 27 bytes before the block's end: a match there is at most 22 long, and one of 16 or more
    is not followed by a second search (it ends behind mflimit, lz4hc.c:1167), so the sequence at that position is the first
    search's answer.  Returns (case, searched position)."""
    rng = np.random.Generator(np.random.PCG64(1000 * level + k))
    cont = rng.integers(48, 90, size=6, dtype=np.uint8)
    dct = np.concatenate([_noise(rng, 500), [np.uint8(254)], _PHRASE, cont, _noise(rng, 300), [np.uint8(255)], _PHRASE, cont[:4], _noise(rng, 200)]).astype(np.uint8)
    parts = [_noise(rng, 19), np.array([199], np.uint8)]    # (the byte in front of every phrase is its own: no match starts there)
    for j in range(k):
        parts += [_PHRASE, cont[:2] if j == 0 else cont[:0], _noise(rng, 7), np.array([200 + j], np.uint8)]
    at = sum(p.size for p in parts)
    parts += [_PHRASE, cont, _noise(rng, 5)]
    return Case(f"budget-l{level}-k{k}", np.ascontiguousarray(dct), np.ascontiguousarray(np.concatenate(parts)), (level,), None), at


def budget_cases(ref):
    """The family for levels 3, 4, 5 with k = attempts - 1, attempts, attempts + 1; the real liblz4's answers at the searched
    position must be the three different ones the family is for, else it has degenerated."""
    out = []
    for level in BUDGET_LEVELS:
        a = 1 << (level - 1)
        got = []
        for k in (a - 1, a, a + 1):
            case, at = budget_case(level, k)
            keep, daddr = ref.new_dict_ctx_hc(dict64(case.dct), level)
            r, comp = ref.stream_ctx_hc(level, daddr)(case.block, bound(case.block.size))
            seq = [s for s in sequences(comp[:r]) if s[0] == at]
            assert len(seq) == 1, (level, k, "no sequence starts at the searched position")
            got.append((seq[0][1], seq[0][2] > at))
            out.append(case)
        # one attempt left: the dictionary's nearest, not the one behind it (16 + 4); none left, the oldest copy reached (16 + 2);
        # not reached (16)
        assert got == [(20, True), (18, False), (16, False)], (level, got)
    return out


def fuzz_cases():
    """Blocks of 0..4096 bytes spliced from pieces of the dictionary, repeats of the block's own bytes and noise."""
    rng = np.random.Generator(np.random.PCG64(FUZZ_SEED))
    d = dict64(TEXT_DICT)
    out = []
    for i in range(FUZZ_BLOCKS):
        n = int(rng.integers(0, 4097)) if i >= 4 else (0, 4096, 13, 12)[i]
        buf = np.empty(n + 600, np.uint8)                   # (the block being spliced: the last piece may run past n.  No encoder
                                                            # writes here -- HcxEmu.compress has its own guarded destination)
        at = 0
        while at < n:
            kind = int(rng.integers(0, 4))
            ln = int(rng.integers(1, 200 if kind else 24))
            if kind == 0:
                piece = rng.integers(0, 256, size=ln, dtype=np.uint8)
            elif kind == 1 or at < 8:
                o = int(rng.integers(0, d.size - ln))
                piece = d[o:o + ln]
            elif kind == 2:
                o = int(rng.integers(0, at))
                piece = buf[o:o + min(ln, at - o)].copy()
            else:
                per = int(rng.integers(1, 9))
                piece = np.resize(buf[at - per:at].copy(), ln)
            buf[at:at + piece.size] = piece
            at += piece.size
        out.append(Case(f"fuzz-{i}", TEXT_DICT, np.ascontiguousarray(buf[:n]), None, [bound(n), n // 2] if i % 3 == 0 else [bound(n)]))
    return out


def exact_cap_cases(ref):
    """Three text cases at their exact compressed size and one byte around it, per level."""
    out = []
    for n in (65, 1000, 4096):
        for level in ALL_LEVELS:
            blk = text_block(n, 2)
            keep, daddr = ref.new_dict_ctx_hc(dict64(TEXT_DICT), level)
            r, _ = ref.stream_ctx_hc(level, daddr)(blk, bound(n))
            assert r > 0
            out.append(Case(f"exact-{n}-l{level}", TEXT_DICT, blk, (level,), [r - 1, r, r + 1]))
    return out


def all_cases(ref):
    return static_cases() + budget_cases(ref) + exact_cap_cases(ref) + fuzz_cases()


def levels_of(case, built=HCX_LEVELS):
    return [l for l in (case.levels or ALL_LEVELS) if l in built]


def caps_of(case):
    return case.caps if case.caps is not None else default_caps(case.block.size)
