"""Blocks for the control flow of the decoder's LDS-staged batch (wave_decode_lds_batch, plz4_amd/csrc/lz4_device.inl), built
sequence by sequence like tests/lz4blocks.py.  Every block is

    HEAD   a literal run of 3000 bytes and a match: a sequential step, so the next vector batch starts exactly at the site
    SITE   the sequences the case is about
    TAIL   220 sequences of 2 literals + a 6-byte match 2500 bytes back (far matches only), then 20 closing literals

so the site has well over 160 input bytes and 1088 bytes of output room behind it and the vector path takes it; the ground
(HEAD + TAIL) makes no near round and no cooperative copy, so those counters belong to the site.  A sequence is (literals,
match length, offset).  Test infrastructure only."""
import numpy as np

from lz4blocks import put_len

FAR = 2500
T = (0, 4, FAR)            # three input bytes: the shortest sequence
F = (2, 6, FAR)            # the ground's sequence
C = (1, 4, 5)              # copies the match of the sequence before it: a chain of these is one near round each
K = (0, 30, 3)             # long and overlapping: a cooperative copy

# name -> (site, what the counters of the ascending order must show).  Counter names: tests/test_decode_flow.py.
CASES = {
    "tokens_21":        ([T] * 21 + [(1, 4, FAR)], {"full": 0}),         # the 22nd token's offset lies beyond the window
    "tokens_22":        ([T] * 22, {"full": 1}),
    "tokens_23":        ([T] * 23, {"full": 1}),
    "rounds_0":         ([C], {"rounds": 0, "coop": 0}),
    "rounds_1":         ([C] * 2, {"rounds": 1, "coop": 0}),
    "rounds_2":         ([C] * 3, {"rounds": 2, "coop": 0}),
    "rounds_3":         ([C] * 4, {"rounds": 3, "coop": 0}),
    "rounds_6":         ([C] * 7, {"rounds": 6, "coop": 0}),
    "coop_first":       ([K], {"rounds": 0, "coop": 1, "coop_mem": 0}),
    "coop_middle":      ([C, C, K, C, C], {"rounds": 3, "coop": 1, "coop_mem": 0}),
    "coop_last":        ([C, C, K], {"rounds": 1, "coop": 1, "coop_mem": 0}),
    "coop_from_memory": ([(0, 40, FAR)], {"rounds": 0, "coop": 1, "coop_mem": 1}),
    # its source starts before the staged tail and runs into the batch: cut, then lane 0 of a batch without members
    "coop_old_source":  ([F, (0, 100, 50)], {"coop": 0, "no_members": 2}),
    "far_only":         ([], {"rounds": 0, "coop": 0, "no_members": 1, "primes": 2}),
    "after_long_match": ([(2, 300, FAR)], {"no_members": 2, "primes": 3}),
    "longlit_member":   ([F, (20, 4, FAR)], {"no_members": 1, "primes": 2}),
    "longlit_cut":      ([F, (215, 4, FAR)], {"no_members": 2, "primes": 3}),
    "out_cut_1024":     ([(0, 273, 1)] * 5, {"coop": 5}),
    "lane0_not_plain":  ([(14, 4, FAR)], {"no_members": 2, "primes": 3}),
}
# two more shapes of block
SPECIAL = ("start_below_32", "input_room_first")
NAMES = tuple(CASES) + SPECIAL
SEEDS_GPU = 19


def _put(comp, plain, rng, ll, ml, off):
    lits = rng.integers(0, 256, ll, dtype=np.uint8).tobytes()
    comp.append((min(ll, 15) << 4) | min(ml - 4, 15))
    if ll >= 15:
        put_len(comp, ll - 15)
    comp += lits
    comp += bytes([off & 0xFF, off >> 8])
    if ml - 4 >= 15:
        put_len(comp, ml - 4 - 15)
    plain += lits
    start = len(plain) - off
    assert start >= 0
    for i in range(ml):
        plain.append(plain[start + i])


def _close(comp, plain, rng, n=20):
    lits = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    comp.append(min(n, 15) << 4)
    if n >= 15:
        put_len(comp, n - 15)
    comp += lits; plain += lits


def damaged(name, comp):
    """A copy of the named case's block whose HEAD match has an offset beyond the start of the output (the decoders reject it)."""
    head = 10 * (1 + 12 + 2) if name == "start_below_32" else 0
    assert comp[head] == 0xF4 and comp[head + 1] == 255
    k = head + 1 + (3000 - 15) // 255 + 1 + 3000            # behind the token, the length bytes and the literals
    d = comp.copy()
    d[k] = 0xFF; d[k + 1] = 0xFF
    return d


def block(name, seed=0):
    """(compressed bytes, plaintext) of the named case."""
    rng = np.random.default_rng(1000 * seed + NAMES.index(name))
    comp, plain = bytearray(), bytearray()
    if name == "start_below_32":
        # the block's first vector batch, output position 0: every match copies its own sequence's literals (one near round)
        for _ in range(10):
            _put(comp, plain, rng, 12, 4, 12)
    _put(comp, plain, rng, 3000, 8, 1000)
    for s in CASES.get(name, ([], None))[0]:
        _put(comp, plain, rng, *s)
    for _ in range(220):
        _put(comp, plain, rng, *F)
    if name == "input_room_first":
        # two very long matches and a short end: the input's 160 bytes run out while 1088 bytes of output room are still there
        _put(comp, plain, rng, 0, 1000, FAR)
        _put(comp, plain, rng, 0, 1000, FAR)
    _close(comp, plain, rng)
    return np.frombuffer(bytes(comp), dtype=np.uint8).copy(), np.frombuffer(bytes(plain), dtype=np.uint8).copy()
