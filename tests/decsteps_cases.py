"""Blocks for the near steps of the decoder's LDS-staged batch (wave_decode_lds_batch, plz4_amd/csrc/lz4_device.inl): near matches
are copied one by one in sequence order, a cooperative copy cuts them into runs.  The blocks follow the HEAD / SITE / TAIL scheme
of tests/decflow_cases.py (the site starts a vector batch of its own; HEAD and TAIL hold no near match and no cooperative copy, so
the step counters belong to the site).  A sequence is (literals, match length, offset).  Test infrastructure only."""
import numpy as np

from decflow_cases import C, F, FAR, K, _close, _put

OWN = (6, 4, 6)            # copies the first four of its own sequence's literals: near wherever it stands, depends on nobody
LIT3 = (1, 4, 4)           # its own literal and the three bytes before it: near wherever it stands, a chain through all of them

# name -> (site, simple near matches in it = steps that copy a match, cooperative copies in it)
CASES = {}
for _n in range(2, 17):
    CASES["chain_%d" % _n] = ([C] * _n, _n - 1, 0)             # (the first C's source ends where the batch begins: far)
CASES.update({
    "own_6":            ([OWN] * 6, 6, 0),
    "own_12":           ([OWN] * 12, 12, 0),                    # (108 input bytes: two batches)
    "reads_far_4":      ([(2, 6, FAR), (0, 4, 6)], 1, 0),       # the first four bytes a far match of the same batch has just put
    "reads_far_18":     ([(0, 18, FAR), (0, 18, 18)], 1, 0),    # ... all eighteen of them
    "tail_first":       ([(3, 6, 8)], 1, 0),                    # source: five bytes of the staged tail and one of the batch, as the first member
    "tail_first_coop":  ([(3, 8, 6)], 0, 1),                    # the same with offset < length: a cooperative copy, no step
    "lengths":          ([(2, 4, 4), (2, 4, 5), (2, 5, 5), (2, 5, 6), (2, 17, 17), (2, 17, 18), (2, 18, 18), (2, 18, 19)], 8, 0),
    "coop_neighbours":  ([C, C, K, (0, 4, 4)], 2, 1),           # K repeats the end of the step before it; the step behind reads K's end
    "coop_between":     ([K, (1, 4, 5), K], 1, 2),
    "fill_16":          ([LIT3] * 16, 16, 0),                   # 64 input bytes: the window holds nothing else
    "none":             ([], 0, 0),
})
NAMES = tuple(CASES)
SEEDS_GPU = 10
N_RANDOM = 300


def block(name, seed=0):
    """(compressed bytes, plaintext) of the named case."""
    rng = np.random.default_rng(7000 + 1000 * seed + NAMES.index(name))
    comp, plain = bytearray(), bytearray()
    _put(comp, plain, rng, 3000, 8, 1000)
    for s in CASES[name][0]:
        _put(comp, plain, rng, *s)
    for _ in range(220):
        _put(comp, plain, rng, *F)
    _close(comp, plain, rng)
    return np.frombuffer(bytes(comp), dtype=np.uint8).copy(), np.frombuffer(bytes(plain), dtype=np.uint8).copy()


def random_block(i):
    """Random block i: between HEAD and TAIL, 20..400 sequences of 0..8 literals and a match of 4..18 bytes (one in twelve: 19..48,
    a cooperative copy) whose offset is drawn from [length, 48], so that most matches are near."""
    rng = np.random.default_rng(90000 + i)
    comp, plain = bytearray(), bytearray()
    _put(comp, plain, rng, 3000, 8, 1000)
    for _ in range(int(rng.integers(20, 401))):
        ml = int(rng.integers(19, 49)) if rng.integers(0, 12) == 0 else int(rng.integers(4, 19))
        off = int(rng.integers(ml, 49))
        _put(comp, plain, rng, int(rng.integers(0, 9)), ml, off)
    for _ in range(220):
        _put(comp, plain, rng, *F)
    _close(comp, plain, rng)
    return np.frombuffer(bytes(comp), dtype=np.uint8).copy(), np.frombuffer(bytes(plain), dtype=np.uint8).copy()
