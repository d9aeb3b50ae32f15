"""LZ4 blocks built sequence by sequence (not by a compressor), with literal and match lengths and offsets drawn around every
boundary the decoder's vector path cares about: 13/14/15 literals, extension bytes 254/255, 18/19/273/274 match bytes, offsets
below the match length, sequences straddling the 64-byte window.  Shared by tests/fuzz/fuzz_decode.py and the GPU bounds tests;
tests/emu/decode_bounds_main.cpp carries the same generator in C++.  Test infrastructure only."""
import numpy as np

LL = [0, 0, 1, 2, 3, 5, 7, 12, 13, 14, 15, 16, 17, 30, 45, 47, 48, 49, 62, 63, 64, 100, 254 + 15, 255 + 15, 300, 600]
ML = [4, 4, 5, 6, 8, 12, 17, 18, 19, 20, 33, 64, 100, 272, 273, 274, 275, 528, 529, 1000]


def put_len(out, v):
    while v >= 255:
        out.append(255); v -= 255
    out.append(v)


def make_block(rng, nseq):
    """Returns (compressed bytes, plaintext) of a valid block that ends the way liblz4 requires (last 5 bytes literals,
    last match starts >= 12 bytes before the end)."""
    comp = bytearray(); plain = bytearray()
    for _ in range(nseq):
        ll = int(rng.choice(LL)) if rng.random() < 0.7 else int(rng.integers(0, 40))
        ml = int(rng.choice(ML)) if rng.random() < 0.6 else int(rng.integers(4, 40))
        if not plain and ll == 0:
            ll = 1
        lits = rng.integers(0, 256, ll, dtype=np.uint8).tobytes()
        have = len(plain) + ll
        kind = rng.random()
        if kind < 0.25:
            off = int(rng.integers(1, min(have, 8) + 1))                   # overlapping / run-length
        elif kind < 0.55:
            off = int(rng.integers(1, min(have, 64) + 1))                  # near: inside the current batch
        elif kind < 0.8:
            off = int(rng.integers(1, min(have, 2000) + 1))
        else:
            off = int(rng.integers(1, min(have, 65535) + 1))
        tok = (min(ll, 15) << 4) | min(ml - 4, 15)
        comp.append(tok)
        if ll >= 15:
            put_len(comp, ll - 15)
        comp += lits
        comp += bytes([off & 0xFF, off >> 8])
        if ml - 4 >= 15:
            put_len(comp, ml - 4 - 15)
        plain += lits
        start = len(plain) - off
        for i in range(ml):
            plain.append(plain[start + i])
    tail = int(rng.integers(12, 40))                                      # closing literal run
    lits = rng.integers(0, 256, tail, dtype=np.uint8).tobytes()
    comp.append(min(tail, 15) << 4)
    if tail >= 15:
        put_len(comp, tail - 15)
    comp += lits; plain += lits
    return np.frombuffer(bytes(comp), dtype=np.uint8).copy(), np.frombuffer(bytes(plain), dtype=np.uint8).copy()
