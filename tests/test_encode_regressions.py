"""Inputs that once broke the level-1 encoder, kept as regression tests (found by tests/fuzz/fuzz_encode.py against the real
LZ4_compress_fast).  CPU: the lane-emulated device code; -m gpu: the kernel through the C ABI."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "fuzz"))
import fuzz_encode  # noqa: E402


def _case_long_match_to_block_end_after_twin_repair():
    """A match that runs to the end of the block (lz4.c:1233 ends the parse there) in a batch whose walk is redone after a
    twin repair: the redo must still end the block (it once re-tested past the last probe position and emitted a match
    inside the last 5 bytes)."""
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "enc_case_block_end_after_repair.npz"))["src"]


def test_emu_long_match_to_block_end_after_twin_repair(ref, orc):
    from emulib import Emu
    emu = Emu()
    src = _case_long_match_to_block_end_after_twin_repair()
    for desc in (False, True):
        emu.set_descending(desc)
        for cap in (orc.bound(src.size), src.size):
            a, da = ref.compress_fast(src, cap)
            b, db = emu.compress_fast(src, cap)
            assert a == b and np.array_equal(da, db), (src.size, cap, desc, a, b)
    emu.set_descending(False)


@pytest.mark.gpu
def test_gpu_long_match_to_block_end_after_twin_repair(orc):
    from plz4_amd._native import Engine
    eng = Engine(0)
    src = _case_long_match_to_block_end_after_twin_repair()
    caps = [orc.bound(src.size), src.size]
    res, outs = eng.compress_batch([src, src], caps)
    for cap, r, o in zip(caps, res, outs):
        want_n, want = orc.compress_fast(src, cap)
        assert int(r) == want_n and np.array_equal(o, want[:want_n]), (cap, int(r), want_n)
    n, out = orc.decompress_safe(np.ascontiguousarray(outs[0]), src.size)
    assert n == src.size and np.array_equal(out[:n], src)
    eng.close()


def _cases_long_match_to_block_end_verified_in_a_later_round():
    """The same ending where the repair takes a SECOND round: the first round measures the long match and sees it end the block, its
    commit is not verified, and the second round -- which hops through the match at its measured length, it is not special any
    more -- must still end the block.  It once left the grid batch with a re-test pending behind the last probe position; the
    generic batch executed it: a 4-byte match and one literal where the last five literals belong, a block that
    LZ4_decompress_safe refuses.  Found by tests/test_gpu_many_blocks.py on a linked 1 KiB block, kept as a fixture (`end`: runs of
    72, 15 and 20 bytes around six single ones, then one run to the block's end); the plain level-1 call shows it on the same
    kilobyte at the end of a block of 70 016 or 131 072 bytes of noise."""
    end = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "enc_case_block_end_later_round.npz"))["end"]
    rng = np.random.default_rng(7)
    return [np.concatenate([rng.integers(0, 256, size=n - end.size, dtype=np.uint8), end]) for n in (70016, 131072)]


def test_emu_long_match_to_block_end_verified_in_a_later_round(ref, orc):
    from emulib import Emu
    emu = Emu()
    for src in _cases_long_match_to_block_end_verified_in_a_later_round():
        for desc in (False, True):
            emu.set_descending(desc)
            for cap in (orc.bound(src.size), src.size):
                a, da = ref.compress_fast(src, cap)
                b, db = emu.compress_fast(src, cap)
                assert a == b and np.array_equal(da, db), (src.size, cap, desc, a, b)
        emu.set_descending(False)


@pytest.mark.gpu
def test_gpu_long_match_to_block_end_verified_in_a_later_round(ref, orc):
    from plz4_amd._native import Engine
    eng = Engine(0)
    srcs = _cases_long_match_to_block_end_verified_in_a_later_round()
    caps = [orc.bound(s.size) for s in srcs]
    res, outs = eng.compress_batch(srcs, caps)
    for s, cap, r, o in zip(srcs, caps, res, outs):
        want_n, want = ref.compress_fast(s, cap)
        assert int(r) == want_n and np.array_equal(o, want[:want_n]), (s.size, int(r), want_n)
        n, out = orc.decompress_safe(np.ascontiguousarray(o), s.size)
        assert n == s.size and np.array_equal(out[:n], s)
    eng.close()
