"""The encoders' answer to "does the block fit dstCap", on the lane-emulated build of the device source.  liblz4 checks the room
sequence by sequence (limitedOutput); the device code takes ONE comparison after the parse -- does the complete block exceed the
capacity (lz4_seq_device.inl, lz4hc_lazy_device.inl) -- and the fused, dictionary, two-table and one-thread encoders carry their
own copies of that arithmetic.  Every entry point of the emulation is swept over the capacities around the block's compressed size
against the function the other tests pair it with: result code and every byte.  The wrappers of tests/emulib.py put sentinel bytes
behind the capacity, so every call here (and every other encode test) also asserts that nothing is written at or past dst + cap."""
import numpy as np
import pytest

import capcases as cc
from capcases import WIDTH, bound


@pytest.fixture(scope="module")
def emu():
    from emulib import Emu
    return Emu()


def threshold_sweep(ref_fn, enc_fn, src, width, what=()):
    """full = the reference's size at bound(n); at every capacity in [full - width, full + width) the encoder(s) -- one callable
    or a dict of them -- answer what the reference answers, in size and bytes, and the reference itself answers 0 exactly below
    `full`: the property the one-comparison design rests on."""
    n = src.size
    full, whole = ref_fn(src, bound(n))
    assert full > 0, (what, n)
    whole = whole[:full].copy()
    encs = enc_fn if isinstance(enc_fn, dict) else {"": enc_fn}
    for cap in range(max(full - width, 0), full + width):
        want, wbytes = ref_fn(src, cap)
        assert want == (0 if cap < full else full), (what, n, cap, full, want)
        if want:
            assert np.array_equal(wbytes[:want], whole), (what, n, cap)
        for name, fn in encs.items():
            got, gbytes = fn(src, cap)
            assert got == want, (what, name, n, cap, full, got, want)
            assert np.array_equal(gbytes, wbytes[:want]), (what, name, n, cap, full)
    return full


@pytest.fixture(scope="module")
def blocks():
    return cc.spec_blocks(200, 0xCA9) + cc.corpus_blocks()


@pytest.fixture(scope="module")
def few():
    """the subset for the entry points that cost more per call, and the three blocks around 64 KiB"""
    return cc.spec_blocks(40, 0xCAA) + cc.corpus_blocks()[:4], cc.big_blocks()


def test_generator_reaches_the_edges(ref):
    """The generated blocks are what they are for: their level-1 sizes cover every residue mod 16, they hold runs and matches on
    both sides of 15 / 19 and 270 / 274, and blocks that end within liblz4's last-literals rules."""
    import hcx_cases
    sizes, lits, mls = set(), set(), set()
    for b in cc.spec_blocks(200, 0xCA9):
        r, comp = ref.compress_fast(b, bound(b.size))
        sizes.add(r % 16)
        at = 0
        for pos, ml, off in hcx_cases.sequences(comp[:r]):
            lits.add(pos - at); mls.add(ml); at = pos + ml
    assert len(sizes) == 16
    assert {14, 15, 16} <= lits and {254, 255, 270, 271} & lits
    assert {18, 19, 20} <= mls and {273, 274} & mls


def test_level1(ref, emu, blocks, few):
    for i, b in enumerate(blocks + few[1]):
        threshold_sweep(ref.compress_fast, {"staged": emu.compress_fast, "fused": emu.compress_fast_fused}, b, WIDTH, ("l1", i))


@pytest.mark.parametrize("level", range(2, 13))
def test_hc_one_thread(ref, emu, blocks, few, level):
    src = blocks if level in (2, 3, 9, 12) else few[0]
    for i, b in enumerate(src + few[1][:1 if level >= 10 else 3]):
        threshold_sweep(lambda s, c: ref.compress_hc(s, c, level), lambda s, c: emu.compress_hc(s, c, level), b, WIDTH, ("hc", level, i))


@pytest.mark.parametrize("level", [3, 5, 9, 11])
def test_hc_lazy_in_segments(ref, emu, few, level):
    encs = {"4x8192": lambda s, c: emu.compress_hc_lazy(s, c, level, 4, 8192), "16x300": lambda s, c: emu.compress_hc_lazy(s, c, level, 16, 300)}
    for i, b in enumerate(few[0] + few[1]):
        threshold_sweep(lambda s, c: ref.compress_hc(s, c, level), encs, b, WIDTH, ("lazy", level, i))


def test_hc12_phases(ref, emu, few):
    encs = {"whole": lambda s, c: emu.compress_hc12(s, c), "16x300": lambda s, c: emu.compress_hc12(s, c, 0, 256, 16, 300)}
    for i, b in enumerate(few[0][:20] + few[1][:1]):
        threshold_sweep(lambda s, c: ref.compress_hc(s, c, 12), encs, b, WIDTH, ("hc12", i))


def test_hc_mid(ref, emu, blocks, few):
    for i, b in enumerate(blocks + few[1]):
        threshold_sweep(lambda s, c: ref.compress_hc(s, c, 2), emu.compress_hc_mid, b, WIDTH, ("mid", i))


# ---- history outside the block
def _table(dctx):
    return np.ctypeslib.as_array(dctx.table).astype(np.uint32).copy()


@pytest.mark.parametrize("dct", [cc.DICT64, cc.DICT1000], ids=["dict64k", "dict1000"])
def test_level1_with_history(orc, emu, dct):
    """compress_dict mode 1 (a linked block behind the previous block's tail), mode 2 (> 4 KiB under a dictionary context: its
    table copied) and mode 3 (<= 4 KiB: looked up) against the oracle's streams, as tests/test_emu_kernels.py pairs them."""
    dctx = orc.dict_ctx(dct)
    tab = _table(dctx)
    for b in cc.hist_blocks(dct):
        n = b.size
        tail = dct.copy()
        threshold_sweep(lambda s, c: orc.compress_linked(s, c, tail), lambda s, c: emu.compress_dict(s, c, tail, 1), b, WIDTH, ("linked", n))
        mode = 2 if n > 4096 else 3
        threshold_sweep(lambda s, c: orc.compress_indie_dict(s, c, dctx), lambda s, c: emu.compress_dict(s, c, dct, mode, tab), b, WIDTH, ("indie", mode, n))


@pytest.mark.parametrize("level", [2, 3, 9, 12])
def test_hc_with_history(ref, emu, level):
    """compress_hc_dict mode 1 (external segment: a linked tail, or the dictionary in front of a block > 4 KiB) and mode 2 (the
    dictionary context of a block <= 4 KiB), and the list / two-table routes the kernels run behind a segment, against the real
    liblz4 streams."""
    for dct in (cc.DICT64, cc.DICT1000):
        keep, daddr = ref.new_dict_ctx_hc(dct, level)
        indie = ref.stream_ctx_hc(level, daddr)
        linked = ref.stream_linked_ctx_hc(level)
        tail = dct.copy()
        for b in cc.hist_blocks(dct):
            n = b.size
            if n > 9000 and (dct.size < 65536 or level > 3):
                continue                                    # (the 70 000-byte block at levels 2 and 3, behind the full dictionary)
            ext = {"one-thread": lambda s, c, seg=dct: emu.compress_hc_dict(s, c, level, seg, 1),
                   "lists": lambda s, c, seg=dct: emu.compress_hc_lazy_ext(s, c, level, seg),
                   "lists-16x300": lambda s, c, seg=dct: emu.compress_hc_lazy_ext(s, c, level, seg, 16, 300)}
            if level == 2:
                ext["mid"] = lambda s, c, seg=dct: emu.compress_hc_mid_ext(s, c, seg)
            threshold_sweep(lambda s, c: linked(s, c, tail), ext, b, WIDTH, ("linked", level, dct.size, n))
            if n > 4096:
                threshold_sweep(indie, ext, b, WIDTH, ("dict-seg", level, dct.size, n))
            else:
                threshold_sweep(indie, lambda s, c: emu.compress_hc_dict(s, c, level, dct, 2), b, WIDTH, ("dict-ctx", level, dct.size, n))


def test_hcx_wave_wide_parser(ref):
    """The wave-wide parser for blocks <= 4 KiB under a dictionary context, every level, both lane orders."""
    import hcx_cases
    from test_hcx_encode import HcxEmu
    hcx = HcxEmu()
    small = [b for b in cc.hist_blocks(cc.DICT64) if b.size <= 4096] + [cc.hist_block(n, 7 + n, cc.DICT64) for n in (65, 777, 1000)]
    for dct in (cc.DICT64, cc.DICT1000):
        for level in (hcx_cases.HCX_LEVELS if dct is cc.DICT64 else (2, 3, 9, 12)):
            keep, daddr = ref.new_dict_ctx_hc(dct, level)
            indie = ref.stream_ctx_hc(level, daddr)
            encs = {"asc": lambda s, c: hcx.compress(s, c, level, dct, False), "desc": lambda s, c: hcx.compress(s, c, level, dct, True)}
            for b in small:
                threshold_sweep(indie, encs, b, WIDTH, ("hcx", level, dct.size, b.size))
