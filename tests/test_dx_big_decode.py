"""The few-block decoder's big path (raw blocks above 4 MiB + 8; dxb_* in plz4_amd/csrc/lz4_dx_device.inl) on the lane-emulated
build, stage by stage as launch_decode enqueues it (tests/emu/dx_train.h): whatever it answers is LZ4_decompress_safe's result
(the oracle's, same bytes and capacity), a valid block with room is ANSWERED, and what it leaves (LEFT) is the one-wave decoder's,
whose parity is tested elsewhere.  GPU: tests/test_gpu_dx_big_decode.py."""
import numpy as np
import pytest

import dx_big_cases as cases
from dx_big_cases import LEFT
from plz4_amd import synth


@pytest.fixture(scope="module")
def emu():
    e = cases.DxBigEmu()
    yield e
    e.set_descending(False)


def _check(orc, emu, comp, cap, must_take=False, **kw):
    a, da = orc.decompress_safe(comp, cap)
    r, out, st = emu.decode(comp, cap, **kw)
    if r == LEFT:
        assert not must_take, (comp.size, cap, a, kw)
        return None
    assert r == a and a >= 0 and np.array_equal(out, da), (comp.size, cap, r, a, kw)   # it only ever answers for blocks that decode
    return st


# (group, run threshold, lanes descending): group sizes 2, 4 and the default, thresholds 4 KiB and the default, both lane orders
SETTINGS = [(0, 0, False), (2, 4096, True), (4, 4096, False), (0, 0, True), (2, 0, False)]


@pytest.mark.parametrize("name", ["T4+9", "T16", "Z16", "R9", "M24"])
def test_emu_dx_big_shapes(orc, emu, name):
    src, comp = cases.shape(orc, name)
    n = src.size
    runs = set()
    for k, (group, thr, desc) in enumerate(SETTINGS):
        emu.set_descending(desc)
        for cap in ((n, n + 8, n - 1) if k < 2 else (n + 8,)):
            st = _check(orc, emu, comp, cap, must_take=cap >= n, group=group, thr=thr)
            if st is None:
                continue
            assert st["taken"] <= st["launched"] <= 32 and st["runs"] <= st["room"]
            if name == "Z16":
                assert st["launched"] >= 25, st                          # 2^24 pointers, each to the byte before it
            if name in ("R9", "M24"):
                assert st["runs"] >= 1, st
                runs.add((thr, st["runs"]))
    if name in ("R9", "M24"):
        assert len({t for t, _ in runs}) == 2                            # (the output was the oracle's under both thresholds)


@pytest.mark.parametrize("group", [2, 4])
def test_emu_dx_big_group_borders(orc, emu, group):
    """a slow entry on a group's first position; the first position behind a group border slow; the chain running into the block's
    end from the third-last segment of a three-group block"""
    for make in (cases.slow_at_group_start, cases.slow_behind_group_border, cases.early_tail_from_third_last):
        comp, plain = make(group)
        a, da = orc.decompress_safe(comp, plain.size)
        assert a == plain.size and np.array_equal(da, plain), make.__name__
        for desc in (False, True):
            emu.set_descending(desc)
            for cap in (plain.size, plain.size + 8, plain.size - 1):
                for g in (group, 2, 0):
                    st = _check(orc, emu, comp, cap, must_take=cap >= plain.size, group=g, thr=4096)
                    if st is not None and g == group and make is cases.early_tail_from_third_last:
                        assert st["groups"] == 3, st


def test_emu_dx_big_damaged_blocks(orc, emu):
    """60 damaged variants of a 5 MiB text block: whatever is answered is the oracle's answer"""
    emu.set_descending(False)
    n = 5 << 20
    src = synth.text(n, seed=11)
    c, comp = orc.compress_fast(src, orc.bound(n))
    comp = np.ascontiguousarray(comp[:c])
    rng = np.random.default_rng(31)
    answered = total = 0
    for at in (c // 7, c // 2, c - 70000, c - 20):
        for kind in range(4):
            for rep in range(4 if kind < 3 else 3):
                bad = cases.damage(comp, rng, kind, at)
                total += 1
                answered += _check(orc, emu, bad, n + 8, group=(0, 2, 4)[rep % 3], thr=(0, 4096)[rep % 2]) is not None
    assert total == 60 and answered >= 1      # (a flipped literal byte still decodes: the path answers, with the reference's wrong bytes)
