"""A linked decode call cut into groups of consecutive blocks (launch_decode's plan, dxl_group; the finish stage dxl_finish with the
window, its length and the chain's dead word carried from group to group) on the lane-emulated build of the same source
(tests/emu/emu_dxl_groups.cpp).  Every case is checked against the sequential walk with the oracle's LZ4_decompress_safe_usingDict
under the reference reader's window rule: results, status, bytes, the final window and its length -- and the number of blocks the
few-block path has to answer -- in both lane orders."""
import numpy as np
import pytest

import dxl_group_cases as gc


@pytest.fixture(scope="module")
def emu():
    return gc.DxlGroupsEmu()


@pytest.fixture(scope="module")
def cases(orc):
    return gc.build_cases(orc)


def _run(emu, case):
    for desc in (False, True):
        emu.set_descending(desc)
        try:
            got, windows, wlens, cnt, taken = emu.decode(case)
        finally:
            emu.set_descending(False)
        case.check(got, windows, wlens)
        nb = sum(len(ch) for ch in case.chains)
        assert cnt["groups"] == -(-nb // case.group), (case.name, cnt)
        assert cnt["taken"] == case.taken, (case.name, cnt, case.taken)
    return taken


def test_emu_dxl_groups_cases(emu, cases):
    names = [c.name for c in cases]
    assert len(set(names)) == len(names) and len(names) >= 25
    for case in cases:
        _run(emu, case)


def test_emu_dxl_groups_one_group_is_the_call(emu, cases):
    """group size >= the call's blocks: one group, the counters of an uncut call"""
    case = next(c for c in cases if c.name == "nine-d70000-g9")
    got, windows, wlens, cnt, taken = emu.decode(case)
    assert cnt == {"taken": 9, "rounds": cnt["rounds"], "groups": 1} and taken.all()


def test_emu_dxl_groups_rounds_follow_the_group(emu, cases):
    """the jump rounds a group needs do not grow with the call: the same chain in groups of 1 and of 9"""
    r = {}
    for g in (1, 9):
        case = next(c for c in cases if c.name == "nine-d70000-g%d" % g)
        r[g] = emu.decode(case)[3]["rounds"]
    assert 1 <= r[1] <= r[9] <= 22, r                                       # (ceil(log2(9 x 64 KiB + 64 KiB)) + 1 = 21 launched at most)


def test_emu_dxl_groups_dead_chain_leaves_the_others(emu, cases):
    """behind the bad block: result 0 / CORRUPT in this group and in every later one; the other chain is answered in full"""
    for case in (c for c in cases if c.name.startswith("bad-")):
        at = int(case.name[-1])
        got, windows, wlens, cnt, taken = emu.decode(case)
        res, st, _ = got[0]
        assert [int(x) for x in st[at + 1:]] == [gc.CORRUPT] * (6 - at) and not any(int(x) for x in res[at + 1:])
        assert list(taken) == [1] * at + [0] * (7 - at) + [1] * 5, (case.name, list(taken))


def test_emu_dxl_groups_flagged_group_walks_and_the_next_is_back(emu, orc):
    case = gc.flagged_case(orc)
    taken = _run(emu, case)
    assert list(taken) == [1, 1, 1, 0, 0, 0, 1, 1, 1]
    assert case.taken == 6
