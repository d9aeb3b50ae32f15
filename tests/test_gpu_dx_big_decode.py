"""Raw blocks above 4 MiB through the C ABI: a call of few such blocks takes the few-block decoder's big path (k_dx_tables,
k_dxb_compose .. k_dxb_gather; dx_big_blocks of plz4hip_ctx_counters moves), and what it answers -- sizes, bytes, error codes -- is
the oracle's decompress_safe on the same bytes and capacity.  The same stages lane-emulated: tests/test_dx_big_decode.py; under the
sanitizers: tests/test_dx_big_bounds.py."""
import numpy as np
import pytest

import dx_big_cases as cases
from dx_big_cases import DX_MAX_OUT
from plz4_amd import synth

pytestmark = pytest.mark.gpu

FILL = 0xA5


@pytest.fixture(scope="module")
def eng():
    from plz4_amd._native import Engine
    e = Engine(0)
    yield e
    e.close()


def _batch(eng, orc, comps, caps):
    """one decompress_batch call, checked against the oracle block by block; returns how far dx_big_blocks moved"""
    c0 = eng.counters()["dx_big_blocks"]
    res, outs = eng.decompress_batch(comps, caps)
    for comp, cap, r, o in zip(comps, caps, res, outs):
        a, da = orc.decompress_safe(comp, cap)
        assert int(r) == a, (comp.size, cap, int(r), a)
        if a >= 0:
            assert np.array_equal(o, da), (comp.size, cap)
    return eng.counters()["dx_big_blocks"] - c0, res


@pytest.mark.parametrize("name,tight", [("T4+9", False), ("T16", False), ("T16", True), ("Z16", False), ("R9", False), ("M24", False), ("T64", False)])
def test_one_big_block(eng, orc, name, tight):
    src, comp = cases.shape(orc, name)
    n = src.size
    moved, res = _batch(eng, orc, [comp], [n if tight else n + 8])
    assert int(res[0]) == n and moved == 1
    c = eng.counters()
    if name == "Z16":
        assert c["dx_big_rounds_last"] >= 25
    if name in ("R9", "M24"):
        assert c["dx_big_runs_last"] >= 1


def test_big_and_small_blocks_in_one_call(eng, orc):
    t16, c16 = cases.shape(orc, "T16")
    plains = [t16, synth.text(300000, seed=21), synth.zeros(5 << 20), synth.text(18, seed=2)]
    comps = [c16] + [np.ascontiguousarray(orc.compress_fast(p, orc.bound(p.size))[1]).copy() for p in plains[1:]]
    assert comps[3].size <= 21                                  # (a token, a length byte, the literals)
    caps = [p.size + 8 for p in plains[:3]] + [plains[3].size]
    moved, res = _batch(eng, orc, comps, caps)
    assert [int(r) for r in res] == [p.size for p in plains]
    assert moved == sum(cap > DX_MAX_OUT for cap in caps) == 2


def test_short_capacities(eng, orc):
    src, comp = cases.shape(orc, "T16")
    for cap in (src.size - 1, src.size // 2):
        moved, res = _batch(eng, orc, [comp], [cap])
        assert int(res[0]) < 0 and moved == 0


def test_damaged_blocks(eng, orc):
    """twelve damaged 6 MiB text blocks, four per call: the oracle's results, codes included"""
    n = 6 << 20
    src = synth.text(n, seed=17)
    c, comp = orc.compress_fast(src, orc.bound(n))
    comp = np.ascontiguousarray(comp[:c])
    rng = np.random.default_rng(9)
    bad = [cases.damage(comp, rng, k % 4, (c // 7, c // 2, c - 70000)[k // 4]) for k in range(12)]
    nbad = 0
    for lo in range(0, 12, 4):
        _, res = _batch(eng, orc, bad[lo:lo + 4], [n + 8] * 4)
        nbad += int((res < 0).sum())
    assert nbad >= 3


def test_switched_off(eng, orc, monkeypatch):
    monkeypatch.setenv("PLZ4HIP_DX_BIG", "0")
    for name in ("T16", "Z16"):
        src, comp = cases.shape(orc, name)
        moved, res = _batch(eng, orc, [comp], [src.size + 8])
        assert int(res[0]) == src.size and moved == 0


def _dev_one(eng, orc, comp, cap, src_stride, dst_stride):
    """plz4hip_dev_decompress of one block, canaries behind the capacity; checked against the oracle"""
    import torch
    dev = torch.device("cuda:0")
    d_src = torch.from_numpy(comp).to(dev)
    d_dst = torch.full((cap + 4096,), FILL, dtype=torch.uint8, device=dev)
    d_len = torch.tensor([comp.size], dtype=torch.int32, device=dev)
    d_cap = torch.tensor([cap], dtype=torch.int32, device=dev)
    d_res = torch.full((1,), -9, dtype=torch.int32, device=dev)
    eng.dev_decompress(1, d_src.data_ptr(), src_stride, d_len.data_ptr(), d_dst.data_ptr(), dst_stride, d_cap.data_ptr(), d_res.data_ptr(),
                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    r = int(d_res.cpu()[0]); out = d_dst.cpu().numpy()
    assert np.array_equal(d_src.cpu().numpy(), comp)
    a, da = orc.decompress_safe(comp, cap)
    assert r == a, (comp.size, cap, r, a)
    if a > 0:
        assert np.array_equal(out[:a], da)
    assert (out[cap:] == FILL).all(), "bytes behind the capacity were written"
    return r


def test_dev_decompress_one_block_strides(eng, orc):
    """nBlocks == 1: strides no smaller than the compressed length and the capacity are the bounds; with zero strides the call is
    what it was"""
    src, comp = cases.shape(orc, "T16")
    cap = src.size + 8
    c0 = eng.counters()["dx_big_blocks"]
    assert _dev_one(eng, orc, comp, cap, comp.size, cap) == src.size
    c1 = eng.counters()["dx_big_blocks"]
    assert _dev_one(eng, orc, comp, cap, 0, 0) == src.size
    c2 = eng.counters()["dx_big_blocks"]
    assert c1 == c0 + 1 and c2 == c1


def test_workspace_grows_and_shrinks(orc):
    """one ctx: T16 -> trim -> T16 -> sixteen 4 MiB blocks on the few-block path -> Z16"""
    from plz4_amd._native import Engine
    e = Engine(0)
    try:
        t16, c16 = cases.shape(orc, "T16")
        z16, cz = cases.shape(orc, "Z16")
        assert _batch(e, orc, [c16], [t16.size + 8])[0] == 1
        e.trim()
        assert _batch(e, orc, [c16], [t16.size + 8])[0] == 1
        bsz = 4 << 20
        small = synth.text(bsz, seed=33)
        cs = np.ascontiguousarray(orc.compress_fast(small, orc.bound(bsz))[1]).copy()
        d0 = e.counters()["dx_blocks"]
        moved, res = _batch(e, orc, [cs] * 16, [bsz + 8] * 16)
        assert moved == 0 and e.counters()["dx_blocks"] == d0 + 16
        assert _batch(e, orc, [cz], [z16.size + 8])[0] == 1
    finally:
        e.close()


def test_hostile_blocks_stay_inside(eng, orc):
    """generator-built blocks of 5-6 MiB with long runs, good and damaged, one per dev_decompress call with canaries behind dst"""
    rng = np.random.default_rng(12)
    comp, plain = cases.make_big_block(rng, 5 << 20)
    assert 5 << 20 <= plain.size <= (6 << 20) + (1 << 20)
    c0 = eng.counters()["dx_big_blocks"]
    assert _dev_one(eng, orc, comp, plain.size + 8, comp.size, plain.size + 8) == plain.size
    assert eng.counters()["dx_big_blocks"] == c0 + 1
    for k in range(8):
        bad = cases.damage(comp, rng, k % 4, (comp.size // 5, comp.size // 2, comp.size - 200)[k % 3])
        cap = (plain.size + 8, plain.size, plain.size - 1)[k % 3]
        _dev_one(eng, orc, bad, cap, max(bad.size, comp.size), plain.size + 8)
