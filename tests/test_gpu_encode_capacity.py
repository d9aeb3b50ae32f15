"""The encoders' answer to "does the block fit dstCap" and where they write, on the GPU.  tests/test_encode_capacity.py sweeps the
lane emulation of the device source over the capacities around a block's compressed size; what exists only on the GPU -- the
kernels of plz4hip.hip around the emit stage, the few-block encoder's gather, the body routes, the route selection by block count and
size, wide stores next to a block's end, the staging of dstCap per chunk -- is swept here: result code and every byte against the
reference at capacities full - 2 .. full + 1, 0, 1 and bound; every byte of a caller's device buffer outside a block's dstCap
compared with its prefill; records whose block compresses to bsz - 1, bsz and bsz + 1 bytes, the stored / compressed flip.

The reference is computed once per (input, level) at bound(n): below that size it answers 0, at or above it the same bytes
(asserted capacity by capacity against the real liblz4 in tests/test_encode_capacity.py's threshold_sweep)."""
import numpy as np
import pytest

import capcases as cc
import hcdict
from capcases import bound

pytestmark = pytest.mark.gpu

K64 = 64 << 10
FILL = 0xA5
POISON = -77


@pytest.fixture(scope="module")
def eng():
    from plz4_amd._native import Engine
    e = Engine(0)
    yield e
    e.close()


def _fresh_engine():
    from plz4_amd._native import Engine
    return Engine(0)


_FULL = {}


def _full(key, src, fn):
    """(size, bytes) of `src` at bound(n) under the reference function `fn`, computed once per key"""
    k = (key, src.ctypes.data, src.size)
    if k not in _FULL:
        r, c = fn(src, bound(src.size))
        assert r > 0
        _FULL[k] = (r, c[:r].copy(), src)                    # (src kept alive: its address is part of the key)
    return _FULL[k][:2]


def _ref_fn(ref, level):
    return ref.compress_fast if level == 1 else (lambda s, c: ref.compress_hc(s, c, level))


def _want(full, comp, cap):
    return (full, comp) if cap >= full else (0, comp[:0])


def _caps7(full, n):
    return [full - 2, full - 1, full, full + 1, 0, 1, bound(n)]


@pytest.fixture(scope="module")
def many():
    """30 inputs: generator blocks, two of the corpus and two around 64 KiB; at seven capacities each, 210 blocks in a call"""
    big = cc.big_blocks()
    return cc.spec_blocks(26, 0xCAB) + [b for b in cc.corpus_blocks() if b.size in (4097, 20000)] + [big[0], big[2]]


@pytest.fixture(scope="module")
def few_l1():
    """14 generator blocks and the 65 547- and 70 001-byte inputs: 112 blocks in a call, the few-block level-1 path"""
    big = cc.big_blocks()
    return cc.spec_blocks(14, 0xCAC) + [big[1], big[2]]


def _batch_verdicts(ref, e, inputs, level):
    srcs, caps, want = [], [], []
    for s in inputs:
        full, comp = _full(("plain", level), s, _ref_fn(ref, level))
        for cap in _caps7(full, s.size):
            srcs.append(s); caps.append(cap); want.append(_want(full, comp, cap))
    res, outs = e.compress_batch(srcs, caps, level=level)
    for i, (s, cap, (wr, wo)) in enumerate(zip(srcs, caps, want)):
        assert int(res[i]) == wr, (level, i, s.size, cap, int(res[i]), wr)
        assert np.array_equal(outs[i], wo), (level, i, s.size, cap)
    return len(srcs)


# ---- a. host-batch verdicts
@pytest.mark.parametrize("level", [1, 2, 3, 6, 9, 10, 12])
def test_batch_verdicts_many_blocks(ref, eng, many, level):
    """More than 128 blocks in the call: the many-block routes of every level (the few-block counter does not move)."""
    c0 = eng.counters()
    assert _batch_verdicts(ref, eng, many, level) > 128
    assert eng.counters()["fx_blocks"] == c0["fx_blocks"]


def test_batch_verdicts_few_block_level1(ref, eng, few_l1):
    c0 = eng.counters()
    assert _batch_verdicts(ref, eng, few_l1, 1) <= 128
    assert eng.counters()["fx_blocks"] > c0["fx_blocks"]


def test_batch_verdicts_level1_fused(ref, many, few_l1, monkeypatch):
    """PLZ4HIP_L1_FUSED=1: the one-kernel level-1 encoder, for the many-block call and the one the few-block path would take."""
    monkeypatch.setenv("PLZ4HIP_L1_FUSED", "1")
    e = _fresh_engine()
    try:
        _batch_verdicts(ref, e, many, 1)
        _batch_verdicts(ref, e, few_l1, 1)
        assert e.counters()["fx_blocks"] == 0
    finally:
        e.close()


@pytest.mark.parametrize("level", [3, 9])
def test_batch_verdicts_hc_small_segments(ref, many, level, monkeypatch):
    """PLZ4HIP_HC_MIN_SEG=2048 PLZ4HIP_HC_SEGS=16: blocks from 4 KiB on are stitched from up to sixteen segments."""
    monkeypatch.setenv("PLZ4HIP_HC_MIN_SEG", "2048")
    monkeypatch.setenv("PLZ4HIP_HC_SEGS", "16")
    e = _fresh_engine()
    try:
        _batch_verdicts(ref, e, many, level)
    finally:
        e.close()


# ---- b. dictionary verdicts
DICT_SIZES = (13, 777, 4096, 4097, 9000, 70000)
SWITCHES = [None, ("PLZ4HIP_HCX", "0"), ("PLZ4HIP_FX_LINKED", "0"), ("PLZ4HIP_HC_EXT_OFF", "1")]


@pytest.fixture(scope="module")
def dict_blocks():
    return [cc.hist_block(n, 2000 + n, cc.DICT64) for n in DICT_SIZES]


@pytest.mark.parametrize("switch", SWITCHES, ids=lambda s: "default" if s is None else "%s=%s" % s)
def test_dict_verdicts(ref, orc, dict_blocks, switch, monkeypatch):
    """plz4hip_compress_batch_dict under a 64 KiB text dictionary, blocks on both sides of the 4 KiB switch, at full - 2 .. full + 1:
    level 1 against the oracle's StreamIndieCtx, the HC levels against the real liblz4 stream with the dictionary attached.  The
    counters show which route ran: the wave-wide parser takes the three small blocks unless PLZ4HIP_HCX=0, the few-block level-1
    path the whole level-1 call unless PLZ4HIP_FX_LINKED=0."""
    if switch:
        monkeypatch.setenv(*switch)
    e = _fresh_engine()
    d = e.dict_create(cc.DICT_USER)
    try:
        dctx = orc.dict_ctx(cc.DICT_USER)
        for level in (1, 2, 5, 12):
            if level == 1:
                fn = lambda s, c: orc.compress_indie_dict(s, c, dctx)
            else:
                keep, daddr = ref.new_dict_ctx_hc(cc.DICT64, level)
                fn = ref.stream_ctx_hc(level, daddr)
            srcs, caps, want = [], [], []
            for s in dict_blocks:
                full, comp = _full(("dict", level), s, fn)
                for cap in range(full - 2, full + 2):
                    srcs.append(s); caps.append(cap); want.append(_want(full, comp, cap))
            c0 = e.counters()
            res, outs = e.compress_batch_dict(srcs, caps, d, level=level)
            c1 = e.counters()
            for i, (s, cap, (wr, wo)) in enumerate(zip(srcs, caps, want)):
                assert int(res[i]) == wr, (switch, level, s.size, cap, int(res[i]), wr)
                assert np.array_equal(outs[i], wo), (switch, level, s.size, cap)
            small = 4 * sum(1 for s in dict_blocks if s.size <= 4096)
            if level == 1:
                assert (c1["fxl_blocks"] > c0["fxl_blocks"]) == (switch is None or switch[0] != "PLZ4HIP_FX_LINKED"), (switch, c0, c1)
            else:
                assert c1["hcx_blocks"] - c0["hcx_blocks"] == (0 if switch and switch[0] == "PLZ4HIP_HCX" else small), (switch, level)
    finally:
        e.dict_destroy(d)
        e.close()


# ---- c. write bounds on the device
def _dev_compress(eng, ref, inputs, caps_of, level, max_len):
    """One plz4hip_dev_compress call over `inputs` x caps_of(full, n) with per-block capacities, destination prefilled with FILL and
    results with POISON: results and bytes are the reference's, every byte outside a block's dstCap still holds FILL, the source
    is unchanged."""
    import torch
    dev = torch.device("cuda:0")
    blocks = []
    for s in inputs:
        full, comp = _full(("plain", level), s, _ref_fn(ref, level))
        for cap in caps_of(full, s.size):
            blocks.append((s, cap, _want(full, comp, cap)))
    nb = len(blocks)
    sstride = (max(s.size for s, _, _ in blocks) + 255) // 256 * 256 + 256
    dstride = (max(cap for _, cap, _ in blocks) + 255) // 256 * 256 + 256
    src = np.full(nb * sstride, 0x5A, dtype=np.uint8)
    for i, (s, _, _) in enumerate(blocks):
        src[i * sstride:i * sstride + s.size] = s
    d_src = torch.from_numpy(src).to(dev)
    d_len = torch.tensor([s.size for s, _, _ in blocks], dtype=torch.int32, device=dev)
    d_cap = torch.tensor([cap for _, cap, _ in blocks], dtype=torch.int32, device=dev)
    d_dst = torch.full((nb * dstride,), FILL, dtype=torch.uint8, device=dev)
    d_res = torch.full((nb,), POISON, dtype=torch.int32, device=dev)
    true_max = max(s.size for s, _, _ in blocks)
    eng._chk(eng.L.plz4hip_dev_compress(eng.h, nb, d_src.data_ptr(), sstride, d_len.data_ptr(), d_dst.data_ptr(), dstride, d_cap.data_ptr(),
                                        level, true_max if max_len else 0, d_res.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    res = d_res.cpu().numpy(); out = d_dst.cpu().numpy()
    model = np.full(nb * dstride, FILL, dtype=np.uint8)
    for i, (s, cap, (wr, wo)) in enumerate(blocks):
        assert int(res[i]) == wr, (level, max_len, i, s.size, cap, int(res[i]), wr)
        assert np.array_equal(out[i * dstride:i * dstride + wr], wo), (level, max_len, i, s.size, cap)
        model[i * dstride:i * dstride + cap] = out[i * dstride:i * dstride + cap]     # inside the capacity: anything
    bad = np.flatnonzero(out != model)
    assert bad.size == 0, (level, max_len, "block %d: byte %d behind its capacity of %d written" %
                           (bad[0] // dstride, bad[0] % dstride - blocks[bad[0] // dstride][1], blocks[bad[0] // dstride][1]))
    assert np.array_equal(d_src.cpu().numpy(), src)
    return nb


def _caps6(full, n):
    return [full - 1, full, full + 1, bound(n), 0, 1]


@pytest.fixture(scope="module")
def dev_inputs():
    return cc.spec_blocks(2, 0xCAD) + [b for b in cc.corpus_blocks() if b.size in (4097, 20000)]


@pytest.mark.parametrize("level,max_len", [(1, True), (1, False), (2, True), (5, True), (9, True), (12, True)])
def test_dev_compress_writes_inside_dstcap(ref, eng, dev_inputs, level, max_len):
    """24 blocks with mixed capacities in one call, per level; level 1 with the true maxLen (the staged call) and with maxLen = 0
    (the one-kernel encoder)."""
    assert _dev_compress(eng, ref, dev_inputs, _caps6, level, max_len) == 24


def test_dev_compress_few_block_path_writes_inside_dstcap(ref, eng, dev_inputs):
    """The few-block level-1 path writing into a caller's buffer: a 70 001-byte block at full - 1 and at full among small ones."""
    c0 = eng.counters()
    _dev_compress(eng, ref, [cc.big_blocks()[2], dev_inputs[0]], lambda full, n: [full - 1, full], 1, True)
    assert eng.counters()["fx_blocks"] > c0["fx_blocks"]


# ---- d. records at the stored / compressed flip
def _tight_set(size_fn_of, seed):
    """blocks of 64 KiB whose reference size is bsz - 1, bsz, bsz + 1 and a short last block of 100 random bytes (its compressed
    form is longer than its plaintext yet below bsz: the reference keeps it compressed); size_fn_of(previous blocks) -> size_fn"""
    blocks = []
    for k, target in enumerate((K64 - 1, K64, K64 + 1)):
        blocks.append(cc.tight_block(size_fn_of(blocks), K64, target, seed=seed * 10 + k))
    blocks.append(np.random.Generator(np.random.PCG64(seed + 99)).integers(0, 256, size=100, dtype=np.uint8))
    return blocks


def _flags(recs):
    return [bool(bytes(r)[3] & 0x80) for r in recs]


_PLAIN = {}


def _plain_set(ref, orc, level):
    """(blocks, {checksum: records}) for independent blocks without dictionary"""
    if level not in _PLAIN:
        fn = _ref_fn(ref, level)
        blocks = _tight_set(lambda prev: (lambda b: fn(b, bound(b.size))[0]), 100 + level)
        want = {}
        for cks in (False, True):
            if level == 1:
                want[cks] = [orc.block_record(b, K64, cks).tobytes() for b in blocks]
            else:
                want[cks] = hcdict.ref_records(ref, orc, blocks, K64, level, False, None, checksum=cks)[0]
        assert _flags(want[True]) == [False, False, True, False]          # bsz - 1 and bsz compressed, bsz + 1 stored, the short one compressed
        _PLAIN[level] = (blocks, want)
    return _PLAIN[level]


def _l1_records(orc, blocks, linked, dctx, cks):
    out, prev = [], None
    for b in blocks:
        if linked:
            r, c = orc.compress_linked(b, K64, None if prev is None else prev[-65536:].copy(), dctx if prev is None else None)
        else:
            r, c = orc.compress_indie_dict(b, K64, dctx)
        out.append(hcdict.record(orc, r, c, b, cks)); prev = b
    return out


@pytest.mark.parametrize("level", [1, 2, 5, 12])
def test_records_at_the_flip_host(ref, orc, eng, level):
    """plz4hip_encode_records with and without block checksums; decoded back."""
    blocks, want = _plain_set(ref, orc, level)
    for cks in (False, True):
        got = eng.encode_records(blocks, K64, cks, level=level)
        assert [g.tobytes() for g in got] == want[cks], (level, cks, [g.size for g in got])
        res, st, outs = eng.decode_records([np.ascontiguousarray(g) for g in got], K64, cks)
        assert not any(st) and all(np.array_equal(o, b) for o, b in zip(outs, blocks)), (level, cks)


@pytest.mark.parametrize("level", [1, 2, 5, 12])
def test_records_at_the_flip_device(ref, orc, eng, level):
    """plz4hip_dev_encode_records + plz4hip_dev_compact_records, and plz4hip_dev_encode_body at the levels it takes (1 and 2), on
    contiguous plaintext: three full blocks and the short one."""
    import torch
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    blocks, want = _plain_set(ref, orc, level)
    data = np.concatenate(blocks); nb = len(blocks)
    d_src = torch.from_numpy(data).to(dev)
    stride = eng.stage_stride(K64)
    for cks in (False, True):
        body = np.frombuffer(b"".join(want[cks]), dtype=np.uint8)
        d_stage = torch.full((nb * stride,), FILL, dtype=torch.uint8, device=dev)
        d_len = torch.full((nb,), POISON, dtype=torch.int32, device=dev)
        d_off = torch.full((nb + 1,), -1, dtype=torch.int64, device=dev)
        d_body = torch.full((body.size + 256,), FILL, dtype=torch.uint8, device=dev)
        eng.dev_encode_records(d_src.data_ptr(), data.size, K64, cks, d_stage.data_ptr(), d_len.data_ptr(), s, level=level)
        eng.dev_compact_records(d_stage.data_ptr(), stride, d_len.data_ptr(), nb, d_off.data_ptr(), d_body.data_ptr(), body.size, s)
        torch.cuda.synchronize()
        assert [int(x) for x in d_len.cpu().numpy()] == [len(w) for w in want[cks]], (level, cks)
        assert int(d_off[-1].item()) == body.size
        got = d_body.cpu().numpy()
        assert np.array_equal(got[:body.size], body) and (got[body.size:] == FILL).all(), (level, cks)
        if level <= 2:
            d_body = torch.full((body.size + 256,), FILL, dtype=torch.uint8, device=dev)
            d_off = torch.full((nb + 1,), -1, dtype=torch.int64, device=dev)
            d_len = torch.full((nb,), POISON, dtype=torch.int32, device=dev)
            eng.dev_encode_body(d_src.data_ptr(), data.size, K64, cks, d_body.data_ptr(), body.size, d_off.data_ptr(), d_len.data_ptr(), s, level=level)
            torch.cuda.synchronize()
            assert [int(x) for x in d_len.cpu().numpy()] == [len(w) for w in want[cks]], (level, cks)
            assert int(d_off[-1].item()) == body.size
            got = d_body.cpu().numpy()
            assert np.array_equal(got[:body.size], body) and (got[body.size:] == FILL).all(), (level, cks, "body")
        assert np.array_equal(d_src.cpu().numpy(), data)


@pytest.mark.parametrize("level", [1, 2, 5, 12])
def test_records_at_the_flip_with_history(ref, orc, eng, level):
    """plz4hip_encode_records_ex: independent blocks under a dictionary, and one linked frame.  Every block is tuned under the
    history it is encoded with.  A linked block above level 1 that does not fit is the stored record, as include/plz4hip.h
    documents it."""
    dctx = orc.dict_ctx(cc.DICT_USER)
    d = eng.dict_create(cc.DICT_USER)
    try:
        # independent blocks under the dictionary
        if level == 1:
            size_of = lambda prev: (lambda b: orc.compress_indie_dict(b, bound(b.size), dctx)[0])
        else:
            keep, daddr = ref.new_dict_ctx_hc(cc.DICT64, level)
            comp = ref.stream_ctx_hc(level, daddr)
            size_of = lambda prev: (lambda b: comp(b, bound(b.size))[0])
        blocks = _tight_set(size_of, 200 + level)
        want = _l1_records(orc, blocks, False, dctx, True) if level == 1 else hcdict.ref_records(ref, orc, blocks, K64, level, False, cc.DICT_USER)[0]
        assert _flags(want) == [False, False, True, False]
        got = eng.encode_records_ex(blocks, K64, True, linked=False, d=d, level=level)
        assert [g.tobytes() for g in got] == want, (level, "dict", [g.size for g in got])
        res, st, outs, _ = eng.decode_records_ex([np.ascontiguousarray(g) for g in got], K64, True, linked=False, d=d)
        assert not any(st) and all(np.array_equal(o, b) for o, b in zip(outs, blocks)), (level, "dict")

        # one linked frame: block k is tuned behind block k - 1's last 64 KiB
        if level == 1:
            size_of = lambda prev: (lambda b: orc.compress_linked(b, bound(b.size), prev[-1][-65536:].copy() if prev else None)[0])
        else:
            def size_of(prev):
                def size(b):
                    lk = ref.stream_linked_ctx_hc(level)
                    return lk(b, bound(b.size), prev[-1][-65536:].copy() if prev else None)[0]
                return size
        blocks = _tight_set(size_of, 300 + level)
        want = _l1_records(orc, blocks, True, None, True) if level == 1 else hcdict.ref_records(ref, orc, blocks, K64, level, True, None)[0]
        assert _flags(want) == [False, False, True, False]
        got = eng.encode_records_ex(blocks, K64, True, linked=True, level=level)
        assert [g.tobytes() for g in got] == want, (level, "linked", [g.size for g in got])
        window = np.zeros(65536, dtype=np.uint8)
        res, st, outs, _ = eng.decode_records_ex([np.ascontiguousarray(g) for g in got], K64, True, linked=True, window=window, window_len=0)
        assert not any(st) and all(np.array_equal(o, b) for o, b in zip(outs, blocks)), (level, "linked")
    finally:
        eng.dict_destroy(d)
