"""The decoders on damaged input, on the GPU: what a call answers is the oracle's, and no byte outside a block's capacity, a
record's output area or the source is written.  Every device buffer is prefilled with 0xA5 and compared whole afterwards.  The
same property on the lane-emulated code, under the sanitizers and with reads included, is tests/emu/decode_bounds_main.cpp's
(tests/test_decode_bounds.py); these tests cover the entry points and launch shapes that program cannot see --
plz4hip_dev_decompress, the record routes on a body of exactly the records' length, plz4hip_dev_scatter_records."""
import numpy as np
import pytest

from lz4blocks import make_block
from plz4_amd import synth

pytestmark = pytest.mark.gpu

K64 = 64 << 10
FILL = 0xA5
DX_MAX_OUT = (4 << 20) + 8                                   # kDxMaxOut, lz4_dx_device.inl
OK, SIZE_OVERFLOW, CORRUPT = 0, 2, 3


@pytest.fixture(scope="module")
def eng():
    from plz4_amd._native import Engine
    e = Engine(0)
    yield e
    e.close()


def _flip(c, rng):
    d = c.copy(); d[int(rng.integers(0, d.size))] ^= 1 << int(rng.integers(0, 8)); return d


def _zero_offset(c):
    """the first sequence's offset <- 0"""
    d = c.copy(); ll = int(d[0]) >> 4; at = 1
    if ll == 15:
        while True:
            b = int(d[at]); at += 1; ll += b
            if b != 255:
                break
    d[at + ll] = 0; d[at + ll + 1] = 0
    return d


@pytest.fixture(scope="module")
def raw_blocks(orc):
    """(compressed bytes, plaintext size) of the blocks the dev_decompress tests draw from: generator-built ones, oracle-compressed
    text of 20 .. 300 KB (several 8 KiB segments of the few-block path), an empty one, random bytes, and damaged copies."""
    rng = np.random.default_rng(7)
    gen = [make_block(rng, n) for n in (5, 60, 600)]
    texts = [synth.text(n, seed=n) for n in (20000, 100000, 300000)]
    comp = [orc.compress_fast(t, orc.bound(t.size))[1].copy() for t in texts]
    assert comp[1].size > 3 * 8192 and comp[2].size < 512 << 10
    small = [(c, p.size) for c, p in gen[:2]] + [(comp[0], texts[0].size)]
    big = [(gen[2][0], gen[2][1].size), (comp[1], texts[1].size), (comp[2], texts[2].size)]
    odd = [(np.zeros(0, dtype=np.uint8), 0), (rng.integers(0, 256, 5000, dtype=np.uint8), 5000)]
    dam_big = [(_flip(comp[1], rng), texts[1].size), (comp[2][:comp[2].size - 77].copy(), texts[2].size), (_zero_offset(gen[2][0]), gen[2][1].size)]
    dam_small = [(_flip(gen[1][0], rng), gen[1][1].size), (comp[0][:comp[0].size - 9].copy(), texts[0].size), (_zero_offset(gen[0][0]), gen[0][1].size)]
    return {"twelve": small + big + odd + dam_big + dam_small[:1], "small": small + odd + dam_small, "one": (comp[0], texts[0].size)}


def _dev_decompress(eng, orc, blocks, caps, stride, dst_bytes=None):
    """one call; returns the results after checking them, the outputs, the gaps behind every capacity and the source"""
    import torch
    dev = torch.device("cuda:0")
    nb = len(blocks)
    src = np.full(nb * stride, FILL, dtype=np.uint8)
    for i, (c, _) in enumerate(blocks):
        assert c.size <= stride and caps[i] <= stride or dst_bytes
        src[i * stride:i * stride + c.size] = c
    d_src = torch.from_numpy(src).to(dev)
    d_dst = torch.full((dst_bytes or nb * stride,), FILL, dtype=torch.uint8, device=dev)
    d_len = torch.tensor([c.size for c, _ in blocks], dtype=torch.int32, device=dev)
    d_cap = torch.tensor(caps, dtype=torch.int32, device=dev)
    d_res = torch.full((nb,), -9, dtype=torch.int32, device=dev)
    eng.dev_decompress(nb, d_src.data_ptr(), stride, d_len.data_ptr(), d_dst.data_ptr(), stride, d_cap.data_ptr(), d_res.data_ptr(),
                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    res = d_res.cpu().numpy(); out = d_dst.cpu().numpy()
    assert np.array_equal(d_src.cpu().numpy(), src)
    for i, (c, _) in enumerate(blocks):
        want, plain = orc.decompress_safe(c, caps[i])
        assert int(res[i]) == want, (i, c.size, caps[i], int(res[i]), want)
        if want > 0:
            assert np.array_equal(out[i * stride:i * stride + want], plain), i
        end = (i + 1) * stride if not dst_bytes else out.size
        assert (out[i * stride + caps[i]:end] == FILL).all(), (i, caps[i])
    return res


def _caps(blocks):
    return [max(v, 0) for v in ((p, p + 8, p - 1, p // 2)[i % 4] for i, (_, p) in enumerate(blocks))]


@pytest.mark.parametrize("route", ["few-block", "one-wave", "129 blocks"])
def test_dev_decompress_parity_and_gaps(eng, orc, raw_blocks, monkeypatch, route):
    """plz4hip_dev_decompress: result[i] and the bytes are orc.decompress_safe's for good and damaged blocks at capacities p, p + 8,
    p - 1, p / 2 held on the device; every byte from dst + i * stride + cap_i to the next block is untouched; the source is unchanged.
    Twelve blocks at a 512 KiB stride on the few-block path (its counter rises) and on the one-wave kernel (it does not), 129 blocks
    at a 32 KiB stride beyond the few-block limit."""
    if route == "one-wave":
        monkeypatch.setenv("PLZ4HIP_DX_MAX_BLOCKS", "0")
    if route == "129 blocks":
        blocks = [raw_blocks["small"][i % len(raw_blocks["small"])] for i in range(129)]
        stride = 32 << 10
    else:
        blocks = raw_blocks["twelve"]
        stride = 512 << 10
    assert len(blocks) in (12, 129)
    before = eng.counters()["dx_blocks"]
    res = _dev_decompress(eng, orc, blocks, _caps(blocks), stride)
    after = eng.counters()["dx_blocks"]
    assert (res > 0).any() and (res < 0).any()
    if route == "few-block":
        assert after > before
    else:
        assert after == before


def test_dev_decompress_one_block(eng, orc, raw_blocks):
    """nBlocks == 1: the workspace is sized from 6 MiB / kDxMaxOut, not from the strides.  Capacity p: the few-block path answers;
    kDxMaxOut + 1: it declines and the one-wave kernel answers the same."""
    c, p = raw_blocks["one"]
    before = eng.counters()["dx_blocks"]
    r0 = _dev_decompress(eng, orc, [(c, p)], [p], K64)
    mid = eng.counters()["dx_blocks"]
    r1 = _dev_decompress(eng, orc, [(c, p)], [DX_MAX_OUT + 1], K64, dst_bytes=DX_MAX_OUT + 1)
    after = eng.counters()["dx_blocks"]
    assert int(r0[0]) == p == int(r1[0])
    assert mid == before + 1 and after == mid


# ---- records

@pytest.fixture(scope="module")
def plain4():
    data = synth.text(4 * K64, seed=5)
    return [data[o:o + K64] for o in range(0, data.size, K64)]


def _word(v):
    return np.frombuffer(np.uint32(v).tobytes(), dtype=np.uint8)


def _hostile_records(orc, plain4, cks, where, short_len):
    """-> (records, index of the plaintext or None): four good records, between them one whose size word says recLen - 3, one with
    bsz + 1, one with 0x7FFFFFFF, and one cut down to short_len bytes (0 .. 3; with checksums also 4 .. 7), last or in the middle"""
    good = [orc.block_record(b, K64, cks) for b in plain4]
    lie = good[1].copy(); lie[:4] = _word(lie.size - 3)
    over = good[2].copy(); over[:4] = _word(K64 + 1)
    huge = good[3].copy(); huge[:4] = _word(0x7FFFFFFF)
    short = good[0][:short_len].copy()
    recs = [(good[0], 0), (good[1], 1), (lie, None), (good[2], 2), (over, None), (huge, None), (good[3], 3)]
    recs.insert(len(recs) if where == "last" else 3, (short, None))
    return [r for r, _ in recs], [k for _, k in recs]


@pytest.mark.parametrize("where", ["last", "middle"])
@pytest.mark.parametrize("cks,short_len", [(False, n) for n in range(4)] + [(True, n) for n in range(8)])
def test_short_and_lying_records_on_every_route(eng, orc, plain4, monkeypatch, cks, short_len, where):
    """A body allocated at exactly the records' total length, with records too short for their size word (or checksum) and records
    whose size word lies: SIZE_OVERFLOW, result 0 and an untouched output area for those, the plaintext for their neighbours -- on
    the bulk kernels, the few-block path, the decode side of the duplex call, under a dictionary, and as one linked chain, where
    the first bad record ends the chain (CORRUPT, result 0 behind it) and the window is the one the good blocks leave."""
    import torch
    dev = torch.device("cuda:0")
    recs, which = _hostile_records(orc, plain4, cks, where, short_len)
    nb = len(recs)
    off = np.zeros(nb + 1, dtype=np.int64); off[1:] = np.cumsum([r.size for r in recs])
    body = np.concatenate(recs)
    d_body = torch.from_numpy(body).to(dev); d_off = torch.from_numpy(off).to(dev)
    assert d_body.numel() == int(off[-1])
    s = torch.cuda.current_stream().cuda_stream

    def fresh():
        return (torch.full((nb * K64,), FILL, dtype=torch.uint8, device=dev), torch.full((nb,), -9, dtype=torch.int32, device=dev),
                torch.full((nb,), -9, dtype=torch.int32, device=dev))

    def check(bufs, linked=False):
        torch.cuda.synchronize()
        out, res, st = (t.cpu().numpy() for t in bufs)
        assert np.array_equal(d_body.cpu().numpy(), body)
        dead = False
        for i, k in enumerate(which):
            area = out[i * K64:(i + 1) * K64]
            if k is None or dead:
                assert (int(st[i]), int(res[i])) == (CORRUPT if dead else SIZE_OVERFLOW, 0), (i, int(st[i]), int(res[i]))
                assert (area == FILL).all(), i
                dead = dead or linked
            else:
                assert (int(st[i]), int(res[i])) == (OK, K64), (i, int(st[i]), int(res[i]))
                assert np.array_equal(area, plain4[k]), i

    def plain_call(bufs):
        eng.dev_decode_records(d_body.data_ptr(), d_off.data_ptr(), nb, K64, cks, bufs[0].data_ptr(), K64, K64, bufs[1].data_ptr(), bufs[2].data_ptr(), s)

    def answered(name, before):
        """blocks the few-block path (dx_blocks) or the one with history outside the block (dxl_blocks) has answered since"""
        torch.cuda.synchronize()
        return eng.counters()[name] - before

    c0 = eng.counters()["dx_blocks"]
    bufs = fresh(); plain_call(bufs); check(bufs)                                        # the few-block path (8 records of <= 64 KiB)
    assert answered("dx_blocks", c0) > 0
    with monkeypatch.context() as m:
        m.setenv("PLZ4HIP_DX_MAX_BLOCKS", "0")                                           # the bulk kernels
        c0 = eng.counters()["dx_blocks"]
        bufs = fresh(); plain_call(bufs); check(bufs)
        assert answered("dx_blocks", c0) == 0
    d_stage = torch.zeros(eng.stage_stride(K64), dtype=torch.uint8, device=dev); d_len = torch.zeros(1, dtype=torch.int32, device=dev)
    bufs = fresh()                                                                       # the decode side of the duplex call
    eng.dev_duplex_records(d_stage.data_ptr(), 0, K64, cks, d_stage.data_ptr(), d_len.data_ptr(), d_body.data_ptr(), d_off.data_ptr(), nb, K64, cks,
                           bufs[0].data_ptr(), K64, K64, bufs[1].data_ptr(), bufs[2].data_ptr(), s)
    check(bufs)
    dct = eng.dict_create(synth.text(5000, seed=9))                                      # independent blocks under a dictionary
    try:
        for dx in ("128", "0"):
            with monkeypatch.context() as m:
                m.setenv("PLZ4HIP_DX_MAX_BLOCKS", dx)
                bufs = fresh(); c0 = eng.counters()["dxl_blocks"]
                eng.dev_decode_records_ex(d_body.data_ptr(), d_off.data_ptr(), nb, K64, cks, bufs[0].data_ptr(), K64, K64, bufs[1].data_ptr(),
                                          bufs[2].data_ptr(), linked=False, d=dct, stream=s)
                check(bufs)
                assert (answered("dxl_blocks", c0) > 0) == (dx == "128")
    finally:
        torch.cuda.synchronize()
        eng.dict_destroy(dct)
    for dx in ("128", "0"):                                                              # one linked chain
        with monkeypatch.context() as m:
            m.setenv("PLZ4HIP_DX_MAX_BLOCKS", dx)
            bufs = fresh(); c0 = eng.counters()["dxl_blocks"]
            d_win = torch.full((131072,), FILL, dtype=torch.uint8, device=dev); d_wl = torch.zeros(1, dtype=torch.int32, device=dev)
            eng.dev_decode_records_ex(d_body.data_ptr(), d_off.data_ptr(), nb, K64, cks, bufs[0].data_ptr(), K64, K64, bufs[1].data_ptr(),
                                      bufs[2].data_ptr(), linked=True, n_chains=1, windows_ptr=d_win.data_ptr(), window_len_ptr=d_wl.data_ptr(), stream=s)
            check(bufs, linked=True)
            first_bad = which.index(None)
            assert (answered("dxl_blocks", c0) > 0) == (dx == "128")
            assert first_bad >= 1 and int(d_wl.item()) == K64
            assert np.array_equal(d_win.cpu().numpy()[:K64], plain4[which[first_bad - 1]])


# ---- plz4hip_dev_scatter_records

SCATTER_LENS = [0, 1, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097, 32767, 32768, 32769, 100003]


@pytest.mark.parametrize("true_max", [True, False])
def test_scatter_records_against_numpy(eng, true_max):
    """dst[dstOff[k] : +len[k]] = src[srcOff[k] : +len[k]] for 70 entries around the kernel's 16-byte step and its 32 768-byte slice,
    source and destination offsets over every residue mod 16, destinations a permutation with gaps of 1 .. 40 bytes; entries with
    len 0, len -3, dstOff -1 and dstOff + len = dstCap + 1 are skipped, one ends exactly at dstCap.  maxLen = 1 gives one slice:
    the stride loop still moves everything.  The whole destination equals the model; the source is unchanged."""
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(3)
    n = 70
    lens = np.array([SCATTER_LENS[k % len(SCATTER_LENS)] for k in range(n)], dtype=np.int64)
    lens[20] = -3
    src_off = np.zeros(n, dtype=np.int64); pos = 0
    for k in range(n):
        pos += (k - pos) % 16                                                             # residue k mod 16
        src_off[k] = pos; pos += max(int(lens[k]), 0) + int(rng.integers(0, 9))
    src = rng.integers(0, 256, pos + 16, dtype=np.uint8)
    order = rng.permutation(n)
    dst_off = np.zeros(n, dtype=np.int64); pos = 3
    for j, k in enumerate(order):
        pos += int(rng.integers(1, 41))
        pos += (5 * j + 7 - pos) % 16                                                     # residues independent of the source's
        dst_off[k] = pos; pos += max(int(lens[k]), 0)
    last = int(order[-1])
    assert lens[last] > 0
    cap = int(dst_off[last] + lens[last])                                                 # the last one ends exactly at dstCap
    assert len({int(x) % 16 for x in src_off}) == 16 and len({int(x) % 16 for x in dst_off}) == 16
    skip = {int(k) for k in range(n) if lens[k] <= 0}
    dst_off[33] = -1; skip.add(33)
    over = next(int(k) for k in order[-2::-1] if lens[k] > 0 and k != 33)
    dst_off[over] = cap + 1 - lens[over]; skip.add(over)                                  # ends one byte past dstCap
    assert lens[over] > 0 and 33 not in (last, over) and 20 in skip and last not in skip
    model = np.full(cap, FILL, dtype=np.uint8)
    for k in range(n):
        if k not in skip:
            model[dst_off[k]:dst_off[k] + lens[k]] = src[src_off[k]:src_off[k] + lens[k]]
    d_src = torch.from_numpy(src).to(dev)
    d_so = torch.from_numpy(src_off).to(dev); d_do = torch.from_numpy(dst_off).to(dev)
    d_len = torch.from_numpy(lens.astype(np.int32)).to(dev)
    d_dst = torch.full((cap,), FILL, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    eng.dev_scatter_records(d_src.data_ptr(), d_so.data_ptr(), d_len.data_ptr(), d_do.data_ptr(), n, int(lens.max()) if true_max else 1,
                            d_dst.data_ptr(), cap, s)
    torch.cuda.synchronize()
    got = d_dst.cpu().numpy()
    assert np.array_equal(got, model), int(np.flatnonzero(got != model)[0])
    assert np.array_equal(d_src.cpu().numpy(), src)
    eng.dev_scatter_records(d_src.data_ptr(), d_so.data_ptr(), d_len.data_ptr(), d_do.data_ptr(), 0, 1, d_dst.data_ptr(), cap, s)   # n = 0: OK
