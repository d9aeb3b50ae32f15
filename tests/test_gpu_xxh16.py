"""The LDS-free emit stage and the block checksums ahead of the bulk decode, on the GPU: k_l1_finish and k_rec_verify16 on
wave_xxh32_x16 (sixteen records per wave), k_scan / k_scan_from on one wave.  Records against the oracle's, offsets against the
running sum, the decoder's verdicts as they were -- a rejected record's output area is not touched."""
import numpy as np
import pytest

from plz4_amd import synth

pytestmark = pytest.mark.gpu

K64 = 64 << 10


@pytest.fixture(scope="module")
def eng():
    from plz4_amd._native import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def blocks35():
    """35 plaintext blocks of 64 KiB of synth kind M: text, random (stored records), text, zeros, ..."""
    data = synth.make("M", 35 * K64, K64)
    return [data[o:o + K64] for o in range(0, data.size, K64)]


@pytest.fixture(scope="module")
def records35(orc, blocks35):
    return [orc.block_record(b, K64, True) for b in blocks35]


@pytest.mark.parametrize("budget_mib", [0, 1])
def test_encode_records_and_body_with_checksums(orc, blocks35, records35, monkeypatch, budget_mib):
    """(i) 33 blocks of 64 KiB + a 5-byte and an empty block: records == the oracle's, offsets == the running sum of the lengths;
    budget_mib = 1 cuts the call into groups (k_scan_from with first = 0 for every group but the first; an engine of its own: the
    budget sizes a workspace that does not exist yet)."""
    import torch
    from plz4_amd._native import Engine
    if budget_mib:
        monkeypatch.setenv("PLZ4HIP_L1_BUDGET_MIB", str(budget_mib))
    eng = Engine(0)
    srcs = blocks35[:33] + [np.arange(5, dtype=np.uint8), np.zeros(0, dtype=np.uint8)]
    want = records35[:33] + [orc.block_record(b, K64, True) for b in srcs[33:]]
    assert any(int(np.frombuffer(w[:4].tobytes(), np.uint32)[0]) >> 31 for w in want)           # stored records occur
    recs = eng.encode_records(srcs, K64, True)
    for i, (r, w) in enumerate(zip(recs, want)):
        assert np.array_equal(r, w), i
    # the same plaintext contiguous in device memory, straight into a frame body: 33 full blocks and the 5-byte one
    dev = torch.device("cuda:0")
    srcs, want = srcs[:34], want[:34]
    data = np.concatenate(srcs)
    nb = len(srcs)
    wantBody = np.concatenate(want)
    d_src = torch.from_numpy(data).to(dev)
    d_body = torch.zeros(wantBody.size, dtype=torch.uint8, device=dev)                            # exact: the last record ends the allocation
    d_off = torch.full((nb + 1,), -1, dtype=torch.int64, device=dev)
    d_len = torch.zeros(nb, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    eng.dev_encode_body(d_src.data_ptr(), data.size, K64, True, d_body.data_ptr(), d_body.numel(), d_off.data_ptr(), d_len.data_ptr(), s)
    torch.cuda.synchronize()
    off = d_off.cpu().numpy(); ln = d_len.cpu().numpy()
    assert [int(x) for x in ln] == [w.size for w in want]
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(ln.astype(np.int64))]))
    assert np.array_equal(d_body.cpu().numpy(), wantBody)
    eng.close()


def test_scan_of_4097_records(eng):
    """(ii) 4097 blocks of 64 bytes into a body: recOff == cumsum(recLen)"""
    import torch
    dev = torch.device("cuda:0")
    nb, bsz = 4097, 64
    data = synth.make("M", nb * bsz, bsz)
    d_src = torch.from_numpy(data).to(dev)
    d_body = torch.zeros(nb * (bsz + 8), dtype=torch.uint8, device=dev)
    d_off = torch.full((nb + 1,), -1, dtype=torch.int64, device=dev)
    d_len = torch.zeros(nb, dtype=torch.int32, device=dev)
    eng.dev_encode_body(d_src.data_ptr(), data.size, bsz, True, d_body.data_ptr(), d_body.numel(), d_off.data_ptr(), d_len.data_ptr(),
                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ln = d_len.cpu().numpy().astype(np.int64)
    assert ln.min() >= 8 and ln.max() <= bsz + 8
    assert np.array_equal(d_off.cpu().numpy(), np.concatenate([[0], np.cumsum(ln)]))


def _damaged(records35):
    """wrong checksum at records 0, 15, 16 and 34; record 7's size word says bsz + 1; -> (records, expected statuses)"""
    recs = [r.copy() for r in records35]
    want_st = np.zeros(35, dtype=np.int32)
    for i in (0, 15, 16, 34):
        recs[i][4 + (recs[i].size - 8) // 2] ^= 0x10
        want_st[i] = 1                                                                            # PLZ4HIP_BLK_HASH_MISMATCH
    word = int(np.frombuffer(recs[7][:4].tobytes(), np.uint32)[0])
    recs[7][:4] = np.frombuffer(np.uint32((word & 0x80000000) | (K64 + 1)).tobytes(), np.uint8)
    want_st[7] = 2                                                                                # PLZ4HIP_BLK_SIZE_OVERFLOW
    return recs, want_st


@pytest.mark.parametrize("dx_off", [False, True])
def test_decode_rejects_before_it_decodes(orc, eng, blocks35, records35, monkeypatch, dx_off):
    """(iii) 35 records of 64 KiB with checksums, five of them damaged, stored ones among the good: statuses 1 / 2 / 0, result 0
    and an untouched output area for the rejected ones, the plaintext for the others -- through dev_decode_records (dx_off: on the
    bulk kernel, k_rec_verify16 + k_decode_rec, where a call this small would take the few-block path) and as the decode side of
    dev_duplex_records (9 + 35 blocks), with identical status arrays; without block checksums everything decodes."""
    import torch
    if dx_off:
        monkeypatch.setenv("PLZ4HIP_DX_MAX_BLOCKS", "0")
    dev = torch.device("cuda:0")
    recs, want_st = _damaged(records35)
    assert any(r[3] & 0x80 for i, r in enumerate(recs) if want_st[i] == 0)                        # a stored record that is good
    nb = 35
    off = np.zeros(nb + 1, dtype=np.int64); off[1:] = np.cumsum([r.size for r in recs])
    d_body = torch.from_numpy(np.concatenate(recs)).to(dev); d_off = torch.from_numpy(off).to(dev)
    s = torch.cuda.current_stream().cuda_stream

    def fresh():
        return (torch.full((nb * K64,), 0xA5, dtype=torch.uint8, device=dev), torch.full((nb,), -9, dtype=torch.int32, device=dev),
                torch.full((nb,), -9, dtype=torch.int32, device=dev))

    def check(d_out, d_res, d_st, untouched=True):
        torch.cuda.synchronize()
        out = d_out.cpu().numpy(); res = d_res.cpu().numpy(); st = d_st.cpu().numpy()
        assert np.array_equal(st, want_st)
        for i in range(nb):
            area = out[i * K64:(i + 1) * K64]
            if want_st[i]:
                assert res[i] == 0 and (not untouched or (area == 0xA5).all()), i
            else:
                assert res[i] == K64 and np.array_equal(area, blocks35[i]), i
        return st

    d_out, d_res, d_st = fresh()
    eng.dev_decode_records(d_body.data_ptr(), d_off.data_ptr(), nb, K64, True, d_out.data_ptr(), K64, K64, d_res.data_ptr(), d_st.data_ptr(), s)
    # (a call this small takes the few-block decoder unless dx_off: that path -- not this file's subject -- decodes beside its
    # checksum kernel and answers a mismatch with status and result alone, so the untouched area is the bulk kernels' property)
    st_plain = check(d_out, d_res, d_st, untouched=dx_off)
    # the decode side of the duplex call, beside the encode of nine blocks
    srcA = np.concatenate(blocks35[:9])
    stride = eng.stage_stride(K64)
    d_src = torch.from_numpy(srcA).to(dev)
    d_stage = torch.zeros(9 * stride, dtype=torch.uint8, device=dev); d_len = torch.zeros(9, dtype=torch.int32, device=dev)
    d_out, d_res, d_st = fresh()
    eng.dev_duplex_records(d_src.data_ptr(), srcA.size, K64, True, d_stage.data_ptr(), d_len.data_ptr(),
                           d_body.data_ptr(), d_off.data_ptr(), nb, K64, True, d_out.data_ptr(), K64, K64, d_res.data_ptr(), d_st.data_ptr(), s)
    st_duplex = check(d_out, d_res, d_st)
    assert np.array_equal(st_plain, st_duplex)
    lens = d_len.cpu().numpy(); stage = d_stage.cpu().numpy()
    for i in range(9):
        assert np.array_equal(stage[i * stride:i * stride + int(lens[i])], records35[i]), i
    # the decode side alone (an empty encode side)
    d_out, d_res, d_st = fresh()
    eng.dev_duplex_records(d_src.data_ptr(), 0, K64, True, d_stage.data_ptr(), d_len.data_ptr(),
                           d_body.data_ptr(), d_off.data_ptr(), nb, K64, True, d_out.data_ptr(), K64, K64, d_res.data_ptr(), d_st.data_ptr(), s)
    check(d_out, d_res, d_st)
    # block checksums off: records without the trailing word, the flipped payload bytes are not looked at by anyone -- all decode
    plain = [orc.block_record(b, K64, False) for b in blocks35]
    offp = np.zeros(nb + 1, dtype=np.int64); offp[1:] = np.cumsum([r.size for r in plain])
    d_bodyp = torch.from_numpy(np.concatenate(plain)).to(dev); d_offp = torch.from_numpy(offp).to(dev)
    d_out, d_res, d_st = fresh()
    eng.dev_decode_records(d_bodyp.data_ptr(), d_offp.data_ptr(), nb, K64, False, d_out.data_ptr(), K64, K64, d_res.data_ptr(), d_st.data_ptr(), s)
    torch.cuda.synchronize()
    assert int(d_st.abs().sum().item()) == 0 and np.array_equal(d_out.cpu().numpy(), np.concatenate(blocks35))


def test_one_long_record_beside_fifteen_short_ones(orc, eng, blocks35, monkeypatch):
    """(iv) one 4 MiB T record beside fifteen 64 KiB ones in a single verify wave: statuses OK, round trip exact"""
    import torch
    monkeypatch.setenv("PLZ4HIP_DX_MAX_BLOCKS", "0")                                              # the bulk kernels
    dev = torch.device("cuda:0")
    bsz = 4 << 20
    srcs = [b for b in blocks35[:16]]
    srcs[5] = synth.make("T", bsz, bsz)
    recs = [orc.block_record(b, bsz, True) for b in srcs]
    got = eng.encode_records(srcs, bsz, True)                                                     # one finish wave over the same sixteen
    for i, (r, w) in enumerate(zip(got, recs)):
        assert np.array_equal(r, w), i
    nb = 16
    off = np.zeros(nb + 1, dtype=np.int64); off[1:] = np.cumsum([r.size for r in recs])
    d_body = torch.from_numpy(np.concatenate(recs)).to(dev); d_off = torch.from_numpy(off).to(dev)
    d_out = torch.full((nb * bsz,), 0xA5, dtype=torch.uint8, device=dev)
    d_res = torch.full((nb,), -9, dtype=torch.int32, device=dev); d_st = torch.full((nb,), -9, dtype=torch.int32, device=dev)
    eng.dev_decode_records(d_body.data_ptr(), d_off.data_ptr(), nb, bsz, True, d_out.data_ptr(), bsz, bsz, d_res.data_ptr(), d_st.data_ptr(),
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert int(d_st.abs().sum().item()) == 0
    res = d_res.cpu().numpy(); out = d_out.cpu().numpy()
    for i, b in enumerate(srcs):
        assert res[i] == b.size and np.array_equal(out[i * bsz:i * bsz + b.size], b), i
