"""plz4hip_dev_index_body / plz4hip_mgpu_dev_index_frame on the GPU (k_index_body): the index of a frame body that is already in
device memory.  Expected values: the recOff plz4hip_dev_encode_body itself returns, the oracle's frames, and the model of
FrameReader._read's walk in body_index_cases.py."""
import functools

import numpy as np
import pytest

import body_index_cases as bic
from plz4_amd import synth

pytestmark = pytest.mark.gpu

K64 = 64 << 10
GUARD = 0x5A5A5A5A5A5A5A5A
BLK_OK, BLK_SIZE_OVERFLOW, BLK_CORRUPT = 0, 2, 3


@pytest.fixture(scope="module")
def eng():
    from plz4_amd._native import Engine
    e = Engine(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def plaintext(n: int, random_at: int) -> np.ndarray:
    """n blocks of 64 KiB of text, block `random_at` (if any) incompressible: its record is a stored one"""
    data = synth.text(n * K64, seed=n)
    if 0 <= random_at < n:
        data[random_at * K64:(random_at + 1) * K64] = synth.random_bytes(K64, seed=n)
    data.setflags(write=False)
    return data


_encoded = {}


def encoded(eng, n, checksum, random_at):
    """(plaintext, body on the host, the encoder's recOff) of plz4hip_dev_encode_body at bsz 65536, encoded once per case"""
    import torch
    key = (n, checksum, random_at)
    if key not in _encoded:
        dev = torch.device("cuda:0")
        data = plaintext(n, random_at)
        d_src = torch.from_numpy(np.array(data)).to(dev)
        d_body = torch.zeros(n * (K64 + 8), dtype=torch.uint8, device=dev)
        d_off = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
        d_len = torch.zeros(n, dtype=torch.int32, device=dev)
        eng.dev_encode_body(d_src.data_ptr(), data.size, K64, checksum, d_body.data_ptr(), d_body.numel(), d_off.data_ptr(), d_len.data_ptr(),
                            torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        off = d_off.cpu().numpy()
        body = d_body.cpu().numpy()[:int(off[n])].copy()
        if 0 <= random_at < n:
            assert body[int(off[random_at]) + 3] & 0x80                                     # (a stored record is among them)
        _encoded[key] = (data, body, off)
    return _encoded[key]


def dev_index(eng, d_body, body_bytes, bsz, checksum, max_blocks):
    """-> (recOff[0 .. max_blocks], end, nBlocks, status) with the guard words around both arrays checked"""
    import torch
    dev = torch.device("cuda:0")
    d_off = torch.full((max_blocks + 1 + 16,), GUARD, dtype=torch.int64, device=dev)
    d_info = torch.full((2 + 8,), GUARD, dtype=torch.int64, device=dev)                     # info: 16 bytes at [4, 6)
    eng.dev_index_body(d_body.data_ptr() if d_body is not None else None, body_bytes, bsz, checksum, max_blocks,
                       d_off.data_ptr() + 8 * 8, d_info.data_ptr() + 4 * 8, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    off = d_off.cpu().numpy(); info = d_info.cpu().numpy()
    assert (off[:8] == GUARD).all() and (off[8 + max_blocks + 1:] == GUARD).all(), "a store outside recOff[0 .. maxBlocks]"
    assert (info[:4] == GUARD).all() and (info[6:] == GUARD).all(), "a store outside info"
    nb, status = (int(x) for x in info[5:6].view(np.int32))
    return off[8:8 + max_blocks + 1].copy(), int(info[4]), nb, status


def check_against_model(eng, body, body_bytes, bsz, checksum, max_blocks, what, d_body=None):
    import torch
    if d_body is None:
        # the body ends where its allocation's used bytes end: nothing behind it belongs to the walk
        d_body = torch.from_numpy(body[:body_bytes].copy()).to("cuda:0") if body_bytes else None
    want = bic.model(bic.word_of(body), body_bytes, bsz, checksum, max_blocks)
    got = dev_index(eng, d_body, body_bytes, bsz, checksum, max_blocks)
    assert np.array_equal(got[0], want[0]), what
    assert got[1:] == want[1:], (what, got[1:], want[1:])
    return got


# ---------------------------------------------------------------------------------------------------- 1. well-formed bodies
@pytest.mark.parametrize("checksum", [False, True])
@pytest.mark.parametrize("n", [1, 64, 65, 130])
def test_index_reproduces_the_encoders_offsets(eng, n, checksum):
    """the body plz4hip_dev_encode_body wrote, as it is and with an end mark (and four more bytes) appended: recOff and nBlocks are
    the encoder's, end and status the model's.  One block: a text block and an incompressible one, each a body of its own."""
    for random_at in ((-1, 0) if n == 1 else (n // 2,)):
        data, body, enc_off = encoded(eng, n, checksum, random_at)
        marked = np.concatenate([body, np.zeros(4, np.uint8), np.full(4, 0x77, np.uint8)])
        for mb in (n, n + 70):
            off, end, nb, status = check_against_model(eng, body, body.size, K64, checksum, mb, (n, checksum, mb))
            assert nb == n and np.array_equal(off[:n + 1], enc_off) and (off[n:] == enc_off[n]).all()
            assert status == bic.END_OF_BYTES and end == body.size
            off, end, nb, status = check_against_model(eng, marked, marked.size, K64, checksum, mb, (n, checksum, mb, "end mark"))
            assert nb == n and np.array_equal(off[:n + 1], enc_off) and (off[n:] == enc_off[n]).all()
            assert status == bic.END_MARK and end == body.size + 4
        if n > 1:
            off, end, nb, status = check_against_model(eng, body, body.size, K64, checksum, n - 1, (n, checksum, "full"))
            assert nb == n - 1 and status == bic.FULL and end == enc_off[n - 1] and np.array_equal(off, enc_off[:n])


# ---------------------------------------------------------------------------------------------------- 2. no host sync
@pytest.mark.parametrize("checksum", [False, True])
@pytest.mark.parametrize("n", [9, 65])
def test_index_then_decode_without_a_host_sync(eng, n, checksum):
    """index with maxBlocks = n + 70 and plz4hip_dev_decode_records of maxBlocks records, one behind the other on one stream: the
    first n blocks decode, the padded tail is PLZ4HIP_BLK_SIZE_OVERFLOW, result 0, its output untouched (n = 9: the few-block
    decoder's call; n = 65: 135 records, the bulk kernels)"""
    import torch
    dev = torch.device("cuda:0")
    data, body, enc_off = encoded(eng, n, checksum, n // 2)
    mb = n + 70
    d_body = torch.from_numpy(body).to(dev)
    d_off = torch.full((mb + 1,), -1, dtype=torch.int64, device=dev)
    d_info = torch.full((2,), -1, dtype=torch.int64, device=dev)
    d_out = torch.full((mb * K64,), 0xA5, dtype=torch.uint8, device=dev)
    d_res = torch.full((mb,), -9, dtype=torch.int32, device=dev); d_st = torch.full((mb,), -9, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    eng.dev_index_body(d_body.data_ptr(), body.size, K64, checksum, mb, d_off.data_ptr(), d_info.data_ptr(), s)
    eng.dev_decode_records(d_body.data_ptr(), d_off.data_ptr(), mb, K64, checksum, d_out.data_ptr(), K64, K64, d_res.data_ptr(), d_st.data_ptr(), s)
    torch.cuda.synchronize()
    info = d_info.cpu().numpy()
    assert int(info[0]) == body.size and tuple(int(x) for x in info[1:2].view(np.int32)) == (n, bic.END_OF_BYTES)
    res = d_res.cpu().numpy(); st = d_st.cpu().numpy(); out = d_out.cpu().numpy()
    assert (st[:n] == BLK_OK).all() and (res[:n] == K64).all() and np.array_equal(out[:n * K64], data)
    assert (st[n:] == BLK_SIZE_OVERFLOW).all() and (res[n:] == 0).all() and (out[n * K64:] == 0xA5).all()


def test_index_then_linked_decode_without_a_host_sync(eng):
    """the same for a linked frame of 8 blocks, one chain, through plz4hip_dev_decode_records_ex.  The first padded record is
    PLZ4HIP_BLK_SIZE_OVERFLOW; behind a bad record the chain decoder answers every later record of the chain with
    PLZ4HIP_BLK_CORRUPT (include/plz4hip.h, B'); result 0 and an untouched output for all of them."""
    import torch
    dev = torch.device("cuda:0")
    n, mb, PAD = 8, 78, 65536
    data = plaintext(n, 3)
    d_src = torch.zeros(PAD + data.size, dtype=torch.uint8, device=dev)
    d_src[PAD:] = torch.from_numpy(np.array(data)).to(dev)
    cap_body = n * (K64 + 8)
    d_body = torch.zeros(cap_body, dtype=torch.uint8, device=dev)
    d_eoff = torch.full((n + 1,), -1, dtype=torch.int64, device=dev); d_len = torch.zeros(n, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    eng.dev_encode_body_ex(d_src.data_ptr() + PAD, data.size, K64, K64, True, d_body.data_ptr(), cap_body, d_eoff.data_ptr(), d_len.data_ptr(),
                           linked=True, stream=s)
    torch.cuda.synchronize()
    enc_off = d_eoff.cpu().numpy(); body_bytes = int(enc_off[n])
    cap = K64 + 8; stride = (cap + 64 + 15) // 16 * 16
    d_off = torch.full((mb + 1,), -1, dtype=torch.int64, device=dev)
    d_info = torch.full((2,), -1, dtype=torch.int64, device=dev)
    d_out = torch.full((mb * stride,), 0xA5, dtype=torch.uint8, device=dev)
    d_res = torch.full((mb,), -9, dtype=torch.int32, device=dev); d_st = torch.full((mb,), -9, dtype=torch.int32, device=dev)
    d_w = torch.zeros(131072, dtype=torch.uint8, device=dev); d_wl = torch.zeros(1, dtype=torch.int32, device=dev)
    eng.dev_index_body(d_body.data_ptr(), body_bytes, K64, True, mb, d_off.data_ptr(), d_info.data_ptr(), s)
    eng.dev_decode_records_ex(d_body.data_ptr(), d_off.data_ptr(), mb, K64, True, d_out.data_ptr(), stride, cap, d_res.data_ptr(), d_st.data_ptr(),
                              linked=True, windows_ptr=d_w.data_ptr(), window_len_ptr=d_wl.data_ptr(), stream=s)
    torch.cuda.synchronize()
    info = d_info.cpu().numpy()
    assert int(info[0]) == body_bytes and tuple(int(x) for x in info[1:2].view(np.int32)) == (n, bic.END_OF_BYTES)
    assert np.array_equal(d_off.cpu().numpy()[:n + 1], enc_off)
    res = d_res.cpu().numpy(); st = d_st.cpu().numpy(); out = d_out.cpu().numpy().reshape(mb, stride)
    assert (st[:n] == BLK_OK).all() and (res[:n] == K64).all() and np.array_equal(out[:n, :K64].reshape(-1), data)
    assert st[n] == BLK_SIZE_OVERFLOW and (st[n + 1:] == BLK_CORRUPT).all() and (res[n:] == 0).all() and (out[n:] == 0xA5).all()


# ---------------------------------------------------------------------------------------------------- 3. hostile words
@pytest.mark.parametrize("checksum", [False, True])
@pytest.mark.parametrize("bsz", bic.BSZS)
def test_hostile_bodies(eng, bsz, checksum):
    """bodies of 0..3 bytes, the last 12 cuts, lying size words: recOff, info and the guard words around both"""
    import torch
    seen = set()
    for name, body, body_bytes in bic.hostile(bsz, checksum):
        # (exactly bodyBytes bytes on the device: what lies behind a cut is not there for the walk to find)
        d_body = torch.from_numpy(body[:body_bytes].copy()).to("cuda:0") if body_bytes else None
        for mb in (0, 5, 80):
            seen.add(check_against_model(eng, body, body_bytes, bsz, checksum, mb, (name, mb), d_body=d_body)[3])
    assert seen == {bic.END_MARK, bic.END_OF_BYTES, bic.FULL, bic.SIZE_OVERFLOW, bic.TRUNCATED_WORD, bic.TRUNCATED_BLOCK}


def test_bad_arguments(eng):
    import torch
    from plz4_amd._native import EngineError
    buf = torch.zeros(64, dtype=torch.int64, device="cuda:0")
    p = buf.data_ptr()
    good = dict(body_ptr=p, body_bytes=16, bsz=1024, block_checksum=False, max_blocks=4, recoff_ptr=p + 64, info_ptr=p + 256)
    for kw in (dict(body_ptr=None), dict(body_bytes=-1), dict(bsz=0), dict(max_blocks=-1), dict(max_blocks=0x7FFFFFFF), dict(recoff_ptr=None),
               dict(info_ptr=None)):
        with pytest.raises(EngineError) as ei:
            eng.dev_index_body(**dict(good, **kw))
        assert ei.value.code == -1, kw
    eng.dev_index_body(**dict(good, body_ptr=None, body_bytes=0))                         # an empty body may be null
    torch.cuda.synchronize()
    assert int(buf[32]) == 0 and tuple(int(x) for x in buf[33:34].cpu().numpy().view(np.int32)) == (0, bic.END_OF_BYTES)


# ---------------------------------------------------------------------------------------------------- 4. beyond 4 GiB
def test_sparse_body_beyond_4_gib(eng):
    """five records of nominal bsz 0x7FFFFFFF, about 1.1 GiB each, in 5.5 GiB of torch.empty that holds their size words and
    nothing else that matters: offsets beyond 2^32 are exact"""
    import torch
    dev = torch.device("cuda:0")
    bsz = 0x7FFFFFFF
    sizes = [0x46000000 + 13 * k for k in range(5)]
    want_off = np.concatenate([[0], np.cumsum([4 + s for s in sizes])]).astype(np.int64)
    total = int(want_off[5])
    assert total > 5 << 30 and want_off[4] > 1 << 32
    d_body = torch.empty(total, dtype=torch.uint8, device=dev)
    words = {}
    for k, s in enumerate(sizes):
        w = s | (0x80000000 if k == 2 else 0)
        words[int(want_off[k])] = w
        d_body[int(want_off[k]):int(want_off[k]) + 4] = torch.from_numpy(bic.le32(w).copy()).to(dev)
    for mb in (4, 5, 70):
        want = bic.model(lambda o: words[o], total, bsz, False, mb)
        got = dev_index(eng, d_body, total, bsz, False, mb)
        assert np.array_equal(got[0], want[0]) and got[1:] == want[1:]
        k = min(mb, 5)
        assert np.array_equal(got[0][:k + 1], want_off[:k + 1]) and got[2] == k and got[3] == (bic.FULL if mb < 5 else bic.END_OF_BYTES)
    got = dev_index(eng, d_body, total - 1, bsz, False, 8)                                # one byte short, beyond 2^32 on both sides
    assert got[1:] == (int(want_off[4]), 4, bic.TRUNCATED_BLOCK) and (got[0][4:] == want_off[4]).all()
    del d_body
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------- 5. several GPUs
def test_mgpu_index_then_decode_frame(orc):
    """a frame from the oracle's writer, its header skipped, on a handle that lists device 0 twice: index_frame, then
    dev_decode_frame of what it listed == the plaintext; a damaged size word is a status and a clean return"""
    import torch
    from plz4_amd._native import MultiEngine
    dev = torch.device("cuda:0")
    m = MultiEngine([0, 0])
    data = synth.make("M", 8 * K64 + 1234, K64)
    frame = orc.frame_encode(data, 4, True, True)                                         # BD index 4 = 64 KiB; block + content checksums
    hdr = len(orc.frame_header(4, block_checksum=True, content_checksum=True))
    body = np.ascontiguousarray(frame[hdr:])
    d_body = torch.from_numpy(body).to(dev)
    torch.cuda.synchronize()
    off, nb, status, end = m.index_frame(1, d_body.data_ptr(), body.size, K64, True, 9 + 70)
    want = bic.model(bic.word_of(body), body.size, K64, True, 79)
    assert np.array_equal(off, want[0]) and (end, nb, status) == want[1:]
    assert nb == 9 and status == bic.END_MARK and end == body.size - 4                    # (the content checksum starts at `end`)
    blocks = [data[o:o + K64] for o in range(0, data.size, K64)]
    outs = [torch.zeros(len(blocks[k::2]) * K64, dtype=torch.uint8, device=dev) for k in range(2)]
    res, st = m.dev_decode_frame(nb, 1, d_body.data_ptr(), off[:nb + 1], K64, True, [t.data_ptr() for t in outs], K64, K64)
    torch.cuda.synchronize()
    assert int(np.abs(st).sum()) == 0 and [int(r) for r in res] == [b.size for b in blocks]
    for k in range(2):
        got = outs[k].cpu().numpy()
        for j, b in enumerate(blocks[k::2]):
            assert np.array_equal(got[j * K64:j * K64 + b.size], b), (k, j)
    # record 4's size word says bsz + 1
    bad = body.copy()
    bad[int(off[4]):int(off[4]) + 4] = bic.le32(K64 + 1)
    d_bad = torch.from_numpy(bad).to(dev)
    torch.cuda.synchronize()
    off2, nb2, status2, end2 = m.index_frame(0, d_bad.data_ptr(), bad.size, K64, True, 79)
    assert (nb2, status2, end2) == (4, bic.SIZE_OVERFLOW, int(off[4])) and np.array_equal(off2[:5], off[:5]) and (off2[4:] == off[4]).all()
    m.close()
