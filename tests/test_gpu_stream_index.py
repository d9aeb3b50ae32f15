"""plz4hip_dev_index_stream on the GPU (k_index_stream): the index of a whole LZ4 stream that is already in device memory.  Expected
values: the model of the header's table of steps in stream_index_cases.py, the offsets this engine's own encoders laid the records
out with, and a decode frame by frame."""
import functools

import numpy as np
import pytest

import body_index_cases as bic
import stream_index_cases as sic
from plz4_amd import synth

pytestmark = pytest.mark.gpu

K64 = 64 << 10
GUARD = 0x5A5A5A5A5A5A5A5A
CANARY = 0xC7
BLK_OK, BLK_SIZE_OVERFLOW = 0, 2


@pytest.fixture(scope="module")
def eng():
    from plz4_amd._native import Engine
    e = Engine(0)
    yield e
    e.close()


def dev_index(eng, d_bytes, n_bytes, max_frames, max_recs):
    """-> (frames, recOff[0 .. max_recs], info) as the model gives them, with the guard words around all three outputs and the
    canary in the entries behind nFrames checked"""
    import torch
    dev = torch.device("cuda:0")
    d_tab = torch.full(((max_frames + 2) * 64,), CANARY, dtype=torch.uint8, device=dev)
    d_off = torch.full((max_recs + 1 + 16,), GUARD, dtype=torch.int64, device=dev)
    d_info = torch.full((32 * 3,), CANARY, dtype=torch.uint8, device=dev)
    eng.dev_index_stream(d_bytes.data_ptr() if d_bytes is not None else None, n_bytes, max_frames, max_recs,
                         d_tab.data_ptr() + 64 if max_frames else None, d_off.data_ptr() + 8 * 8, d_info.data_ptr() + 32,
                         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    tab = d_tab.cpu().numpy(); off = d_off.cpu().numpy(); inf = d_info.cpu().numpy()
    assert (off[:8] == GUARD).all() and (off[8 + max_recs + 1:] == GUARD).all(), "a store outside recOff[0 .. maxRecs]"
    assert (inf[:32] == CANARY).all() and (inf[64:] == CANARY).all(), "a store outside info"
    info = sic.info_of(inf[32:64].view(sic.INFO_DTYPE)[0])
    nf = info["nFrames"]
    assert 0 <= nf <= max_frames
    assert (tab[:64] == CANARY).all() and (tab[64 * (1 + nf):] == CANARY).all(), "a store behind frames[nFrames) or in front of the table"
    return sic.frames_of(tab[64:64 * (1 + max_frames)].view(sic.FRAME_DTYPE), nf), off[8:8 + max_recs + 1].copy(), info


def check_against_model(eng, read, d_bytes, n_bytes, max_frames, max_recs, what):
    want = sic.model(read, n_bytes, max_frames, max_recs)
    got = dev_index(eng, d_bytes, n_bytes, max_frames, max_recs)
    assert got[2] == want[2], (what, got[2], want[2])
    assert got[0] == want[0], (what, [(g, w) for g, w in zip(got[0], want[0]) if g != w][:1])
    assert np.array_equal(got[1], want[1]), what
    return got


# ---------------------------------------------------------------------------------------------------- 1. the case list
def test_the_cases(eng, orc):
    """every case of stream_index_cases.cases on the kernel: with room for everything and with tables of exactly what the stream
    holds, and with the sizes a case names (n - 1, n, n + 1 and 0 of either table)"""
    import torch
    seen = set()
    for c in sic.cases(orc):
        s = c.stream
        # (exactly nBytes bytes on the device: what lies behind a cut is not there for the walk to find)
        d_bytes = torch.from_numpy(s.copy()).to("cuda:0") if s.size else None
        frames, _, info = sic.model(sic.reader_of(s), s.size, *sic.ROOMY)
        for mf, mr in sic.sizes_of(c, frames, info)[:2 if c.sizes is None else None]:
            seen.add(check_against_model(eng, sic.reader_of(s), d_bytes, s.size, mf, mr, (c.name, mf, mr))[2]["status"])
    assert seen == set(range(12))


# ---------------------------------------------------------------------------------------------------- 2. no host sync
@functools.lru_cache(maxsize=None)
def plaintext(n_bytes: int, seed: int) -> np.ndarray:
    """text with one incompressible block of 64 KiB in it (if there is room): its record is a stored one"""
    data = synth.text(n_bytes, seed=seed)
    if n_bytes >= 3 * K64:
        data[K64:2 * K64] = synth.random_bytes(K64, seed=seed)
    data.setflags(write=False)
    return data


def encode_frame(eng, orc, data, linked=False, content_checksum=True):
    """a whole frame around the block section this engine's encoder writes for `data` (64 KiB blocks, block checksums):
    -> (frame on the host, the encoder's recOff relative to the frame's first byte)"""
    import torch
    dev = torch.device("cuda:0")
    n = (data.size + K64 - 1) // K64
    PAD = K64
    d_src = torch.zeros(PAD + data.size, dtype=torch.uint8, device=dev)
    d_src[PAD:] = torch.from_numpy(np.array(data)).to(dev)
    d_body = torch.zeros(n * (K64 + 8), dtype=torch.uint8, device=dev)
    d_off = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    d_len = torch.zeros(n, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    if linked:
        eng.dev_encode_body_ex(d_src.data_ptr() + PAD, data.size, K64, K64, True, d_body.data_ptr(), d_body.numel(), d_off.data_ptr(),
                               d_len.data_ptr(), linked=True, stream=s)
    else:
        eng.dev_encode_body(d_src.data_ptr() + PAD, data.size, K64, True, d_body.data_ptr(), d_body.numel(), d_off.data_ptr(), d_len.data_ptr(), s)
    torch.cuda.synchronize()
    off = d_off.cpu().numpy()
    body = d_body.cpu().numpy()[:int(off[n])]
    hdr = sic.u8(orc.frame_header(4, linked=linked, block_checksum=True, content_checksum=content_checksum))
    tail = [bic.le32(0)] + ([bic.le32(orc.xxh32(data))] if content_checksum else [])
    return np.concatenate([hdr, body] + tail), off + hdr.size


@pytest.mark.parametrize("route,sizes", [("few blocks", (5 * K64 - 1000, 777, 9 * K64)), ("bulk", (65 * K64 - 5, K64, 64 * K64))])
def test_index_then_one_decode_without_a_host_sync(eng, orc, route, sizes):
    """a stream of three frames with block checksums, a skippable frame in front and between; index with upper bounds and ONE
    plz4hip_dev_decode_records of maxRecs records over the global recOff, one behind the other on one stream, one synchronisation.
    A frame's last record is followed by end mark, content checksum, perhaps a skippable frame and the next header before the next
    entry of recOff: the decoders take that distance as a bound only, so plaintext, results and statuses are those of a decode frame
    by frame; the padded tail is PLZ4HIP_BLK_SIZE_OVERFLOW, result 0, its output untouched.  15 records in 85 entries: the
    few-block decoder's call; 130 in 200: the bulk kernels."""
    import torch
    dev = torch.device("cuda:0")
    datas = [plaintext(n, 11 + k) for k, n in enumerate(sizes)]
    built = [encode_frame(eng, orc, d, content_checksum=bool(k != 1)) for k, d in enumerate(datas)]
    parts, where = [sic.skippable(4, 13)], []
    for k, (f, _) in enumerate(built):
        where.append(sum(p.size for p in parts))
        parts.append(f)
        if k == 0:
            parts.append(sic.skippable(9, 1001))
    stream = np.concatenate(parts)
    counts = [(d.size + K64 - 1) // K64 for d in datas]
    n = sum(counts); mr = n + 70; mf = 10
    assert (n <= 128 and mr <= 128) if route == "few blocks" else n > 128
    d_bytes = torch.from_numpy(stream).to(dev)
    d_tab = torch.zeros(mf * 64, dtype=torch.uint8, device=dev)
    d_off = torch.full((mr + 1,), -1, dtype=torch.int64, device=dev)
    d_info = torch.zeros(32, dtype=torch.uint8, device=dev)
    d_out = torch.full((mr * K64,), 0xA5, dtype=torch.uint8, device=dev)
    d_res = torch.full((mr,), -9, dtype=torch.int32, device=dev); d_st = torch.full((mr,), -9, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    eng.dev_index_stream(d_bytes.data_ptr(), stream.size, mf, mr, d_tab.data_ptr(), d_off.data_ptr(), d_info.data_ptr(), s)
    eng.dev_decode_records(d_bytes.data_ptr(), d_off.data_ptr(), mr, K64, True, d_out.data_ptr(), K64, K64, d_res.data_ptr(), d_st.data_ptr(), s)
    torch.cuda.synchronize()
    info = sic.info_of(d_info.cpu().numpy().view(sic.INFO_DTYPE)[0])
    assert info == dict(end=stream.size, nFrames=5, nRecs=n, status=sic.END, nSkippable=2, maxBsz=K64, flagsAnd=0x70, flagsOr=0x74)
    frames = sic.frames_of(d_tab.cpu().numpy().view(sic.FRAME_DTYPE), 5)
    lz4 = [f for f in frames if f["kind"] == 0]
    rec_off = d_off.cpu().numpy()
    want_off = np.concatenate([enc[:-1] + at for (_, enc), at in zip(built, where)])
    assert np.array_equal(rec_off[:n], want_off) and (rec_off[n:] == built[2][1][-1] + where[2]).all()
    assert [(f["hdrOff"], f["firstRec"], f["nRecs"]) for f in lz4] == [(at, first, c) for at, first, c in zip(where, np.cumsum([0] + counts), counts)]
    assert [f["contentSum"] for f in lz4] == [orc.xxh32(datas[0]), 0, orc.xxh32(datas[2])]
    res = d_res.cpu().numpy(); st = d_st.cpu().numpy(); out = d_out.cpu().numpy()
    # the decode frame by frame: each frame's own bytes, its own recOff of exactly its records
    for f, (raw, enc), data, c in zip(lz4, built, datas, counts):
        d_f = torch.from_numpy(raw).to(dev); d_o = torch.from_numpy(enc).to(dev)
        d_out1 = torch.full((c * K64,), 0xA5, dtype=torch.uint8, device=dev)
        d_res1 = torch.full((c,), -9, dtype=torch.int32, device=dev); d_st1 = torch.full((c,), -9, dtype=torch.int32, device=dev)
        eng.dev_decode_records(d_f.data_ptr(), d_o.data_ptr(), c, K64, True, d_out1.data_ptr(), K64, K64, d_res1.data_ptr(), d_st1.data_ptr(), s)
        torch.cuda.synchronize()
        a = f["firstRec"]
        assert np.array_equal(st[a:a + c], d_st1.cpu().numpy()) and (st[a:a + c] == BLK_OK).all(), (route, a)
        assert np.array_equal(res[a:a + c], d_res1.cpu().numpy()) and int(res[a:a + c].sum()) == data.size
        assert np.array_equal(out[a * K64:(a + c) * K64], d_out1.cpu().numpy())
        assert np.array_equal(out[a * K64:a * K64 + data.size], data)
    assert (st[n:] == BLK_SIZE_OVERFLOW).all() and (res[n:] == 0).all() and (out[n * K64:] == 0xA5).all()


def test_linked_frames_take_first_rec_as_chain_first(eng, orc):
    """two linked frames (FLG bit 5 clear) of 3 and 4 blocks, a skippable frame between: the entries' firstRec, read on the host,
    are the chainFirst of plz4hip_dev_decode_records_ex over the global recOff"""
    import torch
    dev = torch.device("cuda:0")
    datas = [plaintext(3 * K64, 21), plaintext(4 * K64, 22)]
    built = [encode_frame(eng, orc, d, linked=True) for d in datas]
    stream = np.concatenate([built[0][0], sic.skippable(0, 40), built[1][0]])
    d_bytes = torch.from_numpy(stream).to(dev)
    frames, rec_off, info = check_against_model(eng, sic.reader_of(stream), d_bytes, stream.size, 3, 7, "linked")
    lz4 = [f for f in frames if f["kind"] == 0]
    assert info["status"] == sic.END and info["nRecs"] == 7 and not info["flagsOr"] & 0x20 and [f["firstRec"] for f in lz4] == [0, 3]
    n = info["nRecs"]
    cap = K64 + 8; stride = (cap + 64 + 15) // 16 * 16
    d_off = torch.from_numpy(rec_off).to(dev)
    d_out = torch.full((n * stride,), 0xA5, dtype=torch.uint8, device=dev)
    d_res = torch.full((n,), -9, dtype=torch.int32, device=dev); d_st = torch.full((n,), -9, dtype=torch.int32, device=dev)
    d_w = torch.zeros(2 * 131072, dtype=torch.uint8, device=dev); d_wl = torch.zeros(2, dtype=torch.int32, device=dev)
    eng.dev_decode_records_ex(d_bytes.data_ptr(), d_off.data_ptr(), n, K64, True, d_out.data_ptr(), stride, cap, d_res.data_ptr(), d_st.data_ptr(),
                              linked=True, chain_first=[f["firstRec"] for f in lz4] + [n], windows_ptr=d_w.data_ptr(), window_len_ptr=d_wl.data_ptr(),
                              stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().reshape(n, stride)
    assert (d_st.cpu().numpy() == BLK_OK).all() and (d_res.cpu().numpy() == K64).all()
    assert np.array_equal(out[:, :K64].reshape(-1), np.concatenate(datas))


# ---------------------------------------------------------------------------------------------------- 3. beyond 4 GiB
def test_sparse_stream_beyond_4_gib(eng, orc):
    """5.5 GiB of torch.empty: a small frame at each end, joined by two skippable frames of 3 GiB and 2.5 GiB whose payload nobody
    wrote or reads: offsets beyond 2^32 are exact; then one byte short of the second skippable frame's end"""
    import torch
    dev = torch.device("cuda:0")
    a, b = sic.made_frame(orc, 3, 4, bck=True, cck=True, seed=5), sic.made_frame(orc, 2, 7, cck=True, seed=6)
    s1, s2 = 3 << 30, (5 << 29) + 13
    at_s1, at_s2, at_b = a.size, a.size + 8 + s1, a.size + 16 + s1 + s2
    total = at_b + b.size
    assert total > (11 << 29) and at_s2 < 1 << 32 < at_b
    pieces = {0: a, at_s1: np.concatenate([bic.le32(0x184D2A5C), bic.le32(s1)]), at_s2: np.concatenate([bic.le32(0x184D2A51), bic.le32(s2)]), at_b: b}
    d_bytes = torch.empty(total, dtype=torch.uint8, device=dev)
    for at, p in pieces.items():
        d_bytes[at:at + p.size] = torch.from_numpy(p.copy()).to(dev)

    def read(off, n):                                          # (the model asks for header bytes, size words and trailers only)
        for at, p in pieces.items():
            if at <= off and off + n <= at + p.size:
                return bytes(p[off - at:off - at + n])
        raise AssertionError("the model reads a byte nobody wrote: %d" % off)

    for mf, mr in ((4, 5), (6, 80), (3, 5), (4, 4)):
        check_against_model(eng, read, d_bytes, total, mf, mr, ("sparse", mf, mr))
    frames, rec_off, info = check_against_model(eng, read, d_bytes, total, 4, 5, "sparse")
    assert (info["status"], info["end"], info["nFrames"], info["nSkippable"], info["nRecs"]) == (sic.END, total, 4, 2, 5)
    assert [(f["kind"], f["nibble"], f["hdrOff"], f["contentSz"]) for f in frames[1:3]] == [(1, 12, at_s1, s1), (1, 1, at_s2, s2)]
    assert frames[3]["hdrOff"] == at_b and frames[3]["firstRec"] == 3 and rec_off[3] == at_b + 7 and frames[3]["end"] == total
    frames, rec_off, info = check_against_model(eng, read, d_bytes, at_b - 1, 4, 5, "sparse, one byte short")
    assert (info["status"], info["end"], info["nFrames"]) == (sic.SKIP, at_s2, 2)
    del d_bytes
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------- 4. arguments
def test_bad_arguments(eng):
    import torch
    from plz4_amd._native import EngineError
    buf = torch.zeros(128, dtype=torch.int64, device="cuda:0")
    p = buf.data_ptr()
    good = dict(bytes_ptr=p, n_bytes=16, max_frames=2, max_recs=4, frames_ptr=p + 128, recoff_ptr=p + 512, info_ptr=p + 768)
    for kw in (dict(bytes_ptr=None), dict(n_bytes=-1), dict(max_frames=-1), dict(frames_ptr=None), dict(max_recs=-1), dict(max_recs=0x7FFFFFFF),
               dict(recoff_ptr=None), dict(info_ptr=None)):
        with pytest.raises(EngineError) as ei:
            eng.dev_index_stream(**dict(good, **kw))
        assert ei.value.code == -1, kw
    # an empty stream may be null, and so may the table when it has no entries
    eng.dev_index_stream(**dict(good, bytes_ptr=None, n_bytes=0, frames_ptr=None, max_frames=0))
    torch.cuda.synchronize()
    info = sic.info_of(buf[96:100].cpu().numpy().view(sic.INFO_DTYPE)[0])
    assert info == dict(end=0, nFrames=0, nRecs=0, status=sic.END, nSkippable=0, maxBsz=0, flagsAnd=0, flagsOr=0)
