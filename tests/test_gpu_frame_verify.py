"""plz4hip_dev_verify_frames on the GPU (k_verify_frames, k_verify_summary): the verdict on every frame of a decoded stream that lies
in device memory.  Expected values: the model of the header's table of rules in frame_verify_cases.py, the oracle's xxh32 of the
plaintext, and the plaintext's length."""
import functools
import os

import numpy as np
import pytest

import body_index_cases as bic
import frame_verify_cases as fvc
import stream_index_cases as sic
from plz4_amd import synth

pytestmark = pytest.mark.gpu

K64 = 64 << 10
CANARY = fvc.CANARY
WAVES = "PLZ4HIP_VERIFY_WAVES"


@pytest.fixture(scope="module")
def eng():
    from plz4_amd._native import Engine
    e = Engine(0)
    yield e
    e.close()


def guarded(a: np.ndarray, guard: int = 64):
    """a host array on the device between two guards of canary bytes -> (the whole tensor, the address of the array in it)"""
    import torch
    whole = np.concatenate([np.full(guard, CANARY, np.uint8), np.ascontiguousarray(a).view(np.uint8).reshape(-1), np.full(guard, CANARY, np.uint8)])
    t = torch.from_numpy(whole).to("cuda:0")
    return t, t.data_ptr() + guard


def verify_on_device(eng, frames_ptr, info_ptr, max_frames, dst_ptr, stride, cap, res_ptr, st_ptr, max_recs, waves=None):
    """the call with canaries around verdicts and sv and in the entries behind nFrames -> (verdicts, sv) as the model gives them"""
    import torch
    dev = torch.device("cuda:0")
    d_ver = torch.full(((max_frames + 2) * 32,), CANARY, dtype=torch.uint8, device=dev)
    d_sv = torch.full((32 * 3,), CANARY, dtype=torch.uint8, device=dev)
    old = os.environ.pop(WAVES, None)
    try:
        if waves is not None:
            os.environ[WAVES] = str(waves)                       # (read per call)
        eng.dev_verify_frames(frames_ptr, info_ptr, max_frames, dst_ptr, stride, cap, res_ptr, st_ptr, max_recs,
                              d_ver.data_ptr() + 32, d_sv.data_ptr() + 32, torch.cuda.current_stream().cuda_stream)
    finally:
        os.environ.pop(WAVES, None)
        if old is not None:
            os.environ[WAVES] = old
    torch.cuda.synchronize()
    ver = d_ver.cpu().numpy(); svb = d_sv.cpu().numpy()
    assert (svb[:32] == CANARY).all() and (svb[64:] == CANARY).all(), "a store outside sv"
    sv = fvc.sv_of(svb[32:64].view(fvc.SV_DTYPE)[0])
    nf = sv["nFrames"]
    assert 0 <= nf <= max_frames
    assert (ver[:32] == CANARY).all() and (ver[32 * (1 + nf):] == CANARY).all(), "a store behind verdicts[nFrames) or in front of them"
    return fvc.verdicts_of(ver[32:32 * (1 + max_frames)].view(fvc.VERDICT_DTYPE), nf), sv


# ---------------------------------------------------------------------------------------------------- 1. the case list
def test_the_cases(eng, orc):
    """every case of frame_verify_cases.cases on the kernel, the inputs between guard words that must come back untouched"""
    seen = set()
    for c in fvc.cases(orc):
        want, want_sv = fvc.model(orc, c)
        ins = [guarded(a) for a in (c.frames, c.info, c.dst, c.result, c.status)]
        (_, p_tab), (_, p_info), (_, p_dst), (_, p_res), (_, p_st) = ins
        got, sv = verify_on_device(eng, p_tab, p_info, c.max_frames, p_dst, c.stride, c.cap, p_res, p_st, c.max_recs, c.waves)
        assert sv == want_sv, (c.name, sv, want_sv)
        assert got == want, (c.name, [(j, g, w) for j, (g, w) in enumerate(zip(got, want)) if g != w][:1])
        for (t, _), a in zip(ins, (c.frames, c.info, c.dst, c.result, c.status)):
            back = t.cpu().numpy()
            assert (back[:64] == CANARY).all() and (back[back.size - 64:] == CANARY).all() and \
                np.array_equal(back[64:back.size - 64], np.ascontiguousarray(a).view(np.uint8).reshape(-1)), (c.name, "an input was written")
        seen |= {v["status"] for v in want}
    assert seen == set(range(7))


# ---------------------------------------------------------------------------------------------------- 2. the pipeline
@functools.lru_cache(maxsize=None)
def plaintext(n_bytes: int, seed: int) -> np.ndarray:
    """text with one incompressible block of 64 KiB in it (if there is room): its record is a stored one"""
    data = synth.text(n_bytes, seed=seed)
    if n_bytes >= 3 * K64:
        data[K64:2 * K64] = synth.random_bytes(K64, seed=seed)
    data.setflags(write=False)
    return data


def encode_frame(eng, orc, data, linked=False, content_size=None):
    """a whole frame around the block section this engine's encoder writes for `data` (64 KiB blocks, block checksums, the oracle's
    content checksum) -> (frame on the host, the encoder's recOff relative to the frame's first byte, the header's length)"""
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
    hdr = sic.u8(orc.frame_header(4, linked=linked, block_checksum=True, content_checksum=True, content_size=content_size))
    return np.concatenate([hdr, body, bic.le32(0), bic.le32(orc.xxh32(data))]), off + hdr.size, hdr.size


def index_decode_verify(eng, stream, mf, mr):
    """plz4hip_dev_index_stream, ONE plz4hip_dev_decode_records of maxRecs records and plz4hip_dev_verify_frames one behind the other on
    one stream, one synchronisation -> (info, frames, verdicts, sv, result, status, the plaintext slots)"""
    import torch
    dev = torch.device("cuda:0")
    d_bytes = torch.from_numpy(stream).to(dev)
    d_tab = torch.zeros(mf * 64, dtype=torch.uint8, device=dev)
    d_off = torch.full((mr + 1,), -1, dtype=torch.int64, device=dev)
    d_info = torch.zeros(32, dtype=torch.uint8, device=dev)
    d_out = torch.full((mr * K64,), 0xA5, dtype=torch.uint8, device=dev)
    d_res = torch.full((mr,), -9, dtype=torch.int32, device=dev); d_st = torch.full((mr,), -9, dtype=torch.int32, device=dev)
    d_ver = torch.full((mf * 32,), CANARY, dtype=torch.uint8, device=dev)
    d_sv = torch.full((32,), CANARY, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    eng.dev_index_stream(d_bytes.data_ptr(), stream.size, mf, mr, d_tab.data_ptr(), d_off.data_ptr(), d_info.data_ptr(), s)
    eng.dev_decode_records(d_bytes.data_ptr(), d_off.data_ptr(), mr, K64, True, d_out.data_ptr(), K64, K64, d_res.data_ptr(), d_st.data_ptr(), s)
    eng.dev_verify_frames(d_tab.data_ptr(), d_info.data_ptr(), mf, d_out.data_ptr(), K64, K64, d_res.data_ptr(), d_st.data_ptr(), mr,
                          d_ver.data_ptr(), d_sv.data_ptr(), s)
    torch.cuda.synchronize()
    info = sic.info_of(d_info.cpu().numpy().view(sic.INFO_DTYPE)[0])
    nf = info["nFrames"]
    sv = fvc.sv_of(d_sv.cpu().numpy().view(fvc.SV_DTYPE)[0])
    ver = d_ver.cpu().numpy()
    assert sv["nFrames"] == nf and (ver[32 * nf:] == CANARY).all()
    return (info, sic.frames_of(d_tab.cpu().numpy().view(sic.FRAME_DTYPE), nf), fvc.verdicts_of(ver.view(fvc.VERDICT_DTYPE), nf), sv,
            d_res.cpu().numpy(), d_st.cpu().numpy(), d_out.cpu().numpy())


@pytest.mark.parametrize("route,repeat", [("few blocks", 1), ("bulk", 9)])
def test_index_decode_verify_with_one_synchronisation(eng, orc, route, repeat):
    """frames of 1, 5 and 9 blocks of 64 KiB with block checksums and a short last block, one stored block among them, the oracle's
    content checksums, a content size in the 5-block frame's header, a skippable frame in front and between: every frame is OK and
    sv.contentBytes is the plaintext's length.  Then the same stream with one stored checksum flipped, with one content size off by
    one, and with one payload byte flipped under its block checksum: that frame's verdict says so, the others' do not change, and
    sv names it with the bytes in front of it.  15 records in 85 entries: the few-block decoder's call; 135 in 205: the bulk kernels."""
    datas = [plaintext(777, 31), plaintext(5 * K64 - 1000, 32), plaintext(9 * K64 - 5, 33)]
    built = [encode_frame(eng, orc, d, content_size=d.size if k == 1 else None) for k, d in enumerate(datas)]
    parts, where, which = [], [], []                            # where: the LZ4 frames' offsets; which: their plaintexts
    for r in range(repeat):
        for k, (f, _, _) in enumerate(built):
            if k != 1:
                parts.append(sic.skippable(4 + k, 13 + 100 * k))
            where.append(sum(p.size for p in parts)); which.append(k)
            parts.append(f)
    stream = np.concatenate(parts)
    n_lz4, n_skip = 3 * repeat, 2 * repeat
    counts = [(datas[k].size + K64 - 1) // K64 for k in which]
    n = sum(counts); mr = n + 70; mf = n_lz4 + n_skip + 5
    assert (n <= 128 and mr <= 128) if route == "few blocks" else n > 128
    total = sum(datas[k].size for k in which)

    info, frames, ver, sv, res, st, out = index_decode_verify(eng, stream, mf, mr)
    assert (info["status"], info["nFrames"], info["nRecs"], info["nSkippable"]) == (sic.END, n_lz4 + n_skip, n, n_skip)
    lz4 = [j for j, f in enumerate(frames) if f["kind"] == 0]
    assert [frames[j]["hdrOff"] for j in lz4] == where
    assert sv == dict(contentBytes=total, firstBadFrame=-1, status=0, nFrames=n_lz4 + n_skip, nOk=n_lz4, nSkippable=n_skip)
    for j, f in enumerate(frames):
        if f["kind"] == 1:
            assert ver[j] == dict(contentSz=0, contentSum=0, status=fvc.SKIPPABLE, firstBad=-1, blockStatus=0)
    for j, k in zip(lz4, which):
        assert ver[j] == dict(contentSz=datas[k].size, contentSum=orc.xxh32(datas[k]), status=fvc.OK, firstBad=-1, blockStatus=0), (route, j)
        a = frames[j]["firstRec"]
        assert np.array_equal(out[a * K64:a * K64 + datas[k].size], datas[k])
    assert any(int.from_bytes(bytes(stream[w + off[1]:w + off[1] + 4]), "little") >> 31 for w, k in zip(where, which) if k
               for off in [built[k][1]]), "no stored block in the stream"

    def bytes_before(j):
        return sum(datas[k].size for jj, k in zip(lz4, which) if jj < j)

    def rerun(changed, j, status):
        info2, frames2, ver2, sv2, res2, st2, _ = index_decode_verify(eng, changed, mf, mr)
        assert info2["status"] == sic.END and info2["nFrames"] == info["nFrames"]
        assert [v for jj, v in enumerate(ver2) if jj != j] == [v for jj, v in enumerate(ver) if jj != j], "another frame's verdict changed"
        assert ver2[j]["status"] == status
        assert (sv2["firstBadFrame"], sv2["status"], sv2["nOk"], sv2["nSkippable"]) == (j, status, n_lz4 - 1, n_skip)
        return ver2[j], sv2, st2

    # one frame's stored checksum flipped: the last 9-block frame
    t = len(where) - 1; j = lz4[t]
    changed = stream.copy(); changed[where[t] + built[2][0].size - 3] ^= 0x10
    v, sv2, _ = rerun(changed, j, fvc.CONTENT_HASH)
    assert v == dict(ver[j], status=fvc.CONTENT_HASH) and sv2["contentBytes"] == bytes_before(j) + datas[2].size
    # one frame's content size off by one: the last 5-block frame (header: magic, FLG, BD, the size, the hash byte)
    t = len(where) - 2; j = lz4[t]
    changed = stream.copy()
    changed[where[t] + 6:where[t] + 14] = np.frombuffer(int(datas[1].size + 1).to_bytes(8, "little"), dtype=np.uint8)
    changed[where[t] + 14] = (sic.xxh32_short(bytes(changed[where[t] + 4:where[t] + 14])) >> 8) & 0xFF
    v, sv2, _ = rerun(changed, j, fvc.CONTENT_SIZE)
    assert v == dict(ver[j], status=fvc.CONTENT_SIZE) and sv2["contentBytes"] == bytes_before(j) + datas[1].size
    # one payload byte flipped under a block checksum: record 2 of the first 9-block frame
    t = 2; j = lz4[t]
    changed = stream.copy(); changed[where[t] + int(built[2][1][2]) + 4 + 9] ^= 0x04
    v, sv2, st2 = rerun(changed, j, fvc.BLOCK)
    bad = frames[j]["firstRec"] + 2
    assert int(st2[bad]) == fvc.BLK_HASH_MISMATCH and (np.delete(st2[:n], bad) == fvc.BLK_OK).all()
    assert v == dict(contentSz=2 * K64, contentSum=orc.xxh32(datas[2][:2 * K64]), status=fvc.BLOCK, firstBad=bad, blockStatus=fvc.BLK_HASH_MISMATCH)
    assert sv2["contentBytes"] == bytes_before(j) + 2 * K64


# ---------------------------------------------------------------------------------------------------- 3. linked frames
def test_two_linked_frames(eng, orc):
    """two linked frames (FLG bit 5 clear) of 3 and 4 blocks, a skippable frame between, decoded by plz4hip_dev_decode_records_ex
    with the entries' firstRec as chainFirst: the call takes that decoder's layout as it takes the other's"""
    import torch
    dev = torch.device("cuda:0")
    datas = [plaintext(3 * K64 - 11, 41), plaintext(4 * K64, 42)]
    built = [encode_frame(eng, orc, d, linked=True) for d in datas]
    stream = np.concatenate([built[0][0], sic.skippable(0, 40), built[1][0]])
    n, mf = 7, 4
    d_bytes = torch.from_numpy(stream).to(dev)
    d_tab = torch.zeros(mf * 64, dtype=torch.uint8, device=dev)
    d_off = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    d_info = torch.zeros(32, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    eng.dev_index_stream(d_bytes.data_ptr(), stream.size, mf, n, d_tab.data_ptr(), d_off.data_ptr(), d_info.data_ptr(), s)
    torch.cuda.synchronize()                                   # (chainFirst is a host array: the table is read here)
    info = sic.info_of(d_info.cpu().numpy().view(sic.INFO_DTYPE)[0])
    frames = sic.frames_of(d_tab.cpu().numpy().view(sic.FRAME_DTYPE), info["nFrames"])
    lz4 = [f for f in frames if f["kind"] == 0]
    assert info["status"] == sic.END and info["nRecs"] == n and not info["flagsOr"] & 0x20 and [f["firstRec"] for f in lz4] == [0, 3]
    cap = K64 + 8; stride = (cap + 64 + 15) // 16 * 16
    d_out = torch.full((n * stride,), 0xA5, dtype=torch.uint8, device=dev)
    d_res = torch.full((n,), -9, dtype=torch.int32, device=dev); d_st = torch.full((n,), -9, dtype=torch.int32, device=dev)
    d_w = torch.zeros(2 * 131072, dtype=torch.uint8, device=dev); d_wl = torch.zeros(2, dtype=torch.int32, device=dev)
    eng.dev_decode_records_ex(d_bytes.data_ptr(), d_off.data_ptr(), n, K64, True, d_out.data_ptr(), stride, cap, d_res.data_ptr(), d_st.data_ptr(),
                              linked=True, chain_first=[f["firstRec"] for f in lz4] + [n], windows_ptr=d_w.data_ptr(), window_len_ptr=d_wl.data_ptr(),
                              stream=s)
    ver, sv = verify_on_device(eng, d_tab.data_ptr(), d_info.data_ptr(), mf, d_out.data_ptr(), stride, cap, d_res.data_ptr(), d_st.data_ptr(), n)
    assert (d_st.cpu().numpy() == fvc.BLK_OK).all()
    assert sv == dict(contentBytes=datas[0].size + datas[1].size, firstBadFrame=-1, status=0, nFrames=3, nOk=2, nSkippable=1)
    assert [v["status"] for v in ver] == [fvc.OK, fvc.SKIPPABLE, fvc.OK]
    assert [(ver[j]["contentSz"], ver[j]["contentSum"]) for j in (0, 2)] == [(d.size, orc.xxh32(d)) for d in datas]


# ---------------------------------------------------------------------------------------------------- 4. arguments
def test_bad_arguments(eng):
    import torch
    from plz4_amd._native import EngineError
    buf = torch.zeros(256, dtype=torch.int64, device="cuda:0")
    p = buf.data_ptr()
    good = dict(frames_ptr=p, info_ptr=p + 256, max_frames=2, dst_ptr=p + 512, dst_stride=64, dst_cap=64, result_ptr=p + 1024,
                status_ptr=p + 1088, max_recs=4, verdicts_ptr=p + 1280, sv_ptr=p + 1536)
    for kw in (dict(frames_ptr=None), dict(info_ptr=None), dict(dst_ptr=None), dict(result_ptr=None), dict(status_ptr=None), dict(verdicts_ptr=None),
               dict(sv_ptr=None), dict(max_frames=-1), dict(max_recs=-1), dict(max_recs=0x7FFFFFFF), dict(dst_cap=-1), dict(dst_stride=63),
               dict(result_ptr=None, max_recs=0), dict(status_ptr=None, max_frames=0), dict(info_ptr=None, max_frames=0), dict(sv_ptr=None, max_frames=0)):
        with pytest.raises(EngineError) as ei:
            eng.dev_verify_frames(**dict(good, **kw))
        assert ei.value.code == -1, kw
    # the call itself, over an empty table (info->nFrames is 0): sv is written, nothing else
    buf[192:196] = -1
    eng.dev_verify_frames(**good)
    torch.cuda.synchronize()
    empty = dict(contentBytes=0, firstBadFrame=-1, status=0, nFrames=0, nOk=0, nSkippable=0)
    assert fvc.sv_of(buf[192:196].cpu().numpy().view(fvc.SV_DTYPE)[0]) == empty and not buf[160:192].any()
    # frames, verdicts and dst may be null where maxFrames == 0 makes them unused, dst where maxRecs == 0 does
    for kw in (dict(frames_ptr=None, verdicts_ptr=None, dst_ptr=None, max_frames=0), dict(dst_ptr=None, max_recs=0)):
        buf[192:196] = -1
        eng.dev_verify_frames(**dict(good, **kw))
        torch.cuda.synchronize()
        assert fvc.sv_of(buf[192:196].cpu().numpy().view(fvc.SV_DTYPE)[0]) == empty, kw
