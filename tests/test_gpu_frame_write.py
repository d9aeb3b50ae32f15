"""plz4hip_dev_write_frames on the GPU (k_frame_edges, k_frame_move, k_frame_summary): whole LZ4 frames around the block section an
encode left in device memory.  Expected values: the model of the header's table of rules in frame_write_cases.py, the stream assembled
on the host from the oracle's header and xxh32, the oracle's frame, and what plz4hip_dev_index_stream lists for the written stream.
The hostile tables are the ones the lane emulation and the sanitizer program ran first: the checks must refuse them."""
import functools
import os

import numpy as np
import pytest

import body_index_cases as bic
import frame_verify_cases as fvc
import frame_write_cases as fwc
import stream_index_cases as sic
from plz4_amd import synth

pytestmark = pytest.mark.gpu

K64 = 64 << 10
CANARY = fwc.CANARY
WAVES = "PLZ4HIP_WRITE_WAVES"


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


def call(eng, c, src_ptr, body_ptr, off_ptr, out_ptr, tab_ptr, out_off_ptr, info_ptr, waves=None, **kw):
    """the call for a case of frame_write_cases; PLZ4HIP_WRITE_WAVES is read per call"""
    import torch
    o = c.opts
    old = os.environ.pop(WAVES, None)
    try:
        if waves is not None:
            os.environ[WAVES] = str(waves)
        args = dict(src_ptr=src_ptr, src_bytes=c.src_bytes, body_ptr=body_ptr, body_bytes=c.body_bytes, recoff_ptr=off_ptr, blocks_per_frame=c.k,
                    out_ptr=out_ptr, out_cap=c.out_cap, frames_ptr=tab_ptr, out_recoff_ptr=out_off_ptr, info_ptr=info_ptr, bsz=o["bsz"],
                    block_checksum=o["blockChecksum"], content_checksum=o["contentChecksum"], content_size=o["contentSize"],
                    dict_id=o["dictId"] if o["hasDictId"] else None, linked=o["linked"], src_stride=c.stride,
                    stream=torch.cuda.current_stream().cuda_stream)
        args.update(kw)
        eng.dev_write_frames(**args)
    finally:
        os.environ.pop(WAVES, None)
        if old is not None:
            os.environ[WAVES] = old


def write_on_device(eng, c):
    """the call with guard words around every input and output -> what test_frame_write.check takes"""
    import torch
    g = fwc.geometry(c)
    n, nf = g["n"], g["nf"]
    ins = [guarded(a) for a in (c.src, c.body, c.rec_off)]
    outs = [guarded(np.full(size, CANARY, np.uint8)) for size in (c.out_cap, nf * 64, (n + 1) * 8, 32)]
    call(eng, c, *[p for _, p in ins], *[p for _, p in outs], waves=c.waves if c.waves < 1 << 20 else None)
    torch.cuda.synchronize()
    for (t, _), a in zip(ins, (c.src, c.body, c.rec_off)):
        back = t.cpu().numpy()
        assert (back[:64] == CANARY).all() and (back[back.size - 64:] == CANARY).all() and \
            np.array_equal(back[64:back.size - 64], np.ascontiguousarray(a).view(np.uint8).reshape(-1)), (c.name, "an input was written")
    got = []
    for (t, _), what in zip(outs, ("[out, out + outCap)", "frames[0 .. nFrames)", "outRecOff[0 .. nBlocks]", "info")):
        back = t.cpu().numpy()
        assert (back[:64] == CANARY).all() and (back[back.size - 64:] == CANARY).all(), (c.name, "a store outside " + what)
        got.append(back[64:back.size - 64].copy())
    return dict(out=got[0], frames=got[1], out_rec_off=got[2].view(np.int64), info=fwc.info_of(got[3].view(fwc.INFO_DTYPE)[0]))


def check(c, got, want):
    """what the call left against the model's answer (test_frame_write.check with this file's canary in recOff)"""
    assert got["info"] == want["info"], (c.name, got["info"], want["info"])
    if want["frames"] is None:                                  # NO_ROOM: nothing but info is written
        assert (got["frames"] == CANARY).all() and (got["out_rec_off"].view(np.uint8) == CANARY).all() and (got["out"] == CANARY).all(), \
            (c.name, "written without room")
        return
    frames = sic.frames_of(got["frames"].view(sic.FRAME_DTYPE), len(want["frames"]))
    assert frames == want["frames"], (c.name, [(j, g, w) for j, (g, w) in enumerate(zip(frames, want["frames"])) if g != w][:1])
    assert np.array_equal(got["out_rec_off"], want["out_rec_off"]), c.name
    if want["stream"] is not None:
        start, end = want["start"], want["info"]["end"]
        assert np.array_equal(got["out"][start:end], want["stream"]), (c.name, "the stream")
        assert (got["out"][:start] == CANARY).all() and (got["out"][end:] == CANARY).all(), (c.name, "a store in front of or behind the stream")


# ---------------------------------------------------------------------------------------------------- 1. the case list
@pytest.fixture(scope="module")
def the_cases(orc):
    good, bad = fwc.cases(orc)
    return [(c, fwc.model(orc, c)) for c in good], [(c, fwc.model(orc, c)) for c in bad]


def test_the_cases(eng, the_cases):
    """every good case of frame_write_cases.cases on the kernels, grids of 1 - 3 waves among them"""
    assert {c.waves for c, _ in the_cases[0]} >= {1, 2, 3}
    for c, want in the_cases[0]:
        assert want["info"]["status"] == fwc.OK
        check(c, write_on_device(eng, c), want)


def test_the_failure_cases(eng, the_cases):
    """failed records, overflowed bodies, tables that hold anything, no room: the verdict, the lowest bad record, and no byte outside"""
    seen = set()
    for c, want in the_cases[1]:
        check(c, write_on_device(eng, c), want)
        seen.add(want["info"]["status"])
    assert seen == {fwc.NO_ROOM, fwc.RECORD}


def test_the_empty_input(eng, orc):
    """srcBytes == 0: one empty frame, the oracle's; recOff is not read (it holds what an encode of nothing left: nothing)"""
    for cck in (False, True):
        c = fwc.Case("empty", fwc.opts(False, cck), np.zeros(0, np.uint8), 0, K64, np.zeros(0, np.uint8), np.array([-77], np.int64), 0, out_cap=11 + 4 * cck)
        got = write_on_device(eng, c)
        assert got["info"] == dict(end=11 + 4 * cck, nFrames=1, nRecs=0, status=fwc.OK, firstBadRec=-1)
        assert np.array_equal(got["out"], orc.frame_encode(np.zeros(0, np.uint8), 4, False, cck)) and got["out_rec_off"][0] == 0
        if cck:
            assert bytes(got["out"][-4:]) == (0x02CC5D05).to_bytes(4, "little")


# ---------------------------------------------------------------------------------------------------- 2. the pipeline
@functools.lru_cache(maxsize=None)
def plaintext(n_bytes: int, seed: int) -> np.ndarray:
    """text with one incompressible block of 64 KiB in it: its record is a stored one"""
    data = synth.text(n_bytes, seed=seed)
    data[K64:2 * K64] = synth.random_bytes(K64, seed=seed)
    data.setflags(write=False)
    return data


@pytest.mark.parametrize("route,n_bytes", [("few blocks", 11 * K64 - 1000), ("bulk", 131 * K64 - 5)])
@pytest.mark.parametrize("k", [0, 1, 3])
def test_encode_write_index_decode_verify_with_one_synchronisation(eng, orc, route, n_bytes, k):
    """plz4hip_dev_encode_body -> plz4hip_dev_write_frames -> plz4hip_dev_index_stream -> ONE plz4hip_dev_decode_records ->
    plz4hip_dev_verify_frames on one stream, one synchronisation behind all five.  Decode and verify run on the WRITER's tables (the
    first fields of its info are laid out as the index's); the index's tables must be the same.  11 records: the few-block decoder's
    call; 131: the bulk kernels."""
    import torch
    dev = torch.device("cuda:0")
    data = plaintext(n_bytes, 51)
    n = (n_bytes + K64 - 1) // K64
    assert (n <= 128) == (route == "few blocks")
    nf = (n + k - 1) // k if k else 1
    H, T = 15, 8
    d_src = torch.from_numpy(np.array(data)).to(dev)
    d_body = torch.zeros(n * (K64 + 8), dtype=torch.uint8, device=dev)
    d_off = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    d_len = torch.zeros(n, dtype=torch.int32, device=dev)
    cap = n * (K64 + 8) + nf * (H + T)
    d_out = torch.full((cap,), CANARY, dtype=torch.uint8, device=dev)
    d_tab = torch.full((nf * 64,), CANARY, dtype=torch.uint8, device=dev)
    d_ooff = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    d_winfo = torch.full((32,), CANARY, dtype=torch.uint8, device=dev)
    d_tab2 = torch.zeros((nf + 2) * 64, dtype=torch.uint8, device=dev)
    d_off2 = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    d_info = torch.zeros(32, dtype=torch.uint8, device=dev)
    d_dst = torch.full((n * K64,), 0xA5, dtype=torch.uint8, device=dev)
    d_res = torch.full((n,), -9, dtype=torch.int32, device=dev); d_st = torch.full((n,), -9, dtype=torch.int32, device=dev)
    d_ver = torch.full((nf * 32,), CANARY, dtype=torch.uint8, device=dev)
    d_sv = torch.full((32,), CANARY, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    eng.dev_encode_body(d_src.data_ptr(), n_bytes, K64, True, d_body.data_ptr(), d_body.numel(), d_off.data_ptr(), d_len.data_ptr(), s)
    eng.dev_write_frames(d_src.data_ptr(), n_bytes, d_body.data_ptr(), d_body.numel(), d_off.data_ptr(), k, d_out.data_ptr(), cap, d_tab.data_ptr(),
                         d_ooff.data_ptr(), d_winfo.data_ptr(), K64, block_checksum=True, content_checksum=True, content_size=True, stream=s)
    # (the index gets the capacity, not the stream's length, which only the device knows: it stops at the canary behind the stream)
    eng.dev_index_stream(d_out.data_ptr(), cap, nf + 2, n, d_tab2.data_ptr(), d_off2.data_ptr(), d_info.data_ptr(), s)
    eng.dev_decode_records(d_out.data_ptr(), d_ooff.data_ptr(), n, K64, True, d_dst.data_ptr(), K64, K64, d_res.data_ptr(), d_st.data_ptr(), s)
    eng.dev_verify_frames(d_tab.data_ptr(), d_winfo.data_ptr(), nf, d_dst.data_ptr(), K64, K64, d_res.data_ptr(), d_st.data_ptr(), n,
                          d_ver.data_ptr(), d_sv.data_ptr(), s)
    torch.cuda.synchronize()

    off = d_off.cpu().numpy(); body = d_body.cpu().numpy()[:int(off[n])]
    winfo = fwc.info_of(d_winfo.cpu().numpy().view(fwc.INFO_DTYPE)[0])
    # the stream assembled on the host, as the tests did before there was a writer
    parts = []
    for f in range(nf):
        first, last = (f * k, min((f + 1) * k, n)) if k else (0, n)
        piece = data[first * K64:min(last * K64, n_bytes)]
        parts += [sic.u8(orc.frame_header(4, block_checksum=True, content_checksum=True, content_size=piece.size)), body[off[first]:off[last]],
                  bic.le32(0), bic.le32(orc.xxh32(piece))]
    want = np.concatenate(parts)
    assert winfo == dict(end=want.size, nFrames=nf, nRecs=n, status=fwc.OK, firstBadRec=-1), (winfo, want.size)
    out = d_out.cpu().numpy()
    assert np.array_equal(out[:want.size], want) and (out[want.size:] == CANARY).all()
    assert any(int.from_bytes(bytes(body[a:a + 4]), "little") >> 31 for a in off[:n]) and not all(
        int.from_bytes(bytes(body[a:a + 4]), "little") >> 31 for a in off[:n]), "stored and compressed records"
    if k == 0:
        hdr = sic.u8(orc.frame_header(4, block_checksum=True, content_checksum=True, content_size=n_bytes))
        assert np.array_equal(out[:want.size], np.concatenate([hdr, orc.frame_encode(np.array(data), 4, True, True)[7:]])), "the oracle's frame"
    # the index lists what the writer listed
    info = sic.info_of(d_info.cpu().numpy().view(sic.INFO_DTYPE)[0])
    assert (info["nFrames"], info["nRecs"], info["end"], info["nSkippable"]) == (nf, n, want.size, 0), info
    assert info["status"] == (sic.END if want.size == cap else sic.MAGIC)
    frames = sic.frames_of(d_tab.cpu().numpy().view(sic.FRAME_DTYPE), nf)
    assert frames == sic.frames_of(d_tab2.cpu().numpy().view(sic.FRAME_DTYPE), nf)
    assert np.array_equal(d_ooff.cpu().numpy(), d_off2.cpu().numpy())
    # every verdict is OK, on the writer's tables
    sv = fvc.sv_of(d_sv.cpu().numpy().view(fvc.SV_DTYPE)[0])
    assert sv == dict(contentBytes=n_bytes, firstBadFrame=-1, status=0, nFrames=nf, nOk=nf, nSkippable=0), sv
    ver = fvc.verdicts_of(d_ver.cpu().numpy().view(fvc.VERDICT_DTYPE), nf)
    assert all(v["status"] == fvc.OK for v in ver) and [v["contentSum"] for v in ver] == [f["contentSum"] for f in frames]
    assert (d_st.cpu().numpy() == fvc.BLK_OK).all() and np.array_equal(d_dst.cpu().numpy()[:n_bytes], data)


# ---------------------------------------------------------------------------------------------------- 3. a linked frame
@pytest.mark.parametrize("dict_id", [None, 0xCAFE0001])
def test_a_linked_frame_is_read_back_by_the_host_layer(eng, orc, dict_id):
    """plz4hip_dev_encode_body_ex(linked = 1) -> plz4hip_dev_write_frames(linked, one frame): FLG bit 5 clear, and the host layer's
    Reader over the oracle's engine reads the plaintext back"""
    import torch
    from hostengine import oracle_engine
    from plz4_amd import host
    dev = torch.device("cuda:0")
    data = plaintext(5 * K64 - 321, 52)
    n = 5
    d_src = torch.zeros(K64 + data.size, dtype=torch.uint8, device=dev)
    d_src[K64:] = torch.from_numpy(np.array(data)).to(dev)
    d_body = torch.zeros(n * (K64 + 8), dtype=torch.uint8, device=dev)
    d_off = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    d_len = torch.zeros(n, dtype=torch.int32, device=dev)
    cap = n * (K64 + 8) + 27
    d_out = torch.full((cap,), CANARY, dtype=torch.uint8, device=dev)
    d_tab = torch.zeros(64, dtype=torch.uint8, device=dev)
    d_ooff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_winfo = torch.zeros(32, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    eng.dev_encode_body_ex(d_src.data_ptr() + K64, data.size, K64, K64, True, d_body.data_ptr(), d_body.numel(), d_off.data_ptr(), d_len.data_ptr(),
                           linked=True, stream=s)
    eng.dev_write_frames(d_src.data_ptr() + K64, data.size, d_body.data_ptr(), d_body.numel(), d_off.data_ptr(), 0, d_out.data_ptr(), cap,
                         d_tab.data_ptr(), d_ooff.data_ptr(), d_winfo.data_ptr(), K64, block_checksum=True, content_checksum=True, content_size=True,
                         dict_id=dict_id, linked=True, stream=s)
    torch.cuda.synchronize()
    winfo = fwc.info_of(d_winfo.cpu().numpy().view(fwc.INFO_DTYPE)[0])
    assert (winfo["status"], winfo["nFrames"], winfo["nRecs"]) == (fwc.OK, 1, n)
    frame = d_out.cpu().numpy()[:winfo["end"]]
    hdr = orc.frame_header(4, linked=True, block_checksum=True, content_checksum=True, content_size=data.size, dict_id=dict_id)
    assert bytes(frame[:len(hdr)]) == hdr and not frame[4] & 0x20
    assert bytes(frame[-4:]) == orc.xxh32(data).to_bytes(4, "little")
    e = oracle_engine()
    try:
        size, plain, err = host.Reader(e, frame.tobytes()).write_to()
        assert int(err) == host.OK and size == data.size and plain == data.tobytes()
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------- 4. arguments
def test_bad_arguments(eng):
    import torch
    from plz4_amd._native import EngineError
    buf = torch.zeros(4096, dtype=torch.int64, device="cuda:0")
    p = buf.data_ptr()
    good = dict(src_ptr=p, src_bytes=100, body_ptr=p + 1024, body_bytes=200, recoff_ptr=p + 2048, blocks_per_frame=1, out_ptr=p + 4096, out_cap=1000,
                frames_ptr=p + 8192, out_recoff_ptr=p + 8192 + 256, info_ptr=p + 8192 + 512, bsz=K64)
    for kw in (dict(src_ptr=None), dict(body_ptr=None), dict(recoff_ptr=None), dict(out_ptr=None), dict(frames_ptr=None), dict(out_recoff_ptr=None),
               dict(info_ptr=None), dict(src_bytes=-1), dict(body_bytes=-1), dict(out_cap=-1), dict(body_bytes=(1 << 62) + 1), dict(out_cap=(1 << 62) + 1),
               dict(bsz=0), dict(bsz=K64 + 1), dict(bsz=32 << 10), dict(bsz=8 << 20), dict(bsz=128 << 10), dict(src_stride=K64 - 1),
               dict(src_stride=K64 + 1), dict(src_stride=2 * K64 - 1), dict(src_stride=0), dict(blocks_per_frame=-1), dict(linked=True),
               dict(linked=True, blocks_per_frame=3), dict(reserved=1)):
        with pytest.raises(EngineError) as ei:
            eng.dev_write_frames(**dict(good, **kw))
        assert ei.value.code == -1, kw
    # the call itself: recOff = {0, 0} is a record that takes no room; then the null pointers the rules allow
    def info():
        torch.cuda.synchronize()
        return fwc.info_of(buf[1024 + 64:1024 + 68].cpu().numpy().view(fwc.INFO_DTYPE)[0])
    eng.dev_write_frames(**good)
    assert info() == dict(end=15, nFrames=1, nRecs=1, status=fwc.RECORD, firstBadRec=0)
    for kw in (dict(src_ptr=None, content_checksum=False), dict(src_ptr=None, src_bytes=0), dict(body_ptr=None, body_bytes=0),
               dict(linked=True, blocks_per_frame=0), dict(src_stride=2 * K64)):
        buf[1024 + 64:1024 + 68] = -1
        eng.dev_write_frames(**dict(good, **kw))
        assert info()["status"] in (fwc.OK, fwc.RECORD), kw
