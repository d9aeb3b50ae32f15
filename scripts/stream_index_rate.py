"""The index of a whole LZ4 stream that is already on the device (plz4hip_dev_index_stream, k_index_stream: one wavefront, a header
in one round trip, one dependent load per record, one per trailer) beside the host loop it replaces -- per frame: copy the header
back and parse it, plz4hip_dev_index_body, wait for its info, copy the trailer back (hipMemcpy through ctypes, a Python loop around
it) -- beside plz4hip_dev_index_body over the same records as ONE bare block section (what the frames add to the chain), and beside
plz4hip_dev_decode_records over the global recOff, which is what the index is there to feed.  Two streams, built on the device from
bodies plz4hip_dev_encode_body wrote from synthetic T text with block checksums: 16384 one-block frames of 64 KiB blocks, and 64
frames of 96 blocks of 4 MiB (fewer frames where the memory does not hold them).  Every frame: the 7-byte header (block and content
checksum flags), its records, the end mark and four bytes where the content checksum goes (zeros: nothing here verifies it).  The
kernels are timed with device events, warm, one call per window, the median of REPS windows (minimum and maximum beside it); the
host loop with a host clock around the whole stream, the median of HOST_REPS walks.  The index must list every frame and reproduce
the offsets the stream was laid out with.  No threshold: the comparison is between the numbers.
    python scripts/stream_index_rate.py [out.json]"""
import ctypes as C
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np
from index_rate import hip_runtime, stats, timed

POOL = 16                                    # distinct blocks, tiled over the plaintext
SHAPES = (("64KiB_1x16384", 64 << 10, 4, 1, 16384), ("4MiB_96x64", 4 << 20, 7, 96, 64))      # name, bsz, BD id, blocks a frame, frames
REPS = int(os.environ.get("STREAM_INDEX_RATE_REPS", "20"))
HOST_REPS = int(os.environ.get("STREAM_INDEX_RATE_HOST_REPS", "3"))
DEC_REPS = int(os.environ.get("STREAM_INDEX_RATE_DEC_REPS", "5"))
HDR, TAIL = 7, 8                             # the header; end mark + content checksum


def host_loop(hip, eng, base, n_bytes, max_recs, recoff_ptr, info_ptr, stream):
    """the reader's walk with the host in the chain: per frame a header copy, the body index, a wait for its info, a trailer copy.
    recOff comes out frame by frame, each frame's offsets from its own first record.  -> (frames, records)"""
    from plz4_amd._native import BodyIndex, BODY_END_MARK
    hdr = (C.c_uint8 * 19)(); info = BodyIndex(); trailer = C.c_uint32(0)
    off, frames, recs = 0, 0, 0
    while off != n_bytes:
        take = min(19, n_bytes - off)
        if take < 7 or hip.hipMemcpy(hdr, base + off, take, 2) != 0:                       # 2: hipMemcpyDeviceToHost
            raise RuntimeError("header")
        flg, bd = hdr[4], hdr[5]
        if bytes(hdr[0:4]) != b"\x04\x22\x4d\x18" or flg >> 6 != 1 or flg & 0x0B:          # (no content size, no dictionary id here)
            raise RuntimeError("not a header of this stream")
        body = off + 7
        eng.dev_index_body(base + body, n_bytes - body, (64 << 10) << 2 * ((bd >> 4 & 7) - 4), bool(flg & 16), max_recs - recs,
                           recoff_ptr + 8 * recs, info_ptr, stream)
        if hip.hipMemcpy(C.byref(info), info_ptr, 16, 2) != 0 or info.status != BODY_END_MARK:
            raise RuntimeError("body")
        recs += info.nBlocks
        off = body + info.end
        if flg & 4:
            if hip.hipMemcpy(C.byref(trailer), base + off, 4, 2) != 0:
                raise RuntimeError("trailer")
            off += 4
        frames += 1
    return frames, recs


class Built:
    """what build_stream leaves: d_stream (n_bytes), d_body (body_bytes: the encoder's bare block section; the caller deletes it),
    nf frames of per_frame records, nb records, frame_at (every frame's offset), want_off (every record's), the host's pool"""


def build_stream(eng, bsz, bd_id, per_frame, want_frames, sums=None):
    """the stream of a shape on the device: frame f = header, records [f * per_frame, (f + 1) * per_frame), end mark, content
    checksum.  sums(pool, nf) -> the nf content checksums (uint32) to store; None: zeros"""
    import torch
    from plz4_amd import host, synth
    dev = torch.device("cuda:0")
    free, _ = torch.cuda.mem_get_info()
    per_block = bsz + 2 * (bsz + 8) + bsz + (9 * bsz) // 4 + 64         # plaintext, body, stream, decoded output / the level-1 workspace
    nf = int(min(want_frames, (free * 7 // 10) // (per_block * per_frame)))
    nb = nf * per_frame
    pool = synth.text(POOL * bsz)
    d_pool = torch.from_numpy(pool).to(dev)
    d_src = torch.empty(nb * bsz, dtype=torch.uint8, device=dev)
    d_src.view(nb, bsz)[:] = d_pool.view(POOL, bsz).repeat((nb + POOL - 1) // POOL, 1)[:nb]
    del d_pool
    cap = nb * (bsz + 8)
    d_body = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_enc_off = torch.zeros(nb + 1, dtype=torch.int64, device=dev); d_len = torch.zeros(nb, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    eng.dev_encode_body(d_src.data_ptr(), nb * bsz, bsz, True, d_body.data_ptr(), cap, d_enc_off.data_ptr(), d_len.data_ptr(), stream=s)
    torch.cuda.synchronize()
    enc_off = d_enc_off.cpu().numpy()
    body_bytes = int(enc_off[nb])
    assert 0 < body_bytes <= cap
    del d_src
    eng.trim(); torch.cuda.empty_cache()
    # the stream: frame f = header, records [f * per_frame, (f + 1) * per_frame), end mark, content checksum
    header = np.frombuffer(host.write_header(block_checksum=True, content_checksum=True, block_size=bd_id), dtype=np.uint8)
    assert header.size == HDR
    first = enc_off[0:nb:per_frame]                                      # the body offset of every frame's first record
    frame_at = first + (HDR + TAIL) * np.arange(nf, dtype=np.int64)      # where every frame starts in the stream
    n_bytes = body_bytes + (HDR + TAIL) * nf
    want_off = enc_off[:nb] + np.repeat(frame_at + HDR - first, per_frame)
    d_stream = torch.empty(n_bytes, dtype=torch.uint8, device=dev)
    for f in range(nf):
        a, b = int(enc_off[f * per_frame]), int(enc_off[(f + 1) * per_frame])
        at = int(frame_at[f]) + HDR
        d_stream[at:at + b - a] = d_body[a:b]
    d_at = torch.from_numpy(frame_at).to(dev)
    d_stream[(d_at[:, None] + torch.arange(HDR, device=dev)[None, :]).reshape(-1)] = torch.from_numpy(header.copy()).to(dev).repeat(nf)
    d_ends = torch.from_numpy(np.append(frame_at[1:], n_bytes) - TAIL).to(dev)
    trailer = np.zeros((nf, TAIL), dtype=np.uint8)
    if sums is not None:
        trailer[:, 4:] = np.ascontiguousarray(sums(pool, nf), dtype="<u4").view(np.uint8).reshape(nf, 4)
    d_stream[(d_ends[:, None] + torch.arange(TAIL, device=dev)[None, :]).reshape(-1)] = torch.from_numpy(trailer.reshape(-1)).to(dev)
    torch.cuda.synchronize()
    b = Built()
    b.d_stream, b.d_body, b.n_bytes, b.body_bytes, b.nf, b.nb, b.frame_at, b.want_off, b.pool = d_stream, d_body, n_bytes, body_bytes, nf, nb, frame_at, want_off, pool
    return b


def measure(name, bsz, bd_id, per_frame, want_frames):
    import torch
    from plz4_amd._native import Engine, FrameIndex, StreamIndex, BODY_END_OF_BYTES, STREAM_END
    dev = torch.device("cuda:0")
    hip = hip_runtime()
    eng = Engine(0)
    b = build_stream(eng, bsz, bd_id, per_frame, want_frames)
    d_stream, d_body, n_bytes, body_bytes, nf, nb, frame_at, want_off = b.d_stream, b.d_body, b.n_bytes, b.body_bytes, b.nf, b.nb, b.frame_at, b.want_off
    b.d_body = None
    s = torch.cuda.current_stream().cuda_stream
    # the new call
    mf, mr = nf + 1, nb + 70
    d_tab = torch.zeros(mf * C.sizeof(FrameIndex), dtype=torch.uint8, device=dev)
    d_off = torch.full((mr + 1,), -1, dtype=torch.int64, device=dev)
    d_info = torch.zeros(C.sizeof(StreamIndex), dtype=torch.uint8, device=dev)
    t_stream = timed(lambda: eng.dev_index_stream(d_stream.data_ptr(), n_bytes, mf, mr, d_tab.data_ptr(), d_off.data_ptr(), d_info.data_ptr(), s), 3, REPS)
    info = StreamIndex.from_buffer_copy(d_info.cpu().numpy().tobytes())
    assert (info.end, info.nFrames, info.nRecs, info.status, info.nSkippable) == (n_bytes, nf, nb, STREAM_END, 0)
    assert (info.maxBsz, info.flagsAnd, info.flagsOr) == (bsz, 0x74, 0x74)
    assert np.array_equal(d_off.cpu().numpy()[:nb], want_off), "the index is not the layout's recOff"
    tab = np.frombuffer(d_tab.cpu().numpy().tobytes(), dtype=np.int64).reshape(mf, 8)
    assert np.array_equal(tab[:nf, 0], frame_at) and np.array_equal(tab[:nf, 2], np.append(frame_at[1:], n_bytes))
    # the same records as one bare block section (the body the encoder wrote): the chain without the frames
    d_boff = torch.full((nb + 1,), -1, dtype=torch.int64, device=dev); d_binfo = torch.zeros(2, dtype=torch.int64, device=dev)
    t_body = timed(lambda: eng.dev_index_body(d_body.data_ptr(), body_bytes, bsz, True, nb, d_boff.data_ptr(), d_binfo.data_ptr(), s), 3, REPS)
    binfo = d_binfo.cpu().numpy()
    assert int(binfo[0]) == body_bytes and tuple(int(x) for x in binfo[1:2].view(np.int32)) == (nb, BODY_END_OF_BYTES)
    del d_body, d_boff
    torch.cuda.empty_cache()
    # the host loop the call replaces (parent functionality)
    d_hoff = torch.full((mr + 1,), -1, dtype=torch.int64, device=dev)
    t_host = []
    for rep in range(1 + HOST_REPS):
        t0 = time.perf_counter()
        got = host_loop(hip, eng, d_stream.data_ptr(), n_bytes, mr, d_hoff.data_ptr(), d_binfo.data_ptr(), s)
        t_host.append((time.perf_counter() - t0) * 1e3)
        assert got == (nf, nb)
    t_host = t_host[1:]
    del d_hoff
    # the decode the index feeds: one call over the global recOff, the padded tail included
    d_out = torch.empty(mr * bsz, dtype=torch.uint8, device=dev)
    d_res = torch.zeros(mr, dtype=torch.int32, device=dev); d_st = torch.zeros(mr, dtype=torch.int32, device=dev)
    t_dec = timed(lambda: eng.dev_decode_records(d_stream.data_ptr(), d_off.data_ptr(), mr, bsz, True, d_out.data_ptr(), bsz, bsz,
                                                 d_res.data_ptr(), d_st.data_ptr(), s), 2, DEC_REPS)
    assert int(d_st[:nb].abs().sum()) == 0 and int(d_res.to(torch.int64).sum()) == nb * bsz and bool((d_st[nb:] == 2).all())
    out = {"shape": name, "bsz": bsz, "frames": nf, "frames_wanted": want_frames, "blocks_per_frame": per_frame, "records": nb,
           "stream_bytes": n_bytes, "index_stream_ms": stats(t_stream), "index_body_same_records_ms": stats(t_body),
           "host_loop_ms": stats(t_host), "decode_records_ms": stats(t_dec)}
    sm, bm, hm, dm = (out[k]["median"] for k in ("index_stream_ms", "index_body_same_records_ms", "host_loop_ms", "decode_records_ms"))
    out["index_stream_us_per_frame_all_in"] = round(sm * 1e3 / nf, 3)
    out["index_stream_us_per_frame_beyond_its_records"] = round((sm - bm) * 1e3 / nf, 3)
    out["host_loop_us_per_frame"] = round(hm * 1e3 / nf, 3)
    out["host_loop_over_index_stream"] = round(hm / sm, 1)
    out["index_stream_over_decode"] = round(sm / dm, 3)
    del d_stream, d_out
    eng.trim(); eng.close(); torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    res = {"workload": "synthetic T text, block checksums, streams of frames around the records plz4hip_dev_encode_body wrote, resident in "
                       "device memory; kernels: one call per device-event window; host loop: per frame hipMemcpy of the header, "
                       "plz4hip_dev_index_body, hipMemcpy of its info, hipMemcpy of the trailer, from a Python loop",
           "reps": {"index": REPS, "host_loop": HOST_REPS, "decode": DEC_REPS}, "runs": []}
    for shape in SHAPES:
        res["runs"].append(measure(*shape))
        sys.stderr.write(json.dumps(res["runs"][-1]) + "\n")
    txt = json.dumps(res, indent=1)
    print(txt)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(txt + "\n")
