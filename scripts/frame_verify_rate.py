"""The verdict on every frame of a decoded stream that is on the device (plz4hip_dev_verify_frames: k_verify_frames, sixteen frames'
xxh32 chains per wavefront over the pieces the record decode left, and k_verify_summary) beside what the parent commit offers for the
same job over the same plaintext -- per frame: plz4hip_xxh32_stream_reset, plz4hip_dev_xxh32_stream_update over each of its blocks,
plz4hip_xxh32_stream_sum (which synchronises), a compare on the host, from a Python loop -- and beside the index and the decode the
verify follows.  The two streams of stream_index_rate.py (its build_stream), with REAL content checksums in the trailers: 16384
one-block frames of 64 KiB blocks, and 64 frames of 96 blocks of 4 MiB (fewer frames where the memory does not hold them).  A
frame's plaintext is tiles of a pool of 16 blocks, so the expected checksums are the engine's one-shot xxh32 (plz4hip_xxh32_batch)
of the few distinct frames, computed from the host's copy.  The kernels are timed with device events, warm, one call per window, the
median of the repetitions (minimum and maximum beside it); the host loop with a host clock around the whole stream (one walk behind
a warm-up frame: it is minutes long where the blocks are large; FRAME_VERIFY_RATE_PARENT_FRAMES walks fewer frames and says so).
Every verdict must be OK with sv.contentBytes the plaintext's length; then one stored checksum is flipped on the device and the run
must report exactly that frame.  No threshold: the comparison is between the numbers.
    python scripts/frame_verify_rate.py [out.json]"""
import ctypes as C
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np
from index_rate import stats, timed
from stream_index_rate import POOL, SHAPES, build_stream

REPS = int(os.environ.get("FRAME_VERIFY_RATE_REPS", "7"))
DEC_REPS = int(os.environ.get("FRAME_VERIFY_RATE_DEC_REPS", "5"))
PARENT_FRAMES = int(os.environ.get("FRAME_VERIFY_RATE_PARENT_FRAMES", "0"))          # 0: the whole stream


def measure(name, bsz, bd_id, per_frame, want_frames):
    import torch
    from plz4_amd._native import Engine, FrameIndex, FrameVerdict, StreamIndex, StreamVerdict, FRAME_OK, FRAME_CONTENT_HASH, STREAM_END
    dev = torch.device("cuda:0")
    eng = Engine(0)

    def sums(pool, nf):
        """frame f is blocks (f * per_frame + j) % POOL of the pool: one digest per distinct start"""
        blocks = pool.reshape(POOL, bsz)
        starts = sorted({(f * per_frame) % POOL for f in range(nf)})
        frames = [np.ascontiguousarray(blocks[(a + np.arange(per_frame)) % POOL]).reshape(-1) for a in starts]
        by_start = dict(zip(starts, (int(x) for x in eng.xxh32_batch(frames))))
        return np.array([by_start[(f * per_frame) % POOL] for f in range(nf)], dtype=np.uint32)

    b = build_stream(eng, bsz, bd_id, per_frame, want_frames, sums)
    b.d_body = None
    eng.trim(); torch.cuda.empty_cache()
    d_stream, n_bytes, nf, nb = b.d_stream, b.n_bytes, b.nf, b.nb
    want_sums = sums(b.pool, nf)
    s = torch.cuda.current_stream().cuda_stream
    mf, mr = nf + 1, nb + 70
    d_tab = torch.zeros(mf * C.sizeof(FrameIndex), dtype=torch.uint8, device=dev)
    d_off = torch.full((mr + 1,), -1, dtype=torch.int64, device=dev)
    d_info = torch.zeros(C.sizeof(StreamIndex), dtype=torch.uint8, device=dev)
    d_out = torch.empty(mr * bsz, dtype=torch.uint8, device=dev)
    d_res = torch.zeros(mr, dtype=torch.int32, device=dev); d_st = torch.zeros(mr, dtype=torch.int32, device=dev)
    d_ver = torch.zeros(mf * C.sizeof(FrameVerdict), dtype=torch.uint8, device=dev)
    d_sv = torch.zeros(C.sizeof(StreamVerdict), dtype=torch.uint8, device=dev)
    index = lambda: eng.dev_index_stream(d_stream.data_ptr(), n_bytes, mf, mr, d_tab.data_ptr(), d_off.data_ptr(), d_info.data_ptr(), s)
    decode = lambda: eng.dev_decode_records(d_stream.data_ptr(), d_off.data_ptr(), mr, bsz, True, d_out.data_ptr(), bsz, bsz, d_res.data_ptr(),
                                            d_st.data_ptr(), s)
    verify = lambda: eng.dev_verify_frames(d_tab.data_ptr(), d_info.data_ptr(), mf, d_out.data_ptr(), bsz, bsz, d_res.data_ptr(), d_st.data_ptr(),
                                           mr, d_ver.data_ptr(), d_sv.data_ptr(), s)
    t_index = timed(index, 2, REPS)
    t_dec = timed(decode, 2, DEC_REPS)
    t_ver = timed(verify, 2, REPS)
    t_all = timed(lambda: (index(), decode(), verify()), 1, DEC_REPS)                # the three calls in one window, no host in between
    info = StreamIndex.from_buffer_copy(d_info.cpu().numpy().tobytes())
    assert (info.end, info.nFrames, info.nRecs, info.status) == (n_bytes, nf, nb, STREAM_END)

    def verdicts():
        sv = StreamVerdict.from_buffer_copy(d_sv.cpu().numpy().tobytes())
        ver = np.frombuffer(d_ver.cpu().numpy().tobytes(), dtype=np.dtype([("contentSz", "<u8"), ("contentSum", "<u4"), ("status", "<i4"),
                                                                            ("firstBad", "<i4"), ("blockStatus", "<i4"), ("reserved", "<i4", (2,))]))
        return sv, ver[:nf]

    sv, ver = verdicts()
    assert (sv.nFrames, sv.nOk, sv.nSkippable, sv.firstBadFrame, sv.status, sv.contentBytes) == (nf, nf, 0, -1, 0, nb * bsz), "not every frame is OK"
    assert (ver["status"] == FRAME_OK).all() and (ver["contentSz"] == per_frame * bsz).all() and np.array_equal(ver["contentSum"], want_sums)
    # one stored checksum flipped on the device: exactly that frame is reported
    flip = nf * 2 // 3
    tab = np.frombuffer(d_tab.cpu().numpy().tobytes(), dtype=np.int64).reshape(mf, 8)
    at = int(tab[flip, 2]) - 2                                                       # a byte of the trailer's checksum
    d_stream[at] ^= 0x20
    index(); decode(); verify()
    torch.cuda.synchronize()
    sv2, ver2 = verdicts()
    assert (sv2.firstBadFrame, sv2.status, sv2.nOk, sv2.contentBytes) == (flip, FRAME_CONTENT_HASH, nf - 1, (flip + 1) * per_frame * bsz)
    assert ver2["status"][flip] == FRAME_CONTENT_HASH and (np.delete(ver2["status"], flip) == FRAME_OK).all()
    assert np.array_equal(ver2["contentSum"], want_sums)
    d_stream[at] ^= 0x20
    index(); decode(); verify()
    torch.cuda.synchronize()
    # the parent commit's way: a host loop per frame over the streaming checksum (one wavefront, four busy lanes)
    res = d_res.cpu().numpy()
    stored = np.frombuffer(d_tab.cpu().numpy().tobytes(), dtype=np.uint32).reshape(mf, 16)[:nf, 9].copy()
    h = eng.hash_create()
    out_ptr = d_out.data_ptr()

    def parent_walk(frames):
        bad = 0
        for f in range(frames):
            eng.hash_reset(h)
            for i in range(f * per_frame, (f + 1) * per_frame):
                eng.dev_hash_update(h, out_ptr + i * bsz, int(res[i]), s)
            bad += eng.hash_sum(h) != int(stored[f])
        return bad

    walked = nf if PARENT_FRAMES <= 0 else min(nf, PARENT_FRAMES)
    assert parent_walk(1) == 0                                                       # warm
    t0 = time.perf_counter()
    assert parent_walk(walked) == 0
    t_parent = (time.perf_counter() - t0) * 1e3
    eng.hash_destroy(h)
    out = {"shape": name, "bsz": bsz, "frames": nf, "frames_wanted": want_frames, "blocks_per_frame": per_frame, "records": nb,
           "plaintext_bytes": nb * bsz, "verify_frames_ms": stats(t_ver), "index_stream_ms": stats(t_index), "decode_records_ms": stats(t_dec),
           "index_decode_verify_one_window_ms": stats(t_all), "parent_host_loop_frames_walked": walked, "parent_host_loop_ms": round(t_parent, 3),
           "flipped_frame_reported": flip}
    vm, dm = out["verify_frames_ms"]["median"], out["decode_records_ms"]["median"]
    parent_whole = t_parent * nf / walked
    out["parent_host_loop_whole_stream_ms"] = round(parent_whole, 3)                 # (== the measured time where every frame was walked)
    out["parent_over_verify"] = round(parent_whole / vm, 1)
    out["verify_over_decode"] = round(vm / dm, 3)
    out["verify_GBps"] = round(nb * bsz / vm / 1e6, 2)
    # a frame is one chain: sixteen to a wave, at most the grid's cap of waves at a time
    out["chains_in_flight"] = min(nf, 16 * eng.resident_waves(True))
    out["verify_MBps_per_chain"] = round(nb * bsz / vm / 1e3 / out["chains_in_flight"], 1)
    out["parent_MBps"] = round(walked * per_frame * bsz / t_parent / 1e3, 1)
    del d_stream, d_out
    eng.trim(); eng.close(); torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    res = {"workload": "synthetic T text, block checksums, streams of frames around the records plz4hip_dev_encode_body wrote, real content "
                       "checksums, resident in device memory; kernels: one call per device-event window; parent: per frame "
                       "plz4hip_xxh32_stream_reset, plz4hip_dev_xxh32_stream_update per block, plz4hip_xxh32_stream_sum and a compare, from "
                       "a Python loop, a host clock around the stream",
           "reps": {"verify": REPS, "index": REPS, "decode": DEC_REPS, "parent_host_loop": 1}, "runs": []}
    for shape in SHAPES:
        res["runs"].append(measure(*shape))
        sys.stderr.write(json.dumps(res["runs"][-1]) + "\n")
    txt = json.dumps(res, indent=1)
    print(txt)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(txt + "\n")
