"""Whole frames around an encoded block section that is on the device (plz4hip_dev_write_frames: k_frame_edges, sixteen frames'
headers, trailers and xxh32 chains per wavefront over the plaintext; k_frame_move, one pass over the records; k_frame_summary) beside
the plz4hip_dev_encode_body it follows and beside the parent commit's way to the same bytes -- synchronise and read recOff, then per
frame a header copy, a device-to-device copy of its span, plz4hip_xxh32_stream_reset / plz4hip_dev_xxh32_stream_update per block /
plz4hip_xxh32_stream_sum (which synchronises) and a trailer copy, from a Python loop.  The streams of stream_index_rate.py and
frame_verify_rate.py from the writing side: 16384 frames of one 64 KiB block; 6144 blocks of 4 MiB as k = 1 and as k = 96 (64 frames;
fewer blocks where the memory does not hold them), each with and without the content checksum -- without it the call is the move
alone, the cost of the extra pass over the compressed bytes.  The plaintext is tiles of a pool of 16 blocks of text.  The kernels are
timed with device events, warm, one call per window, the median of the repetitions (minimum and maximum beside it); the host loop
with a host clock (FRAME_WRITE_RATE_PARENT_FRAMES walks fewer frames and says so; the whole stream is extrapolated from them).  Every
written stream is verified by index -> decode -> verify with all verdicts OK, the index's tables must be the writer's, and the
parent's bytes must be the writer's.  No threshold: the comparison is between the numbers.
    python scripts/frame_write_rate.py [out.json]"""
import ctypes as C
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np
from index_rate import stats, timed

POOL = 16
SHAPES = (("64KiB_1x16384", 64 << 10, 4, 1, 16384), ("4MiB_1x6144", 4 << 20, 7, 1, 6144), ("4MiB_96x64", 4 << 20, 7, 96, 64))
REPS = int(os.environ.get("FRAME_WRITE_RATE_REPS", "5"))
ENC_REPS = int(os.environ.get("FRAME_WRITE_RATE_ENC_REPS", "3"))
PARENT_FRAMES = int(os.environ.get("FRAME_WRITE_RATE_PARENT_FRAMES", "0"))           # 0: the whole stream


def measure(name, bsz, bd_id, k, want_frames):
    import torch
    from plz4_amd import host, synth
    from plz4_amd._native import (Engine, FrameIndex, FrameVerdict, StreamIndex, StreamVerdict, WriteInfo, FRAME_OK, STREAM_END, WRITE_OK)
    dev = torch.device("cuda:0")
    eng = Engine(0)
    free, _ = torch.cuda.mem_get_info()
    per_block = bsz + 3 * (bsz + 8 + 27) + bsz + (9 * bsz) // 4 + 64    # plaintext, body, two streams, decoded output, the level-1 workspace
    nf = int(min(want_frames, (free * 7 // 10) // (per_block * k)))
    nb = nf * k
    pool = synth.text(POOL * bsz)
    d_pool = torch.from_numpy(pool).to(dev)
    d_src = torch.empty(nb * bsz, dtype=torch.uint8, device=dev)
    d_src.view(nb, bsz)[:] = d_pool.view(POOL, bsz).repeat((nb + POOL - 1) // POOL, 1)[:nb]
    del d_pool
    cap = nb * (bsz + 8)
    out_cap = cap + nf * 27
    d_body = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_off = torch.zeros(nb + 1, dtype=torch.int64, device=dev); d_len = torch.zeros(nb, dtype=torch.int32, device=dev)
    d_out = torch.empty(out_cap, dtype=torch.uint8, device=dev)
    d_tab = torch.zeros(nf * C.sizeof(FrameIndex), dtype=torch.uint8, device=dev)
    d_ooff = torch.zeros(nb + 1, dtype=torch.int64, device=dev)
    d_winfo = torch.zeros(C.sizeof(WriteInfo), dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    encode = lambda: eng.dev_encode_body(d_src.data_ptr(), nb * bsz, bsz, True, d_body.data_ptr(), cap, d_off.data_ptr(), d_len.data_ptr(), stream=s)
    t_enc = timed(encode, 1, ENC_REPS)
    enc_off = d_off.cpu().numpy()
    body_bytes = int(enc_off[nb])
    eng.trim(); torch.cuda.empty_cache()
    # for the check: index -> decode -> verify over what was written
    d_tab2 = torch.zeros((nf + 1) * C.sizeof(FrameIndex), dtype=torch.uint8, device=dev)
    d_off2 = torch.zeros(nb + 1, dtype=torch.int64, device=dev)
    d_info = torch.zeros(C.sizeof(StreamIndex), dtype=torch.uint8, device=dev)
    d_dst = torch.empty(nb * bsz, dtype=torch.uint8, device=dev)
    d_res = torch.zeros(nb, dtype=torch.int32, device=dev); d_st = torch.zeros(nb, dtype=torch.int32, device=dev)
    d_ver = torch.zeros((nf + 1) * C.sizeof(FrameVerdict), dtype=torch.uint8, device=dev)
    d_sv = torch.zeros(C.sizeof(StreamVerdict), dtype=torch.uint8, device=dev)
    d_parent = torch.empty(out_cap, dtype=torch.uint8, device=dev)
    out = {"shape": name, "bsz": bsz, "blocks_per_frame": k, "frames": nf, "frames_wanted": want_frames, "records": nb, "plaintext_bytes": nb * bsz,
           "body_bytes": body_bytes, "encode_body_ms": stats(t_enc)}
    chains = min(nf, 16 * eng.resident_waves(True))
    h = eng.hash_create()
    for cck in (True, False):
        write = lambda: eng.dev_write_frames(d_src.data_ptr(), nb * bsz, d_body.data_ptr(), cap, d_off.data_ptr(), k, d_out.data_ptr(), out_cap,
                                             d_tab.data_ptr(), d_ooff.data_ptr(), d_winfo.data_ptr(), bsz, block_checksum=True, content_checksum=cck,
                                             stream=s)
        t_w = timed(write, 2, REPS)
        t_both = timed(lambda: (encode(), write()), 1, ENC_REPS)                     # the two calls in one window, no host in between
        wi = WriteInfo.from_buffer_copy(d_winfo.cpu().numpy().tobytes())
        H, T = 7, 8 if cck else 4
        end = body_bytes + nf * (H + T)
        assert (wi.status, wi.end, wi.nFrames, wi.nRecs, wi.firstBadRec) == (WRITE_OK, end, nf, nb, -1), (wi.status, wi.end, end)
        # index -> decode -> verify: every verdict OK, and the index lists what the writer listed
        eng.dev_index_stream(d_out.data_ptr(), end, nf + 1, nb, d_tab2.data_ptr(), d_off2.data_ptr(), d_info.data_ptr(), s)
        eng.dev_decode_records(d_out.data_ptr(), d_off2.data_ptr(), nb, bsz, True, d_dst.data_ptr(), bsz, bsz, d_res.data_ptr(), d_st.data_ptr(), s)
        eng.dev_verify_frames(d_tab2.data_ptr(), d_info.data_ptr(), nf + 1, d_dst.data_ptr(), bsz, bsz, d_res.data_ptr(), d_st.data_ptr(), nb,
                              d_ver.data_ptr(), d_sv.data_ptr(), s)
        torch.cuda.synchronize()
        info = StreamIndex.from_buffer_copy(d_info.cpu().numpy().tobytes())
        sv = StreamVerdict.from_buffer_copy(d_sv.cpu().numpy().tobytes())
        assert (info.end, info.nFrames, info.nRecs, info.status) == (end, nf, nb, STREAM_END)
        assert (sv.nFrames, sv.nOk, sv.firstBadFrame, sv.status, sv.contentBytes) == (nf, nf, -1, FRAME_OK, nb * bsz), "not every frame is OK"
        assert torch.equal(d_tab, d_tab2[:d_tab.numel()]) and torch.equal(d_ooff, d_off2) and bool((d_res == bsz).all()) and not bool(d_st.any())
        # the parent commit's way to the same bytes, from the host
        header = torch.from_numpy(np.frombuffer(host.write_header(block_checksum=True, content_checksum=cck, block_size=bd_id), dtype=np.uint8).copy())
        assert header.numel() == H
        src_ptr = d_src.data_ptr()

        def parent_walk(frames):
            torch.cuda.synchronize()
            off = d_off.cpu().numpy()                                                # where the trailers go is known only here
            for f in range(frames):
                a, b = int(off[f * k]), int(off[(f + 1) * k])
                at = f * (H + T) + a
                d_parent[at:at + H].copy_(header, non_blocking=True)
                d_parent[at + H:at + H + b - a].copy_(d_body[a:b], non_blocking=True)
                trailer = np.zeros(T, dtype=np.uint8)
                if cck:
                    eng.hash_reset(h)
                    for i in range(f * k, (f + 1) * k):
                        eng.dev_hash_update(h, src_ptr + i * bsz, bsz, s)
                    trailer[4:] = np.frombuffer(int(eng.hash_sum(h)).to_bytes(4, "little"), dtype=np.uint8)
                d_parent[at + H + b - a:at + H + b - a + T].copy_(torch.from_numpy(trailer), non_blocking=True)
            torch.cuda.synchronize()

        walked = nf if PARENT_FRAMES <= 0 else min(nf, PARENT_FRAMES)
        parent_walk(1)                                                               # warm
        t0 = time.perf_counter()
        parent_walk(walked)
        t_parent = (time.perf_counter() - t0) * 1e3
        upto = int(enc_off[walked * k]) + walked * (H + T)
        assert torch.equal(d_parent[:upto], d_out[:upto]), "the parent's bytes are not the writer's"
        wm = stats(t_w)["median"]
        r = {"write_frames_ms": stats(t_w), "encode_then_write_one_window_ms": stats(t_both), "stream_bytes": end,
             "write_over_encode": round(wm / out["encode_body_ms"]["median"], 4),
             "parent_host_loop_frames_walked": walked, "parent_host_loop_ms": round(t_parent, 3),
             "parent_host_loop_whole_stream_ms": round(t_parent * nf / walked, 3), "parent_over_write": round(t_parent * nf / walked / wm, 1)}
        if cck:
            r["chains_in_flight"] = chains
            r["checksum_GBps_all_chains"] = round(nb * bsz / wm / 1e6, 2)
            r["checksum_MBps_per_chain"] = round(nb * bsz / wm / 1e3 / chains, 1)
        else:
            r["move_GBps_read_plus_write"] = round(2 * body_bytes / wm / 1e6, 2)
        out["content_checksum" if cck else "move_alone"] = r
    eng.hash_destroy(h)
    del d_src, d_body, d_out, d_dst, d_parent
    eng.trim(); eng.close(); torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    res = {"workload": "synthetic T text, block checksums, plz4hip_dev_encode_body then plz4hip_dev_write_frames on one stream, resident in device "
                       "memory; kernels: one call per device-event window; parent: synchronise, read recOff, per frame a header copy, a "
                       "device-to-device copy of its records, the streaming checksum over its blocks and a trailer copy, from a Python loop, a "
                       "host clock around the stream",
           "reps": {"write": REPS, "encode": ENC_REPS, "parent_host_loop": 1}, "runs": []}
    only = os.environ.get("FRAME_WRITE_RATE_SHAPES")
    for shape in SHAPES:
        if only and shape[0] not in only.split(","):
            continue
        res["runs"].append(measure(*shape))
        sys.stderr.write(json.dumps(res["runs"][-1]) + "\n")
        if len(sys.argv) > 1:                                                        # (after every shape: a long run leaves what it has)
            with open(sys.argv[1], "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res, indent=1))
