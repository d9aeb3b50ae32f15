"""The index of a frame body that is already on the device (plz4hip_dev_index_body, k_index_body: one wavefront, one dependent load
per record) beside what a caller did without it -- the host chasing the chain of size words with one 4-byte device-to-host copy per
record (hipMemcpy through ctypes, a Python loop around it) -- and beside plz4hip_dev_decode_records of the same body, which is what
the index is there to feed.  Two bodies, both written by plz4hip_dev_encode_body from synthetic T text with block checksums and
resident in device memory: 6144 records of 4 MiB blocks (the benchmark's shape; fewer where the memory does not hold them) and 65536
records of 64 KiB blocks.  The kernels are timed with device events, warm, one call per window, the median of REPS windows (minimum
and maximum beside it); the host walk with a host clock around the whole chain, the median of HOST_REPS walks.  The index must
reproduce the encoder's recOff.  No threshold: the comparison is between the three numbers.
    python scripts/index_rate.py [out.json]"""
import ctypes as C
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

POOL = 16                                    # distinct blocks, tiled over the body
SHAPES = (("4MiB_x6144", 4 << 20, 6144), ("64KiB_x65536", 64 << 10, 65536))
REPS = int(os.environ.get("INDEX_RATE_REPS", "20"))
HOST_REPS = int(os.environ.get("INDEX_RATE_HOST_REPS", "3"))
DEC_REPS = int(os.environ.get("INDEX_RATE_DEC_REPS", "5"))


def hip_runtime():
    """the HIP runtime this process already has (torch's), for hipMemcpy as a C caller would call it"""
    for name in ("libamdhip64.so.7", "libamdhip64.so.6", "libamdhip64.so"):
        try:
            L = C.CDLL(name)
        except OSError:
            continue
        L.hipMemcpy.restype = C.c_int
        L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        return L
    raise RuntimeError("no HIP runtime to call hipMemcpy from")


def stats(times):
    return {"median": round(float(np.median(times)), 3), "min": round(min(times), 3), "max": round(max(times), 3)}


def timed(call, warm, reps):
    import torch
    out = []
    for rep in range(warm + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out[warm:]


def host_walk(hip, body_ptr, body_bytes, bsz, checksum, max_blocks):
    """FrameReader._read's chain from the host: four bytes per hipMemcpy, one round trip per record -> the offsets"""
    word = C.c_uint32(0)
    off, offs = 0, []
    tail = 8 if checksum else 4
    while off != body_bytes and body_bytes - off >= 4 and len(offs) < max_blocks:
        if hip.hipMemcpy(C.byref(word), body_ptr + off, 4, 2) != 0:                       # 2: hipMemcpyDeviceToHost
            raise RuntimeError("hipMemcpy")
        size = word.value & 0x7FFFFFFF
        if word.value == 0 or size > bsz or size + tail > body_bytes - off:
            break
        offs.append(off); off += size + tail
    offs.append(off)
    return offs


def measure(name, bsz, want_blocks):
    import torch
    from plz4_amd import synth
    from plz4_amd._native import Engine, BODY_END_OF_BYTES
    dev = torch.device("cuda:0")
    hip = hip_runtime()
    eng = Engine(0)
    free, _ = torch.cuda.mem_get_info()
    per_block = bsz + (bsz + 8) + bsz + (9 * bsz) // 4 + 64             # plaintext, body, decoded output, the level-1 workspace
    nb = int(min(want_blocks, (free * 7 // 10) // per_block))
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
    body_bytes = int(d_enc_off[nb])
    assert 0 < body_bytes <= cap
    del d_src
    eng.trim(); torch.cuda.empty_cache()
    # the index kernel alone
    d_off = torch.full((nb + 1,), -1, dtype=torch.int64, device=dev); d_info = torch.zeros(2, dtype=torch.int64, device=dev)
    t_index = timed(lambda: eng.dev_index_body(d_body.data_ptr(), body_bytes, bsz, True, nb, d_off.data_ptr(), d_info.data_ptr(), s), 3, REPS)
    info = d_info.cpu().numpy()
    assert int(info[0]) == body_bytes and tuple(int(x) for x in info[1:2].view(np.int32)) == (nb, BODY_END_OF_BYTES)
    assert torch.equal(d_off, d_enc_off), "the index is not the encoder's recOff"
    # what a caller does today: the chain from the host
    t_host = []
    enc_off = d_enc_off.cpu().numpy()
    for rep in range(1 + HOST_REPS):
        t0 = time.perf_counter()
        offs = host_walk(hip, d_body.data_ptr(), body_bytes, bsz, True, nb)
        t_host.append((time.perf_counter() - t0) * 1e3)
        assert len(offs) == nb + 1 and np.array_equal(np.asarray(offs, dtype=np.int64), enc_off)
    t_host = t_host[1:]
    # the decode the index feeds
    d_out = torch.empty(nb * bsz, dtype=torch.uint8, device=dev)
    d_res = torch.zeros(nb, dtype=torch.int32, device=dev); d_st = torch.zeros(nb, dtype=torch.int32, device=dev)
    t_dec = timed(lambda: eng.dev_decode_records(d_body.data_ptr(), d_off.data_ptr(), nb, bsz, True, d_out.data_ptr(), bsz, bsz,
                                                 d_res.data_ptr(), d_st.data_ptr(), s), 2, DEC_REPS)
    assert int(d_st.abs().sum()) == 0 and int(d_res.to(torch.int64).sum()) == nb * bsz
    out = {"shape": name, "bsz": bsz, "blocks": nb, "blocks_wanted": want_blocks, "body_bytes": body_bytes,
           "index_kernel_ms": stats(t_index), "host_walk_ms": stats(t_host), "decode_records_ms": stats(t_dec)}
    im, hm, dm = (out[k]["median"] for k in ("index_kernel_ms", "host_walk_ms", "decode_records_ms"))
    out["index_us_per_record"] = round(im * 1e3 / nb, 3)
    out["host_walk_us_per_record"] = round(hm * 1e3 / nb, 3)
    out["host_walk_over_index"] = round(hm / im, 1)
    out["index_over_decode"] = round(im / dm, 3)
    del d_body, d_out
    eng.trim(); eng.close(); torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    res = {"workload": "synthetic T text, block checksums, the body plz4hip_dev_encode_body wrote, resident in device memory; "
                       "index: one call per device-event window; host walk: hipMemcpy of 4 bytes per record from a Python loop",
           "reps": {"index": REPS, "host_walk": HOST_REPS, "decode": DEC_REPS}, "runs": []}
    for name, bsz, nb in SHAPES:
        res["runs"].append(measure(name, bsz, nb))
        sys.stderr.write(json.dumps(res["runs"][-1]) + "\n")
    txt = json.dumps(res, indent=1)
    print(txt)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(txt + "\n")
