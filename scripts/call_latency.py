"""Time per call of the two few-block calls a millisecond of kernels long, where the host's share of a call can show: a one-block
4 MiB level-1 encode (plz4hip_dev_compress, the few-block parse) and the raw decode of its output (plz4hip_dev_decompress, the
few-block decoder), device-resident, warm.  Per call, CALLS calls each followed by a synchronise:
    host_us   until the call returns: planning, reserving, binding and the launches themselves
    dev_us    HIP events around the call
    call_us   until the synchronise returns
and back to back, one synchronise at the end: stream_us per call.  Means and medians; the library is this tree's or PLZ4HIP_LIB's (a build of the parent commit).
    python scripts/call_latency.py [out.json]"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

CALLS, WARM = 300, 20


def main():
    from plz4_amd import _native, synth
    if os.environ.get("PLZ4HIP_LIB"):
        _native.LIB_PATH = os.environ["PLZ4HIP_LIB"]
    import torch
    eng = _native.Engine(0)
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream()
    bsz = 4 << 20
    plain = synth.text(bsz, seed=7)
    bound = bsz + bsz // 255 + 16
    d_plain = torch.from_numpy(plain).to(dev)
    d_comp = torch.zeros(bound + 64, dtype=torch.uint8, device=dev)
    d_back = torch.zeros(bsz + 64, dtype=torch.uint8, device=dev)
    d_len = torch.tensor([bsz], dtype=torch.int32, device=dev); d_cap = torch.tensor([bound], dtype=torch.int32, device=dev)
    d_res = torch.zeros(1, dtype=torch.int32, device=dev)

    def encode():
        eng._chk(eng.L.plz4hip_dev_compress(eng.h, 1, d_plain.data_ptr(), bsz, d_len.data_ptr(), d_comp.data_ptr(), bound, d_cap.data_ptr(),
                                            1, bsz, d_res.data_ptr(), s.cuda_stream))
    encode(); torch.cuda.synchronize()
    n = int(d_res.item())
    assert 0 < n < bsz
    d_clen = torch.tensor([n], dtype=torch.int32, device=dev); d_bcap = torch.tensor([bsz + 8], dtype=torch.int32, device=dev)
    d_bres = torch.zeros(1, dtype=torch.int32, device=dev)

    def decode():
        eng.dev_decompress(1, d_comp.data_ptr(), n, d_clen.data_ptr(), d_back.data_ptr(), bsz + 8, d_bcap.data_ptr(), d_bres.data_ptr(), s.cuda_stream)
    decode(); torch.cuda.synchronize()
    assert int(d_bres.item()) == bsz and np.array_equal(d_back[:bsz].cpu().numpy(), plain)

    out = {"lib": "a build of the parent commit" if os.environ.get("PLZ4HIP_LIB") else "this tree", "calls": CALLS, "compressed": n}
    for name, call in (("encode_l1_1x4MiB", encode), ("decode_raw_1x4MiB", decode)):
        for _ in range(WARM):
            call()
        torch.cuda.synchronize()
        host, devt, whole = [], [], []
        for _ in range(CALLS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter(); e0.record(s); t1 = time.perf_counter()
            call()
            t2 = time.perf_counter(); e1.record(s); torch.cuda.synchronize(); t3 = time.perf_counter()
            host.append((t2 - t1) * 1e6); devt.append(e0.elapsed_time(e1) * 1e3); whole.append((t3 - t0) * 1e6)
        t0 = time.perf_counter()
        for _ in range(CALLS):
            call()
        torch.cuda.synchronize()
        stream = (time.perf_counter() - t0) * 1e6 / CALLS
        out[name] = {k: {"mean": round(statistics.fmean(v), 1), "median": round(statistics.median(v), 1)}
                     for k, v in (("host_us", host), ("dev_us", devt), ("call_us", whole))}
        out[name]["stream_us"] = round(stream, 1)
    c = eng.counters()
    assert c["fx_blocks"] > CALLS and c["dx_blocks"] > CALLS, c          # both calls took the few-block paths
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
