"""The few-block level-1 encode path (lz4_fx_device.inl) against one wave per block: plz4hip_compress_batch of 1 .. 256 blocks of
4 MiB text through host buffers (staging copies and PCIe included, warm), and the kernels alone on device-resident blocks
(plz4hip_dev_compress, HIP events).  "fx": the path forced on for every size (PLZ4HIP_FX_MAX_BLOCKS large), "off": the same in a
second process with PLZ4HIP_FX_MAX_BLOCKS=0 (the one-wave parse).  Where the two cross is the default of PLZ4HIP_FX_MAX_BLOCKS.
    python scripts/fx_rate.py [out.json]"""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

SIZES = (1, 4, 16, 64, 128, 192, 256)


def measure():
    import torch
    from plz4_amd import synth
    from plz4_amd._native import Engine
    import orclib
    bsz = 4 << 20
    orc = orclib.Oracle()
    pool = synth.text(16 * bsz)
    blocks = [np.ascontiguousarray(pool[i * bsz:(i + 1) * bsz]) for i in range(16)]
    bound = orc.bound(bsz)
    want = [orc.compress_fast(b, bound) for b in blocks]
    eng = Engine(0)
    out = {"fx_max_blocks": os.environ.get("PLZ4HIP_FX_MAX_BLOCKS", "default"), "piece_kib": os.environ.get("PLZ4HIP_FX_PIECE_KIB", "default"),
           "warmup_kib": os.environ.get("PLZ4HIP_FX_WARMUP_KIB", "default"), "host_buffers_ms": {}, "device_resident_ms": {}, "rounds": {}}
    dev = torch.device("cuda:0")
    for nb in SIZES:
        srcs = [blocks[i % 16] for i in range(nb)]
        best = 1e9
        for rep in range(3):
            t0 = time.perf_counter()
            res, outs = eng.compress_batch(srcs, [bound] * nb)
            best = min(best, time.perf_counter() - t0)
        for i in (0, nb - 1):
            assert int(res[i]) == want[i % 16][0] and np.array_equal(outs[i], want[i % 16][1][:int(res[i])])
        out["host_buffers_ms"][str(nb)] = round(best * 1e3, 2)
        out["rounds"][str(nb)] = eng.counters()["fx_rounds_last"]
        stride = bsz + 64
        d_src = torch.zeros(nb * stride, dtype=torch.uint8, device=dev)
        for i, b in enumerate(srcs): d_src[i * stride:i * stride + bsz] = torch.from_numpy(b).to(dev)
        d_len = torch.full((nb,), bsz, dtype=torch.int32, device=dev)
        d_cap = torch.full((nb,), bound, dtype=torch.int32, device=dev)
        d_dst = torch.zeros(nb * (bound + 64), dtype=torch.uint8, device=dev)
        d_res = torch.zeros(nb, dtype=torch.int32, device=dev)
        s = torch.cuda.current_stream()
        best = 1e9
        for rep in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            eng._chk(eng.L.plz4hip_dev_compress(eng.h, nb, d_src.data_ptr(), stride, d_len.data_ptr(), d_dst.data_ptr(), bound + 64,
                                                d_cap.data_ptr(), 1, bsz, d_res.data_ptr(), s.cuda_stream))
            e1.record(s); torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1))
        r0 = int(d_res[nb - 1].item())
        assert r0 == want[(nb - 1) % 16][0]
        assert np.array_equal(d_dst[(nb - 1) * (bound + 64):(nb - 1) * (bound + 64) + r0].cpu().numpy(), want[(nb - 1) % 16][1][:r0])
        out["device_resident_ms"][str(nb)] = round(best, 3)
        del d_src, d_dst
        eng.trim()
    out["MiBps_host"] = {k: round(int(k) * 4 / (v * 1e-3), 1) for k, v in out["host_buffers_ms"].items()}
    out["MiBps_device"] = {k: round(int(k) * 4 / (v * 1e-3), 1) for k, v in out["device_resident_ms"].items()}
    eng.close()
    return out


if __name__ == "__main__":
    if os.environ.get("FX_RATE_CHILD"):
        print(json.dumps(measure()))
        sys.exit(0)
    res = {}
    for name, extra in (("fx", {"PLZ4HIP_FX_MAX_BLOCKS": "100000"}), ("off", {"PLZ4HIP_FX_MAX_BLOCKS": "0"})):
        env = dict(os.environ, FX_RATE_CHILD="1", **extra)
        p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-3000:])
            sys.exit(p.returncode)
        res[name] = json.loads(p.stdout.strip().splitlines()[-1])
    res["speedup_host"] = {k: round(res["off"]["host_buffers_ms"][k] / v, 2) for k, v in res["fx"]["host_buffers_ms"].items()}
    res["speedup_device"] = {k: round(res["off"]["device_resident_ms"][k] / v, 2) for k, v in res["fx"]["device_resident_ms"].items()}
    txt = json.dumps(res, indent=1)
    print(txt)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(txt + "\n")
