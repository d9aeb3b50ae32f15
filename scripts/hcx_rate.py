"""Blocks of at most 4 KiB under a dictionary context at the HC levels the wave-wide parser is built for (k_hcx, levels 2..12)
against the one-thread parsers it replaces (PLZ4HIP_HCX=0): 4096 blocks of 4096 bytes and 4096 blocks of 512 bytes of text under a
64 KiB text dictionary, levels 2, 3, 6, 9, 10, 12.  Timed: plz4hip_dev_encode_records_ex on the gapped stride (the kernels alone, stream
synchronised) and plz4hip_compress_batch_dict through host memory (staging copies included), warm, best of three calls.  "on": the
default, "off": PLZ4HIP_HCX=0; fresh processes, the two sides alternating, RUNS a side.  The real liblz4 on one host thread over the
same blocks (oracle/_ref, when built) is measured on the machine the script runs on and stored beside them.
    python scripts/hcx_rate.py [out.json]"""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

LEVELS = tuple(int(x) for x in os.environ.get("HCX_RATE_LEVELS", "2,3,6,9,10,12").split(","))
SIZES = (4096, 512)
NB = int(os.environ.get("HCX_RATE_BLOCKS", "4096"))
RUNS = 3
PAD = 65536


def inputs():
    from plz4_amd import synth
    t = synth.text(65536 + NB * 4096, seed=77)
    return np.ascontiguousarray(t[:65536]), t[65536:]


def measure():
    import torch
    from plz4_amd._native import Engine
    user, pool = inputs()
    eng = Engine(0)
    d = eng.dict_create(user)
    dev = torch.device("cuda:0")
    out = {"hcx": os.environ.get("PLZ4HIP_HCX", "default"), "kernels_ms": {}, "host_ms": {}, "hcx_blocks": {}, "sha": {}}
    import hashlib
    for bs in SIZES:
        srcs = [np.ascontiguousarray(pool[i * 4096:i * 4096 + bs]) for i in range(NB)]
        caps = [bs + bs // 255 + 16] * NB
        stride = bs + 65536
        host = np.zeros(PAD + NB * stride + 256, np.uint8)
        for i, s in enumerate(srcs):
            host[PAD + i * stride:PAD + i * stride + bs] = s
        d_src = torch.from_numpy(host).to(dev)
        sstride = eng.stage_stride(bs)
        d_stage = torch.zeros(NB * sstride + 64, dtype=torch.uint8, device=dev)
        d_len = torch.zeros(NB, dtype=torch.int32, device=dev)
        st = torch.cuda.current_stream().cuda_stream
        for lvl in LEVELS:
            key = "%d/%d" % (bs, lvl)
            c0 = eng.counters()
            best_k = best_h = 1e9
            for rep in range(4):                                 # (the first call warms up)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.dev_encode_records_ex(d_src.data_ptr() + PAD, NB * bs, stride, bs, False, d_stage.data_ptr(), d_len.data_ptr(),
                                          linked=False, d=d, stream=st, level=lvl)
                torch.cuda.synchronize()
                if rep: best_k = min(best_k, time.perf_counter() - t0)
            for rep in range(4):
                t0 = time.perf_counter()
                res, outs = eng.compress_batch_dict(srcs, caps, d, level=lvl)
                if rep: best_h = min(best_h, time.perf_counter() - t0)
            c1 = eng.counters()
            h = hashlib.sha256()
            for o in outs: h.update(o.tobytes())
            out["kernels_ms"][key] = round(best_k * 1e3, 3)
            out["host_ms"][key] = round(best_h * 1e3, 3)
            out["hcx_blocks"][key] = (c1.get("hcx_blocks", 0) - c0.get("hcx_blocks", 0)) // 8
            out["sha"][key] = h.hexdigest()[:16]
    eng.dict_destroy(d)
    eng.close()
    return out


def host_reference():
    """The real liblz4, one thread, the same blocks: MiB/s per size and level (None when oracle/_ref is not built)."""
    import orclib
    if not os.path.exists(orclib.REF_SO):
        return None
    ref = orclib.Ref()
    user, pool = inputs()
    out = {}
    for bs in SIZES:
        srcs = [np.ascontiguousarray(pool[i * 4096:i * 4096 + bs]) for i in range(NB)]
        cap = bs + bs // 255 + 16
        for lvl in LEVELS:
            keep, daddr = ref.new_dict_ctx_hc(user, lvl)
            comp = ref.stream_ctx_hc(lvl, daddr)
            t0 = time.perf_counter()
            for s in srcs: comp(s, cap)
            out["%d/%d" % (bs, lvl)] = round(NB * bs / (1 << 20) / (time.perf_counter() - t0), 1)
    return out


if __name__ == "__main__":
    if os.environ.get("HCX_RATE_CHILD"):
        print(json.dumps(measure()))
        sys.exit(0)
    res = {"blocks": NB, "on": [], "off": []}
    for run in range(RUNS):
        for name, extra in (("on", {}), ("off", {"PLZ4HIP_HCX": "0"})):
            env = dict(os.environ, HCX_RATE_CHILD="1", **extra)
            if name == "on":
                env.pop("PLZ4HIP_HCX", None)
            p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                sys.stderr.write(p.stderr[-3000:])
                sys.exit(p.returncode)
            res[name].append(json.loads(p.stdout.strip().splitlines()[-1]))
            sys.stderr.write("run %d %s: done\n" % (run, name)); sys.stderr.flush()
    keys = list(res["on"][0]["kernels_ms"])
    res["same_bytes"] = all(r["sha"] == res["on"][0]["sha"] for r in res["on"] + res["off"])
    for what in ("kernels_ms", "host_ms"):
        res["on_beats_off_every_run_" + what] = {k: max(r[what][k] for r in res["on"]) < min(r[what][k] for r in res["off"]) for k in keys}
        res["speedup_best_" + what] = {k: round(min(r[what][k] for r in res["off"]) / min(r[what][k] for r in res["on"]), 2) for k in keys}
    res["MiBps_kernels_on"] = {k: round(NB * int(k.split("/")[0]) / (1 << 20) / (min(r["kernels_ms"][k] for r in res["on"]) * 1e-3), 1) for k in keys}
    res["MiBps_kernels_off"] = {k: round(NB * int(k.split("/")[0]) / (1 << 20) / (min(r["kernels_ms"][k] for r in res["off"]) * 1e-3), 1) for k in keys}
    res["MiBps_liblz4_one_host_thread"] = host_reference()
    txt = json.dumps(res, indent=1)
    print(txt)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(txt + "\n")
