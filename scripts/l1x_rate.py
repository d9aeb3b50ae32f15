"""Linked frames from device-resident plaintext at bulk block counts (plz4hip_dev_encode_body_ex): the staged route (k_l1x_parse +
the kSeg emit stage) against the one-kernel encoder k_encode_rec_dict (PLZ4HIP_L1X=0: the baseline), with plz4hip_dev_encode_body
on the same bytes as independent blocks (the ceiling) and plz4hip_encode_records_ex through host buffers (what a producer had
before) beside them.  Synthetic T text, linked 4 MiB blocks behind a 64 KiB dictionary, resident in device memory; 512 blocks and
the largest count the memory plan allows up to 6144.  Every call is timed with device events (the host route: a host clock around
the blocking call), warm, the median of REPS calls; the two routes alternate, twice each, every step a fresh process under its own
time limit, and the run ends at the first step that fails.  The bodies of the two routes must be the same bytes.
The bulk default (kL1xDefault, plz4hip.hip) is whichever route is faster at both block counts.
    python scripts/l1x_rate.py [out.json]"""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

BSZ = 4 << 20
POOL = 16                                    # distinct blocks, tiled over the call
COUNTS = tuple(int(x) for x in os.environ.get("L1X_RATE_COUNTS", "512,6144").split(","))
HOST_MAX = 2304                              # blocks of the host-buffer call (its output lives in host memory)
REPS = int(os.environ.get("L1X_RATE_REPS", "5"))
STEP_LIMIT = int(os.environ.get("L1X_RATE_STEP_LIMIT", "240"))
PER_BLOCK = BSZ + (BSZ + 8) + (9 * BSZ) // 4 + 4096     # plaintext, body, the level-1 workspace (2.25 bytes per byte)


def plan(nb, free):
    """the largest count <= nb that fits 70 % of the free device memory"""
    return int(min(nb, (free * 7 // 10) // PER_BLOCK))


def measure(step):
    import torch
    from plz4_amd import synth
    from plz4_amd._native import Engine
    dev = torch.device("cuda:0")
    user = np.ascontiguousarray(synth.text(65536, seed=77))
    pool = synth.text(POOL * BSZ)
    eng = Engine(0)
    d = eng.dict_create(user)
    out = {"step": step, "l1x": os.environ.get("PLZ4HIP_L1X", "default"), "ms": {}, "GiBps": {}, "blocks": {}, "body_bytes": {}, "body_sum": {}}
    free, _ = torch.cuda.mem_get_info()
    s = torch.cuda.current_stream().cuda_stream
    for want in COUNTS:
        nb = plan(want, free)
        if step == "host":
            nb = min(nb, HOST_MAX)
            srcs = [pool[(i % POOL) * BSZ:(i % POOL + 1) * BSZ] for i in range(nb)]
            times = []
            for rep in range(1 + 3):
                t0 = time.perf_counter()
                recs = eng.encode_records_ex(srcs, BSZ, True, linked=True, d=d)
                times.append((time.perf_counter() - t0) * 1e3)
            times = times[1:]
            total = sum(r.size for r in recs); bsum = 0
            del recs
        else:
            d_pool = torch.from_numpy(pool).to(dev)
            d_src = torch.empty(65536 + nb * BSZ + 256, dtype=torch.uint8, device=dev)
            d_src[:65536] = 0
            d_src[65536:65536 + nb * BSZ].view(nb, BSZ)[:] = d_pool.view(POOL, BSZ).repeat((nb + POOL - 1) // POOL, 1)[:nb]
            del d_pool
            cap = nb * (BSZ + 8)
            d_body = torch.empty(cap + 64, dtype=torch.uint8, device=dev)
            d_off = torch.zeros(nb + 1, dtype=torch.int64, device=dev); d_len = torch.zeros(nb, dtype=torch.int32, device=dev)
            src = d_src.data_ptr() + 65536

            def call():
                if step == "indie":
                    eng.dev_encode_body(src, nb * BSZ, BSZ, True, d_body.data_ptr(), cap, d_off.data_ptr(), d_len.data_ptr(), stream=s)
                else:
                    eng.dev_encode_body_ex(src, nb * BSZ, BSZ, BSZ, True, d_body.data_ptr(), cap, d_off.data_ptr(), d_len.data_ptr(),
                                           linked=True, d=d, stream=s)
            times = []
            for rep in range(2 + REPS):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); call(); e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1))
            times = times[2:]
            total = int(d_off[nb])
            assert 0 < total <= cap and int(d_len.min()) > 0
            bsum = int(d_body[:total // 8 * 8].view(torch.int64).sum())        # (wraps; the same bytes give the same sum)
            del d_src, d_body
        med = float(np.median(times))
        out["ms"][str(want)] = {"median": round(med, 2), "min": round(min(times), 2), "max": round(max(times), 2)}
        out["GiBps"][str(want)] = round(nb * BSZ / 2**30 / (med * 1e-3), 2)
        out["blocks"][str(want)] = nb; out["body_bytes"][str(want)] = total; out["body_sum"][str(want)] = bsum
        eng.trim()
        torch.cuda.empty_cache()
    eng.dict_destroy(d)
    eng.close()
    return out


if __name__ == "__main__":
    if os.environ.get("L1X_RATE_CHILD"):
        print(json.dumps(measure(os.environ["L1X_RATE_CHILD"])))
        sys.exit(0)
    steps = [("staged", {"PLZ4HIP_L1X": "1"}), ("fused", {"PLZ4HIP_L1X": "0"}), ("staged", {"PLZ4HIP_L1X": "1"}), ("fused", {"PLZ4HIP_L1X": "0"}),
             ("indie", {}), ("host", {})]
    res = {"workload": "synthetic T text, linked 4 MiB blocks behind a 64 KiB dictionary, block checksums, device-resident", "runs": []}
    for name, extra in steps:
        env = dict(os.environ, L1X_RATE_CHILD=name, **extra)
        # (every GPU step under its own time limit; the first one that fails ends the run)
        p = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True)
        if p.returncode != 0:
            sys.stderr.write("step %s: exit %d\n%s\n" % (name, p.returncode, p.stderr[-3000:]))
            sys.exit(p.returncode)
        res["runs"].append(json.loads(p.stdout.strip().splitlines()[-1]))
        sys.stderr.write("%s %s\n" % (name, json.dumps(res["runs"][-1]["ms"])))
    by = lambda n: [r for r in res["runs"] if r["step"] == n]
    for k in map(str, COUNTS):
        assert len({(r["body_bytes"][k], r["body_sum"][k]) for r in by("staged") + by("fused")}) == 1, "the two routes wrote different bodies"
    med = {n: {k: float(np.median([r["ms"][k]["median"] for r in by(n)])) for k in map(str, COUNTS)} for n in ("staged", "fused", "indie", "host")}
    res["median_ms"] = med
    res["staged_over_fused"] = {k: round(med["fused"][k] / med["staged"][k], 2) for k in map(str, COUNTS)}
    faster = {k: ("staged" if med["staged"][k] < med["fused"][k] else "fused") for k in map(str, COUNTS)}
    res["faster"] = faster
    res["bulk_default"] = faster[str(COUNTS[0])] if len(set(faster.values())) == 1 else "split by block count: see faster"
    txt = json.dumps(res, indent=1)
    print(txt)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(txt + "\n")
