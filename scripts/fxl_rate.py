"""The few-block level-1 encode path for blocks with history outside the block (the kExt flavour of lz4_fx_device.inl) against one
wave per block (k_encode_rec_dict): plz4hip_encode_records_ex of 1 .. 128 linked blocks of 4 MiB text behind a 64 KiB dictionary,
through host buffers (staging copies and PCIe included, warm).  "on": the default, "off": PLZ4HIP_FX_LINKED=0; fresh processes, the
two sides alternating, RUNS a side.  The path stays on at a block count only where every "on" run beats every "off" run.
(The kernels alone: such calls have no device-resident entry point; a rocprofv3 --kernel-trace --stats run of this script's child
-- FXL_RATE_CHILD=1 FXL_RATE_SIZES=1 -- gives them, see profiles/README.md.)
    python scripts/fxl_rate.py [out.json]"""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

SIZES = tuple(int(x) for x in os.environ.get("FXL_RATE_SIZES", "1,4,16,64,128").split(","))
RUNS = 3


def measure():
    from plz4_amd import synth
    from plz4_amd._native import Engine
    import orclib
    bsz = 4 << 20
    orc = orclib.Oracle()
    user = np.ascontiguousarray(synth.text(65536, seed=77))
    pool = synth.text(16 * bsz)
    blocks = [pool[i * bsz:(i + 1) * bsz].copy() for i in range(16)]
    dctx = orc.dict_ctx(user)
    eng = Engine(0)
    d = eng.dict_create(user)
    out = {"fx_linked": os.environ.get("PLZ4HIP_FX_LINKED", "default"), "host_buffers_ms": {}, "rounds": {}, "fxl_blocks": {}}
    for nb in SIZES:
        srcs = [blocks[i % 16] for i in range(nb)]
        c0 = eng.counters()
        best = 1e9
        for rep in range(3):
            t0 = time.perf_counter()
            recs = eng.encode_records_ex(srcs, bsz, True, linked=True, d=d)
            best = min(best, time.perf_counter() - t0)
        c1 = eng.counters()
        for i in sorted({0, nb - 1}):                    # the first block against the context, the last against its predecessor's tail
            r, c = orc.compress_linked(srcs[i], bsz, None if i == 0 else srcs[i - 1][-65536:].copy(), dctx if i == 0 else None)
            assert r > 0 and recs[i][4:4 + r].tobytes() == c.tobytes(), (nb, i)
        out["host_buffers_ms"][str(nb)] = round(best * 1e3, 2)
        out["rounds"][str(nb)] = c1["fx_rounds_last"]
        out["fxl_blocks"][str(nb)] = (c1.get("fxl_blocks", 0) - c0.get("fxl_blocks", 0)) // 3     # (.get: the script also runs on trees without the path)
        eng.trim()
    out["MiBps_host"] = {k: round(int(k) * 4 / (v * 1e-3), 1) for k, v in out["host_buffers_ms"].items()}
    eng.dict_destroy(d)
    eng.close()
    return out


if __name__ == "__main__":
    if os.environ.get("FXL_RATE_CHILD"):
        print(json.dumps(measure()))
        sys.exit(0)
    res = {"on": [], "off": []}
    for run in range(RUNS):
        for name, extra in (("on", {}), ("off", {"PLZ4HIP_FX_LINKED": "0"})):
            env = dict(os.environ, FXL_RATE_CHILD="1", **extra)
            if name == "on":
                env.pop("PLZ4HIP_FX_LINKED", None)
            p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                sys.stderr.write(p.stderr[-3000:])
                sys.exit(p.returncode)
            res[name].append(json.loads(p.stdout.strip().splitlines()[-1]))
    res["on_beats_off_every_run"] = {str(k): max(r["host_buffers_ms"][str(k)] for r in res["on"]) < min(r["host_buffers_ms"][str(k)] for r in res["off"])
                                     for k in SIZES}
    res["speedup_host_best"] = {str(k): round(min(r["host_buffers_ms"][str(k)] for r in res["off"]) / min(r["host_buffers_ms"][str(k)] for r in res["on"]), 2)
                                for k in SIZES}
    txt = json.dumps(res, indent=1)
    print(txt)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(txt + "\n")
