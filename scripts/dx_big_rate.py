"""Raw blocks above 4 MiB on the few-block decoder's big path (dxb_*, lz4_dx_device.inl) against one wave per block: one block of
text at 8, 64 and 256 MiB, of random bytes and of zeros at 64 MiB, through plz4hip_dev_decompress (nBlocks == 1, strides = the
compressed length and the capacity; the kernels alone, HIP events) and through plz4hip_decompress_batch (host buffers, staging and
PCIe included).  Warm, the median of about a second of repetitions (at least one), a fresh process per side, the sides alternating,
PASSES passes:
    on      the library of this tree, defaults
    off     the library of this tree, PLZ4HIP_DX_BIG=0
    parent  the library named by DX_BIG_RATE_PARENT_LIB (a build of the parent commit), when given
The bar of DESIGN 3.9b: the 256 MiB text block on the big path against the SAME text as 64 independent 4 MiB blocks in one
dev_decompress call ("t64x4" -- the few-block path as it was; taken from the parent side when there is one).  The run threshold:
the "on" side once more at PLZ4HIP_DX_BIG_RUN_KIB = 16, 64, 256 on the R and Z shapes.
    python scripts/dx_big_rate.py [out.json]"""
import json, os, statistics, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

MIB = 1 << 20
PASSES = 2
SHAPES = (("T8", "T", 8), ("T64", "T", 64), ("T256", "T", 256), ("R64", "R", 64), ("Z64", "Z", 64))


def make_inputs(d):
    """the plaintexts and their compressed blocks, written once for every child"""
    import orclib
    from plz4_amd import synth
    orc = orclib.Oracle()
    for name, kind, mib in SHAPES:
        n = mib * MIB
        src = synth.text(n, seed=7) if kind == "T" else (synth.random_bytes(n, seed=4) if kind == "R" else synth.zeros(n))
        comp = orc.compress_fast(src, orc.bound(n))[1]
        np.save(os.path.join(d, name + ".plain.npy"), src); np.save(os.path.join(d, name + ".comp.npy"), np.ascontiguousarray(comp))
        if name == "T256":
            parts = [np.ascontiguousarray(orc.compress_fast(src[o:o + 4 * MIB], orc.bound(4 * MIB))[1]) for o in range(0, n, 4 * MIB)]
            np.save(os.path.join(d, "T256.parts.npy"), np.concatenate(parts))
            np.save(os.path.join(d, "T256.partlen.npy"), np.array([p.size for p in parts], np.int64))


def _median_ms(call, budget=1.0, most=200):
    call()                                                       # warm: workspaces, staging
    ts = []
    t_end = time.perf_counter() + budget
    while not ts or (time.perf_counter() < t_end and len(ts) < most):
        ts.append(call())
    return round(statistics.median(ts), 3), len(ts)


def measure(d, only):
    lib = os.environ.get("DX_BIG_RATE_LIB")
    from plz4_amd import _native
    if lib:
        _native.LIB_PATH = lib
    import torch
    eng = _native.Engine(0)
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream()
    out = {"lib": "a build of the parent commit" if lib else "this tree", "dx_big": os.environ.get("PLZ4HIP_DX_BIG", "default"),
           "run_kib": os.environ.get("PLZ4HIP_DX_BIG_RUN_KIB", "default"), "dev_ms": {}, "host_ms": {}, "reps": {}}

    def dev_call(nb, d_src, sstride, d_len, d_dst, dstride, d_cap, d_res):
        def f():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            eng.dev_decompress(nb, d_src.data_ptr(), sstride, d_len.data_ptr(), d_dst.data_ptr(), dstride, d_cap.data_ptr(), d_res.data_ptr(), s.cuda_stream)
            e1.record(s); torch.cuda.synchronize()
            return e0.elapsed_time(e1)
        return f

    for name, kind, mib in SHAPES:
        if only and name not in only:
            continue
        plain = np.load(os.path.join(d, name + ".plain.npy")); comp = np.load(os.path.join(d, name + ".comp.npy"))
        n = plain.size; cap = n + 8
        d_src = torch.from_numpy(comp).to(dev)
        d_dst = torch.zeros(cap + 64, dtype=torch.uint8, device=dev)
        d_len = torch.tensor([comp.size], dtype=torch.int32, device=dev); d_cap = torch.tensor([cap], dtype=torch.int32, device=dev)
        d_res = torch.zeros(1, dtype=torch.int32, device=dev)
        out["dev_ms"][name], out["reps"][name] = _median_ms(dev_call(1, d_src, comp.size, d_len, d_dst, cap, d_cap, d_res))
        assert int(d_res.item()) == n and np.array_equal(d_dst[:n].cpu().numpy(), plain), name
        del d_src, d_dst

        def host():
            t0 = time.perf_counter()
            host.res, host.outs = eng.decompress_batch([comp], [cap])
            return (time.perf_counter() - t0) * 1e3
        out["host_ms"][name], _ = _median_ms(host)
        assert int(host.res[0]) == n and np.array_equal(host.outs[0], plain), name
        if name == "T256" and not only:
            # the same text as 64 independent 4 MiB blocks, one call: the few-block path of blocks up to 4 MiB
            parts = np.load(os.path.join(d, "T256.parts.npy")); plen = np.load(os.path.join(d, "T256.partlen.npy"))
            nb = plen.size; stride = 5 * MIB
            h = np.zeros(nb * stride, np.uint8); o = 0
            for i, ln in enumerate(plen):
                h[i * stride:i * stride + ln] = parts[o:o + ln]; o += int(ln)
            d_src = torch.from_numpy(h).to(dev); d_dst = torch.zeros(nb * stride, dtype=torch.uint8, device=dev)
            d_len = torch.tensor(plen, dtype=torch.int32, device=dev); d_cap = torch.full((nb,), 4 * MIB + 8, dtype=torch.int32, device=dev)
            d_res = torch.zeros(nb, dtype=torch.int32, device=dev)
            out["dev_ms"]["t64x4"], out["reps"]["t64x4"] = _median_ms(dev_call(nb, d_src, stride, d_len, d_dst, stride, d_cap, d_res))
            assert int(d_res.sum().item()) == n
            assert np.array_equal(d_dst[(nb - 1) * stride:(nb - 1) * stride + 4 * MIB].cpu().numpy(), plain[n - 4 * MIB:])
            del d_src, d_dst
    names = ("dx_blocks", "dx_big_blocks", "dx_big_rounds_last", "dx_big_runs_last")
    out["counters"] = {k: v for k, v in eng.counters().items() if k in names} if not lib else {}
    eng.close()
    return out


def child(env_extra, d, only=""):
    env = dict(os.environ, DX_BIG_RATE_CHILD=d, DX_BIG_RATE_ONLY=only)
    for k in ("PLZ4HIP_DX_BIG", "PLZ4HIP_DX_BIG_RUN_KIB", "DX_BIG_RATE_LIB"):
        env.pop(k, None)
    env.update(env_extra)
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:                                        # (nothing more is started on the GPU behind a failed side)
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        sys.exit(p.returncode if p.returncode > 0 else 1)
    return json.loads(p.stdout.strip().splitlines()[-1])


if __name__ == "__main__":
    if os.environ.get("DX_BIG_RATE_CHILD"):
        only = os.environ.get("DX_BIG_RATE_ONLY", "")
        print(json.dumps(measure(os.environ["DX_BIG_RATE_CHILD"], set(only.split(",")) if only else None)))
        sys.exit(0)
    parent_lib = os.environ.get("DX_BIG_RATE_PARENT_LIB")
    sides = ([("parent", {"DX_BIG_RATE_LIB": parent_lib})] if parent_lib else []) + [("on", {}), ("off", {"PLZ4HIP_DX_BIG": "0"})]
    res = {"passes": PASSES, "shapes": [s[0] for s in SHAPES]}
    for name, _ in sides:
        res[name] = []
    with tempfile.TemporaryDirectory() as d:
        make_inputs(d)
        for run in range(PASSES):
            for name, extra in sides:
                res[name].append(child(extra, d))
                sys.stderr.write("pass %d %s: done\n" % (run, name)); sys.stderr.flush()
        res["run_kib"] = {}
        for run in range(PASSES):
            for kib in ("16", "64", "256"):
                r = child({"PLZ4HIP_DX_BIG_RUN_KIB": kib}, d, only="R64,Z64")
                res["run_kib"].setdefault(kib, []).append({"dev_ms": r["dev_ms"], "host_ms": r["host_ms"], "runs_last": r["counters"].get("dx_big_runs_last")})
    keys = [s[0] for s in SHAPES]
    others = [r for name in ("off", "parent") if name in res for r in res[name]]
    for what in ("dev_ms", "host_ms"):
        res["on_beats_every_other_run_" + what] = {k: max(r[what][k] for r in res["on"]) < min(r[what][k] for r in others) for k in keys}
        res["speedup_median_" + what] = {k: round(statistics.median(r[what][k] for r in others) / statistics.median(r[what][k] for r in res["on"]), 2) for k in keys}
    base = res["parent"] if parent_lib else res["on"]
    res["bar"] = {"t256_one_block_ms": [r["dev_ms"]["T256"] for r in res["on"]], "t64x4_ms": [r["dev_ms"]["t64x4"] for r in base],
                  "t64x4_from": "parent" if parent_lib else "this tree"}
    res["bar"]["ratio"] = round(max(res["bar"]["t256_one_block_ms"]) / min(res["bar"]["t64x4_ms"]), 3)
    res["bar"]["met"] = res["bar"]["ratio"] <= 1.5
    txt = json.dumps(res, indent=1)
    print(txt)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(txt + "\n")
