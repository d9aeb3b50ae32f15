"""The three few-block decoders (lz4_dx_device.inl: dx, dxb, dxl) at their defaults, for comparing two builds of the engine point by
point: what scripts/dx_rate.py ("dx": 1 / 16 / 64 text blocks of 4 MiB, dev_decompress by device events and decompress_batch by the
host clock), scripts/dx_big_rate.py ("big": one raw block of 64 MiB of text, the same two calls) and scripts/dxl_group_rate.py
("dxl": one linked chain of 32 blocks of 4 MiB behind a 64 KiB dictionary, block checksums on, decode_records_ex by the host clock)
time, with one warm-up call and then RUNS timed calls a point; median, min and max are kept (spread = max - min), and per point the
path's counters (plz4hip_ctx_counters 3, 4, 5, 6, 10, 11, 12).  Two builds agree at a point when their medians differ by no more
than the two spreads together (the rule of scripts/pieces_rate.py).
    python scripts/dxt_rate.py dx|big|dxl [--tree DIR] [out.json]      (DIR: a built checkout; default this one; one process a column)"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = 5
COUNTERS = ("dx_blocks", "dxl_blocks", "dxl_rounds_last", "dxl_groups_last", "dx_big_blocks", "dx_big_rounds_last", "dx_big_runs_last")


def _stat(ts):
    return {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}


def measure(kind, tree):
    sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, tree)
    import numpy as np
    import torch
    from plz4_amd import synth
    from plz4_amd._native import Engine
    import orclib
    MIB = 1 << 20
    bsz = 4 * MIB
    orc = orclib.Oracle()
    eng = Engine(0)
    out = {"kind": kind, "tree": os.path.relpath(tree, ROOT), "runs_per_point": RUNS, "counters": {}}
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream()

    def counted(point, call, key):
        c0 = eng.counters()
        ts = []
        for rep in range(RUNS + 1):                                        # (the first call warms up: code objects, workspaces)
            t = call()
            if rep: ts.append(t)
        c1 = eng.counters()
        out.setdefault(key, {})[point] = _stat(ts)
        # counted ones per call, "last" ones as the last call left them
        out["counters"][key + ":" + point] = {k: (c1[k] if k.endswith("_last") else (c1[k] - c0[k]) // (RUNS + 1)) for k in COUNTERS}

    def raw_points(point, srcs, comps, cap):
        nb = len(comps)
        sstride = (max(c.size for c in comps) + 64 + 15) // 16 * 16; dstride = (cap + 64 + 15) // 16 * 16
        d_src = torch.zeros(nb * sstride, dtype=torch.uint8, device=dev)
        for i, c in enumerate(comps): d_src[i * sstride:i * sstride + c.size] = torch.from_numpy(c).to(dev)
        d_len = torch.tensor([c.size for c in comps], dtype=torch.int32, device=dev)
        d_cap = torch.full((nb,), cap, dtype=torch.int32, device=dev)
        d_dst = torch.zeros(nb * dstride, dtype=torch.uint8, device=dev)
        d_res = torch.zeros(nb, dtype=torch.int32, device=dev)

        def kernels():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            eng._chk(eng.L.plz4hip_dev_decompress(eng.h, nb, d_src.data_ptr(), sstride, d_len.data_ptr(), d_dst.data_ptr(), dstride,
                                                  d_cap.data_ptr(), d_res.data_ptr(), s.cuda_stream))
            e1.record(s); torch.cuda.synchronize()
            return e0.elapsed_time(e1)
        counted(point, kernels, "device_resident_ms")
        assert d_res.cpu().tolist() == [x.size for x in srcs]
        assert np.array_equal(d_dst[(nb - 1) * dstride:(nb - 1) * dstride + srcs[-1].size].cpu().numpy(), srcs[-1])
        del d_src, d_dst
        got = {}

        def host():
            t0 = time.perf_counter()
            got["res"], got["outs"] = eng.decompress_batch(comps, [cap] * nb)
            return (time.perf_counter() - t0) * 1e3
        counted(point, host, "host_buffers_ms")
        assert [int(r) for r in got["res"]] == [x.size for x in srcs] and np.array_equal(got["outs"][nb - 1], srcs[-1])
        eng.trim()

    if kind == "dx":
        pool = synth.text(16 * bsz)
        srcs = [np.ascontiguousarray(pool[i * bsz:(i + 1) * bsz]) for i in range(16)]
        comps = [np.ascontiguousarray(orc.compress_fast(x, orc.bound(bsz))[1]) for x in srcs]
        for nb in (1, 16, 64):
            raw_points(str(nb), [srcs[i % 16] for i in range(nb)], [comps[i % 16] for i in range(nb)], bsz + 8)
    elif kind == "big":
        n = 64 * MIB
        src = synth.text(n, seed=7)
        comp = np.ascontiguousarray(orc.compress_fast(src, orc.bound(n))[1])
        raw_points("T64", [src], [comp], n + 8)
    else:
        nb = 32
        pool = synth.text(32 * bsz)
        blocks = [np.ascontiguousarray(pool[i * bsz:(i + 1) * bsz]) for i in range(nb)]
        dct = np.ascontiguousarray(synth.text(65536, seed=77))
        d = eng.dict_create(dct)
        linked = [np.ascontiguousarray(r) for r in eng.encode_records_ex(blocks, bsz, True, linked=True, d=d)]
        got = {}

        def host():
            w = dct.copy()
            t0 = time.perf_counter()
            got["r"] = eng.decode_records_ex(linked, bsz, True, linked=True, window=w, window_len=65536)
            return (time.perf_counter() - t0) * 1e3
        counted(str(nb), host, "host_buffers_ms")
        assert not any(int(k) for k in got["r"][1]) and all(np.array_equal(o, x) for o, x in zip(got["r"][2], blocks))
        eng.dict_destroy(d)
    eng.close()
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    tree = ROOT
    if "--tree" in args: i = args.index("--tree"); tree = os.path.abspath(args[i + 1]); del args[i:i + 2]
    txt = json.dumps(measure(args[0], tree), indent=1)
    print(txt)
    if len(args) > 1:
        with open(args[1], "w") as f:
            f.write(txt + "\n")
