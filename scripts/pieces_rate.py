"""The two level-1 few-block paths (lz4_fx_device.inl) at their defaults, for comparing two builds of the engine point by point:
what scripts/fx_rate.py ("fx": independent 4 MiB text blocks, dev_compress by device events and compress_batch by the host clock)
and scripts/fxl_rate.py ("fxl": linked blocks behind a 64 KiB dictionary, encode_records_ex by the host clock) time, with one
warm-up call and then RUNS timed calls a point; median, min and max are kept (spread = max - min), and per call the path's
counters: blocks it encoded, rounds of the last call, pieces parsed again.  Two builds agree at a point when their medians differ
by no more than the two spreads together (the rule of scripts/mx_rate.py, which does the same for level 2 with --parent).
    python scripts/pieces_rate.py fx|fxl [--tree DIR] [--sizes 1,16,128] [out.json]      (DIR: a built checkout; default this one)"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = 5


def _stat(ts):
    return {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}


def measure(kind, tree, sizes):
    sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, tree)
    import numpy as np
    import torch
    from plz4_amd import synth
    from plz4_amd._native import Engine
    import orclib
    bsz = 4 << 20
    orc = orclib.Oracle()
    pool = synth.text(16 * bsz)
    blocks = [np.ascontiguousarray(pool[i * bsz:(i + 1) * bsz]) for i in range(16)]
    eng = Engine(0)
    out = {"kind": kind, "tree": os.path.relpath(tree, ROOT), "runs_per_point": RUNS, "blocks": {}, "rounds": {}, "pieces_again": {}}

    def counted(nb, call, key):
        c0 = eng.counters()
        ts = []
        for rep in range(RUNS + 1):                                        # (the first call warms up: code objects, workspaces)
            t = call()
            if rep: ts.append(t)
        c1 = eng.counters()
        out.setdefault(key, {})[str(nb)] = _stat(ts)
        blk = "fxl_blocks" if kind == "fxl" else "fx_blocks"
        out["blocks"][str(nb)] = (c1[blk] - c0[blk]) // (RUNS + 1)
        out["rounds"][str(nb)] = c1["fx_rounds_last"]
        out["pieces_again"][str(nb)] = (c1["fx_pieces_again"] - c0["fx_pieces_again"]) // (RUNS + 1)

    if kind == "fx":
        bound = orc.bound(bsz)
        want = [orc.compress_fast(b, bound) for b in blocks]
        dev = torch.device("cuda:0")
        s = torch.cuda.current_stream()
        for nb in sizes:
            srcs = [blocks[i % 16] for i in range(nb)]
            stride = bsz + 64
            d_src = torch.zeros(nb * stride, dtype=torch.uint8, device=dev)
            for i, b in enumerate(srcs): d_src[i * stride:i * stride + bsz] = torch.from_numpy(b).to(dev)
            d_len = torch.full((nb,), bsz, dtype=torch.int32, device=dev)
            d_cap = torch.full((nb,), bound, dtype=torch.int32, device=dev)
            d_dst = torch.zeros(nb * (bound + 64), dtype=torch.uint8, device=dev)
            d_res = torch.zeros(nb, dtype=torch.int32, device=dev)

            def kernels():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                eng._chk(eng.L.plz4hip_dev_compress(eng.h, nb, d_src.data_ptr(), stride, d_len.data_ptr(), d_dst.data_ptr(), bound + 64,
                                                    d_cap.data_ptr(), 1, bsz, d_res.data_ptr(), s.cuda_stream))
                e1.record(s); torch.cuda.synchronize()
                return e0.elapsed_time(e1)
            counted(nb, kernels, "device_resident_ms")
            for i in (0, nb - 1):
                r = int(d_res[i].item())
                assert r == want[i % 16][0]
                assert np.array_equal(d_dst[i * (bound + 64):i * (bound + 64) + r].cpu().numpy(), want[i % 16][1][:r])
            del d_src, d_dst
            got = {}

            def host():
                t0 = time.perf_counter()
                got["res"], got["outs"] = eng.compress_batch(srcs, [bound] * nb)
                return (time.perf_counter() - t0) * 1e3
            counted(nb, host, "host_buffers_ms")
            for i in (0, nb - 1):
                assert int(got["res"][i]) == want[i % 16][0] and np.array_equal(got["outs"][i], want[i % 16][1][:int(got["res"][i])])
            eng.trim()
    else:
        user = np.ascontiguousarray(synth.text(65536, seed=77))
        dctx = orc.dict_ctx(user)
        d = eng.dict_create(user)
        for nb in sizes:
            srcs = [blocks[i % 16].copy() for i in range(nb)]
            got = {}

            def host():
                t0 = time.perf_counter()
                got["recs"] = eng.encode_records_ex(srcs, bsz, True, linked=True, d=d)
                return (time.perf_counter() - t0) * 1e3
            counted(nb, host, "host_buffers_ms")
            for i in sorted({0, nb - 1}):                # the first block against the context, the last against its predecessor's tail
                r, c = orc.compress_linked(srcs[i], bsz, None if i == 0 else srcs[i - 1][-65536:].copy(), dctx if i == 0 else None)
                assert r > 0 and got["recs"][i][4:4 + r].tobytes() == c.tobytes(), (nb, i)
            eng.trim()
        eng.dict_destroy(d)
    eng.close()
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    tree, sizes = ROOT, [1, 16, 128]
    if "--tree" in args: i = args.index("--tree"); tree = os.path.abspath(args[i + 1]); del args[i:i + 2]
    if "--sizes" in args: i = args.index("--sizes"); sizes = [int(x) for x in args[i + 1].split(",")]; del args[i:i + 2]
    txt = json.dumps(measure(args[0], tree, sizes), indent=1)
    print(txt)
    if len(args) > 1:
        with open(args[1], "w") as f:
            f.write(txt + "\n")
