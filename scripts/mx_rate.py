"""The few-block level-2 encode path (lz4_mx_device.inl) against one wave per block (k_hc_mid): level 2 on 1 .. 2048 blocks of 4 MiB
text per call, the kernels alone on device-resident blocks (plz4hip_dev_compress, device events) and the call through host buffers
(plz4hip_compress_batch, host clock around the call, which ends in a synchronise).  Three columns, one process each:
  "mx"      this tree with the path forced on at every count (PLZ4HIP_MX_MAX_BLOCKS large),
  "off"     this tree with PLZ4HIP_MX_MAX_BLOCKS=0 (today's launch),
  "parent"  a built checkout of the parent commit (--parent DIR), when given.
Every point: one warm-up call, then RUNS timed calls; median, min and max are kept, spread = max - min.  "mx" beats a column at a
count when the medians differ by more than the two spreads together; the largest count up to which that holds without a gap is the
default of PLZ4HIP_MX_MAX_BLOCKS (route.h).  --pieces: piece / warm-up choices at 1 and 128 blocks instead of the table.
    python scripts/mx_rate.py [--parent DIR] [--pieces] [--sizes 1,4,...] [out.json]"""
import json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES = (1, 4, 16, 64, 128, 256, 512, 1024, 2048)
PIECES = ((64, 256), (128, 256), (128, 320), (256, 256))
RUNS = 5


def _stat(ts):
    return {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}


def measure(tree, sizes):
    sys.path.insert(0, tree); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    from plz4_amd import synth
    from plz4_amd._native import Engine
    import orclib
    bsz = 4 << 20
    ref = orclib.Ref()
    pool = synth.text(16 * bsz)
    blocks = [np.ascontiguousarray(pool[i * bsz:(i + 1) * bsz]) for i in range(16)]
    bound = bsz + bsz // 255 + 16
    want = [ref.compress_hc(b, bound, 2) for b in blocks]
    eng = Engine(0)
    has = "mx_blocks" in Engine.COUNTERS
    out = {"tree": os.path.relpath(tree, ROOT), "mx_max_blocks": os.environ.get("PLZ4HIP_MX_MAX_BLOCKS", "default"),
           "piece_kib": os.environ.get("PLZ4HIP_MX_PIECE_KIB", "default"), "warmup_kib": os.environ.get("PLZ4HIP_MX_WARMUP_KIB", "default"),
           "device_resident_ms": {}, "host_buffers_ms": {}, "mx_blocks": {}, "rounds": {}, "pieces_again": {}}
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream()
    for nb in sizes:
        srcs = [blocks[i % 16] for i in range(nb)]
        stride = bsz + 64
        d_src = torch.zeros(nb * stride, dtype=torch.uint8, device=dev)
        d_blk = [torch.from_numpy(b).to(dev) for b in blocks]
        for i in range(nb): d_src[i * stride:i * stride + bsz] = d_blk[i % 16]
        del d_blk
        d_len = torch.full((nb,), bsz, dtype=torch.int32, device=dev)
        d_cap = torch.full((nb,), bound, dtype=torch.int32, device=dev)
        d_dst = torch.zeros(nb * (bound + 64), dtype=torch.uint8, device=dev)
        d_res = torch.zeros(nb, dtype=torch.int32, device=dev)
        c0 = eng.counters()
        ts = []
        for rep in range(RUNS + 1):                                        # (the first call warms up: code objects, workspaces)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            eng._chk(eng.L.plz4hip_dev_compress(eng.h, nb, d_src.data_ptr(), stride, d_len.data_ptr(), d_dst.data_ptr(), bound + 64,
                                                d_cap.data_ptr(), 2, bsz, d_res.data_ptr(), s.cuda_stream))
            e1.record(s); torch.cuda.synchronize()
            if rep: ts.append(e0.elapsed_time(e1))
        c1 = eng.counters()
        for i in (0, nb - 1):
            r = int(d_res[i].item())
            assert r == want[i % 16][0]
            assert np.array_equal(d_dst[i * (bound + 64):i * (bound + 64) + r].cpu().numpy(), want[i % 16][1][:r])
        out["device_resident_ms"][str(nb)] = _stat(ts)
        if has:
            out["mx_blocks"][str(nb)] = (c1["mx_blocks"] - c0["mx_blocks"]) // (RUNS + 1)
            out["rounds"][str(nb)] = c1["mx_rounds_last"]
            out["pieces_again"][str(nb)] = (c1["mx_pieces_again"] - c0["mx_pieces_again"]) // (RUNS + 1)
        del d_src, d_dst
        ts = []
        for rep in range(RUNS + 1):
            t0 = time.perf_counter()
            res, outs = eng.compress_batch(srcs, [bound] * nb, level=2)
            if rep: ts.append((time.perf_counter() - t0) * 1e3)
        for i in (0, nb - 1):
            assert int(res[i]) == want[i % 16][0] and np.array_equal(outs[i], want[i % 16][1][:int(res[i])])
        out["host_buffers_ms"][str(nb)] = _stat(ts)
        del res, outs
        eng.trim()
    eng.close()
    return out


def child(name, tree, sizes, extra):
    env = dict(os.environ, MX_RATE_CHILD=tree, MX_RATE_SIZES=",".join(map(str, sizes)), **extra)
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=1100)
    if p.returncode != 0:
        sys.stderr.write("%s: %s\n" % (name, p.stderr[-3000:]))
        sys.exit(p.returncode)
    return json.loads(p.stdout.strip().splitlines()[-1])


def beats(a, b):
    """per count: a's median below b's by more than the two spreads together"""
    return {k: bool(b[k]["median"] - v["median"] > (v["max"] - v["min"]) + (b[k]["max"] - b[k]["min"])) for k, v in a.items()}


if __name__ == "__main__":
    if os.environ.get("MX_RATE_CHILD"):
        print(json.dumps(measure(os.environ["MX_RATE_CHILD"], [int(x) for x in os.environ["MX_RATE_SIZES"].split(",")])))
        sys.exit(0)
    args = sys.argv[1:]
    parent = None
    sizes = list(SIZES)
    if "--parent" in args: i = args.index("--parent"); parent = os.path.abspath(args[i + 1]); del args[i:i + 2]
    if "--sizes" in args: i = args.index("--sizes"); sizes = [int(x) for x in args[i + 1].split(",")]; del args[i:i + 2]
    pieces = "--pieces" in args
    if pieces: args.remove("--pieces")
    res = {"runs_per_point": RUNS}
    if pieces:
        for pk, wk in PIECES:
            res["%d/%d" % (pk, wk)] = child("pieces", ROOT, (1, 128), {"PLZ4HIP_MX_MAX_BLOCKS": "100000", "PLZ4HIP_MX_PIECE_KIB": str(pk), "PLZ4HIP_MX_WARMUP_KIB": str(wk)})
    else:
        res["mx"] = child("mx", ROOT, sizes, {"PLZ4HIP_MX_MAX_BLOCKS": "100000"})
        res["off"] = child("off", ROOT, sizes, {"PLZ4HIP_MX_MAX_BLOCKS": "0"})
        cols = ["off"]
        if parent:
            res["parent"] = child("parent", parent, sizes, {})
            cols.append("parent")
        for c in cols:
            for kind in ("device_resident_ms", "host_buffers_ms"):
                res["speedup_%s_over_%s" % (kind[:-3], c)] = {k: round(res[c][kind][k]["median"] / v["median"], 2) for k, v in res["mx"][kind].items()}
                res["mx_beats_%s_%s" % (c, kind[:-3])] = beats(res["mx"][kind], res[c][kind])
    txt = json.dumps(res, indent=1)
    print(txt)
    if args:
        with open(args[0], "w") as f:
            f.write(txt + "\n")
