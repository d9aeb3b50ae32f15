"""Chain and lists of few blocks built in pieces (lz4hc_lists_device.inl, k_hb_count .. k_hb_chain) against one wave per block
(k_hc12_hist + k_hc12_chain): levels 3 and 9 on 1 .. 512 blocks of 4 MiB text per call, level 12 on 1 and 16 blocks (its search
dominates), the kernels alone on device-resident blocks (plz4hip_dev_compress, device events) and the call through host buffers
(plz4hip_compress_batch, host clock around the call, which ends in a synchronise).  Three columns, a fresh process per column and
level, the columns taking turns:
  "hb"      this tree with the path forced on at every count (PLZ4HIP_HB_MAX_BLOCKS large),
  "off"     this tree with PLZ4HIP_HB_MAX_BLOCKS=0 (today's builder),
  "parent"  a built checkout of the parent commit (--parent DIR), when given.
Every point: one warm-up call, then RUNS timed calls; median, min and max are kept, spread = max - min.  "hb" beats a column at a
count when the medians differ by more than the two spreads together; the default of PLZ4HIP_HB_MAX_BLOCKS (route.h) is the largest
count up to which that holds without a gap at level 3, kernels alone and through host buffers, without losing at level 9.
--pieces: pieces of 16, 32, 64 and 128 KiB at 1 and 64 blocks, level 3, instead of the table; the default piece is the fastest at
1 block that stays within a fifth of the fastest at 64 blocks.
    python scripts/hb_rate.py [--parent DIR] [--pieces] [--sizes 1,2,...] [--levels 3,9,12] [out.json]"""
import json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES = (1, 2, 4, 8, 16, 32, 64, 128, 256, 512)
SIZES_12 = (1, 16)
LEVELS = (3, 9, 12)
PIECES = (16, 32, 64, 128)
RUNS = 5


def _stat(ts):
    return {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}


def measure(tree, level, sizes):
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
    want = {}

    def check(i, r, got):                                                  # block i of the pool against the real liblz4
        if i not in want: want[i] = ref.compress_hc(blocks[i], bound, level)
        assert r == want[i][0] and np.array_equal(got(r), want[i][1][:r]), (level, i)
    eng = Engine(0)
    has = "hb_blocks" in Engine.COUNTERS
    out = {"tree": "this tree" if os.path.abspath(tree) == ROOT else "parent commit", "level": level, "hb_max_blocks": os.environ.get("PLZ4HIP_HB_MAX_BLOCKS", "default"),
           "piece_kib": os.environ.get("PLZ4HIP_HB_PIECE_KIB", "default"), "device_resident_ms": {}, "host_buffers_ms": {}, "hb_blocks": {}, "pieces": {}}
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
                                                d_cap.data_ptr(), level, bsz, d_res.data_ptr(), s.cuda_stream))
            e1.record(s); torch.cuda.synchronize()
            if rep: ts.append(e0.elapsed_time(e1))
        c1 = eng.counters()
        for i in {0, nb - 1}:
            check(i % 16, int(d_res[i].item()), lambda r: d_dst[i * (bound + 64):i * (bound + 64) + r].cpu().numpy())
        out["device_resident_ms"][str(nb)] = _stat(ts)
        if has:
            out["hb_blocks"][str(nb)] = (c1["hb_blocks"] - c0["hb_blocks"]) // (RUNS + 1)
            out["pieces"][str(nb)] = c1["hb_pieces_last"]
        del d_src, d_dst
        ts = []
        for rep in range(RUNS + 1):
            t0 = time.perf_counter()
            res, outs = eng.compress_batch(srcs, [bound] * nb, level=level)
            if rep: ts.append((time.perf_counter() - t0) * 1e3)
        for i in {0, nb - 1}:
            check(i % 16, int(res[i]), lambda r: outs[i])
        out["host_buffers_ms"][str(nb)] = _stat(ts)
        del res, outs
        eng.trim()
    eng.close()
    return out


def child(name, tree, level, sizes, extra):
    env = dict(os.environ, HB_RATE_CHILD=tree, HB_RATE_LEVEL=str(level), HB_RATE_SIZES=",".join(map(str, sizes)), **extra)
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=1100)
    if p.returncode != 0:
        sys.stderr.write("%s level %d: %s\n" % (name, level, p.stderr[-3000:]))
        sys.exit(p.returncode)
    sys.stderr.write("%s level %d done\n" % (name, level)); sys.stderr.flush()
    return json.loads(p.stdout.strip().splitlines()[-1])


def beats(a, b):
    """per count: a's median below b's by more than the two spreads together"""
    return {k: bool(b[k]["median"] - v["median"] > (v["max"] - v["min"]) + (b[k]["max"] - b[k]["min"])) for k, v in a.items()}


if __name__ == "__main__":
    if os.environ.get("HB_RATE_CHILD"):
        print(json.dumps(measure(os.environ["HB_RATE_CHILD"], int(os.environ["HB_RATE_LEVEL"]), [int(x) for x in os.environ["HB_RATE_SIZES"].split(",")])))
        sys.exit(0)
    args = sys.argv[1:]
    parent = None
    sizes, levels = list(SIZES), list(LEVELS)
    if "--parent" in args: i = args.index("--parent"); parent = os.path.abspath(args[i + 1]); del args[i:i + 2]
    if "--sizes" in args: i = args.index("--sizes"); sizes = [int(x) for x in args[i + 1].split(",")]; del args[i:i + 2]
    if "--levels" in args: i = args.index("--levels"); levels = [int(x) for x in args[i + 1].split(",")]; del args[i:i + 2]
    pieces = "--pieces" in args
    if pieces: args.remove("--pieces")
    res = {"runs_per_point": RUNS}
    if pieces:
        for pk in PIECES:
            res[str(pk)] = child("pieces %d" % pk, ROOT, 3, (1, 64), {"PLZ4HIP_HB_MAX_BLOCKS": "100000", "PLZ4HIP_HB_PIECE_KIB": str(pk)})
    else:
        for level in levels:
            sz = [n for n in sizes if level < 12 or n in SIZES_12]
            r = res["level_%d" % level] = {}
            r["hb"] = child("hb", ROOT, level, sz, {"PLZ4HIP_HB_MAX_BLOCKS": "100000"})
            r["off"] = child("off", ROOT, level, sz, {"PLZ4HIP_HB_MAX_BLOCKS": "0"})
            cols = ["off"]
            if parent:
                r["parent"] = child("parent", parent, level, sz, {})
                cols.append("parent")
            for c in cols:
                for kind in ("device_resident_ms", "host_buffers_ms"):
                    r["speedup_%s_over_%s" % (kind[:-3], c)] = {k: round(r[c][kind][k]["median"] / v["median"], 2) for k, v in r["hb"][kind].items()}
                    r["hb_beats_%s_%s" % (c, kind[:-3])] = beats(r["hb"][kind], r[c][kind])
            if args:                                                       # (what is measured so far, should a later level run out of time)
                with open(args[0], "w") as f:
                    f.write(json.dumps(res, indent=1) + "\n")
    txt = json.dumps(res, indent=1)
    print(txt)
    if args:
        with open(args[0], "w") as f:
            f.write(txt + "\n")
