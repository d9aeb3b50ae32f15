"""The few-block level-2 encode path behind external segments (MxlFlavour, lz4_mx_device.inl) against one wave per block
(k_hc_mid<true>): level 2 on 1 .. 1024 linked blocks of 4 MiB text per call behind a 64 KiB dictionary, the kernels alone on
device-resident plaintext (plz4hip_dev_encode_records_ex, device events) and the call through host buffers
(plz4hip_encode_records_ex, host clock around the call, which ends in a synchronise).  Three columns, one process each:
  "mxl"     this tree with the route forced on at every count (PLZ4HIP_MXL_MAX_BLOCKS large),
  "off"     this tree with PLZ4HIP_MXL_MAX_BLOCKS=0 (one wave per block),
  "parent"  a built checkout of the parent commit (--parent DIR), when given.
Every point: one warm-up call, then RUNS timed calls; median, min and max are kept, spread = max - min.  "mxl" beats a column at a
count when the medians differ by more than the two spreads together; the largest count up to which that holds for both columns and
both kinds of call without a gap is the default of PLZ4HIP_MXL_MAX_BLOCKS (route.h; 0 when it holds at no count).
    python scripts/mxl_rate.py [--parent DIR] [--sizes 1,4,...] [--only mxl|off|parent] [out.json]
--only: one column into out.json (a later run with the same out.json adds its column and the comparison)."""
import json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES = (1, 4, 16, 64, 128, 256, 512, 1024)
RUNS = 5
KINDS = ("device_resident_ms", "host_buffers_ms")


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
    dct = np.ascontiguousarray(synth.text(65536, seed=77))
    keep, daddr = ref.new_dict_ctx_hc(dct, 2)
    # block 0 starts under the dictionary, block i > 0 behind the last 64 KiB of block i - 1 (blocks cycle through the pool of 16)
    first = ref.stream_linked_ctx_hc(2, daddr)(blocks[0], bsz, None)
    later = [ref.stream_linked_ctx_hc(2)(blocks[j], bsz, blocks[(j - 1) % 16][-65536:].copy()) for j in range(16)]
    want = lambda i: first if i == 0 else later[i % 16]
    eng = Engine(0)
    d = eng.dict_create(dct)
    has = "mxl_blocks" in Engine.COUNTERS
    out = {"mxl_max_blocks": os.environ.get("PLZ4HIP_MXL_MAX_BLOCKS", "default"),
           "device_resident_ms": {}, "host_buffers_ms": {}, "mxl_blocks": {}, "rounds": {}, "pieces_again": {}}
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream()
    sstride = eng.stage_stride(bsz)

    def check(i, rec):
        c, comp = want(i)
        assert c > 0 and int(rec[:4].view(np.uint32)[0]) == c and np.array_equal(rec[4:4 + c], comp[:c]), i

    for nb in sizes:
        sys.stderr.write("%s blocks\n" % nb); sys.stderr.flush()
        srcs = [blocks[i % 16] for i in range(nb)]
        d_src = torch.zeros(65536 + nb * bsz + 256, dtype=torch.uint8, device=dev)
        d_blk = [torch.from_numpy(b).to(dev) for b in blocks]
        for i in range(nb): d_src[65536 + i * bsz:65536 + (i + 1) * bsz] = d_blk[i % 16]
        del d_blk
        d_stage = torch.zeros(nb * sstride + 64, dtype=torch.uint8, device=dev)
        d_len = torch.zeros(nb, dtype=torch.int32, device=dev)
        c0 = eng.counters()
        ts = []
        for rep in range(RUNS + 1):                                        # (the first call warms up: code objects, workspaces)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            eng.dev_encode_records_ex(d_src.data_ptr() + 65536, nb * bsz, bsz, bsz, False, d_stage.data_ptr(), d_len.data_ptr(), linked=True, d=d,
                                      stream=s.cuda_stream, level=2)
            e1.record(s); torch.cuda.synchronize()
            if rep: ts.append(e0.elapsed_time(e1))
        c1 = eng.counters()
        for i in (0, nb - 1):
            n = int(d_len[i].item())
            check(i, d_stage[i * sstride:i * sstride + n].cpu().numpy())
        out["device_resident_ms"][str(nb)] = _stat(ts)
        if has:
            out["mxl_blocks"][str(nb)] = (c1["mxl_blocks"] - c0["mxl_blocks"]) // (RUNS + 1)
            out["rounds"][str(nb)] = c1["mx_rounds_last"]
            out["pieces_again"][str(nb)] = (c1["mx_pieces_again"] - c0["mx_pieces_again"]) // (RUNS + 1)
        del d_src, d_stage
        ts = []
        for rep in range(RUNS + 1):
            t0 = time.perf_counter()
            recs = eng.encode_records_ex(srcs, bsz, False, linked=True, d=d, level=2)
            if rep: ts.append((time.perf_counter() - t0) * 1e3)
        for i in (0, nb - 1):
            check(i, recs[i])
        out["host_buffers_ms"][str(nb)] = _stat(ts)
        del recs
        eng.trim()
    eng.dict_destroy(d)
    eng.close()
    return out


def child(name, tree, sizes, extra):
    env = dict(os.environ, MXL_RATE_CHILD=tree, MXL_RATE_SIZES=",".join(map(str, sizes)), **extra)
    sys.stderr.write("column %s\n" % name); sys.stderr.flush()
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, stdout=subprocess.PIPE, text=True, timeout=1100)   # (progress on stderr)
    if p.returncode != 0:
        sys.stderr.write("%s: exit %d\n" % (name, p.returncode))
        sys.exit(p.returncode if p.returncode > 0 else 1)
    return dict(json.loads(p.stdout.strip().splitlines()[-1]), tree="parent commit" if name == "parent" else "this tree")


def beats(a, b):
    """per count: a's median below b's by more than the two spreads together"""
    return {k: bool(b[k]["median"] - v["median"] > (v["max"] - v["min"]) + (b[k]["max"] - b[k]["min"])) for k, v in a.items() if k in b}


def compare(res):
    cols = [c for c in ("off", "parent") if c in res]
    if "mxl" not in res or not cols:
        return
    for c in cols:
        for kind in KINDS:
            res["speedup_%s_over_%s" % (kind[:-3], c)] = {k: round(res[c][kind][k]["median"] / v["median"], 2) for k, v in res["mxl"][kind].items() if k in res[c][kind]}
            res["mxl_beats_%s_%s" % (c, kind[:-3])] = beats(res["mxl"][kind], res[c][kind])
    limit = 0
    for k in sorted(res["mxl"][KINDS[0]], key=int):                       # the largest count up to which every comparison holds, without a gap
        if not all(res["mxl_beats_%s_%s" % (c, kind[:-3])].get(k, False) for c in cols for kind in KINDS):
            break
        limit = int(k)
    res["limit_by_the_rule"] = limit


if __name__ == "__main__":
    if os.environ.get("MXL_RATE_CHILD"):
        print(json.dumps(measure(os.environ["MXL_RATE_CHILD"], [int(x) for x in os.environ["MXL_RATE_SIZES"].split(",")])))
        sys.exit(0)
    args = sys.argv[1:]
    parent = only = None
    sizes = list(SIZES)
    if "--parent" in args: i = args.index("--parent"); parent = os.path.abspath(args[i + 1]); del args[i:i + 2]
    if "--sizes" in args: i = args.index("--sizes"); sizes = [int(x) for x in args[i + 1].split(",")]; del args[i:i + 2]
    if "--only" in args: i = args.index("--only"); only = args[i + 1]; del args[i:i + 2]
    res = {"runs_per_point": RUNS}
    if only and args and os.path.exists(args[0]):
        with open(args[0]) as f:
            res = json.load(f)
    if only in (None, "mxl"): res["mxl"] = child("mxl", ROOT, sizes, {"PLZ4HIP_MXL_MAX_BLOCKS": "100000"})
    if only in (None, "off"): res["off"] = child("off", ROOT, sizes, {"PLZ4HIP_MXL_MAX_BLOCKS": "0"})
    if parent and only in (None, "parent"): res["parent"] = child("parent", parent, sizes, {})
    compare(res)
    txt = json.dumps(res, indent=1)
    print(txt)
    if args:
        with open(args[0], "w") as f:
            f.write(txt + "\n")
