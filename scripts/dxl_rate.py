"""Few blocks with history outside the block -- linked chains, independent blocks under a dictionary -- through host buffers (staging
copies and PCIe included, warm): 4 MiB blocks of synthetic text, block checksums on, a 64 KiB dictionary.  Beside them
decode_records of the same number of INDEPENDENT records, the yardstick for "the chain is cut".  Only entry points every tree has
(counters where they exist).
    python scripts/dxl_rate.py [NAME=]TREE [[NAME=]TREE ...] [--passes N]
runs the trees in alternating child processes (each loads plz4_amd from its tree) and prints one JSON line per run."""
import json, os, subprocess, sys, time


def _measure(call, check):
    """Median, smallest and largest of enough repetitions that the timed window is about a second (at least one), in ms."""
    check(call())                                                            # warm, and the result is right
    t0 = time.perf_counter(); call(); t1 = time.perf_counter() - t0
    reps = max(1, min(200, int(round(1.0 / max(t1, 1e-4)))))
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); call(); ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return {"ms": round(ts[len(ts) // 2], 3), "min": round(ts[0], 3), "max": round(ts[-1], 3), "reps": reps}


def child(arg):
    name, _, tree = arg.rpartition("=")
    sys.path.insert(0, tree)
    import numpy as np
    from plz4_amd import synth
    from plz4_amd._native import Engine
    bsz = 4 << 20
    eng = Engine(0)
    pool = synth.text(32 * bsz)
    blocks = [np.ascontiguousarray(pool[i * bsz:(i + 1) * bsz]) for i in range(32)]
    dct = np.ascontiguousarray(synth.text(65536, seed=77))
    d = eng.dict_create(dct)
    out = {"tree": name or tree, "dx_linked": os.environ.get("PLZ4HIP_DX_LINKED", "default")}

    def same(srcs):
        def check(r):
            outs = r[2] if len(r) >= 3 and isinstance(r[2], list) else r[1]
            assert all(np.array_equal(o, s) for o, s in zip(outs, srcs))
        return check

    linked = [np.ascontiguousarray(r) for r in eng.encode_records_ex(blocks, bsz, True, linked=True, d=d)]
    out["linked_ms"] = {}
    for nb in (1, 4, 16, 32):
        def call(nb=nb):
            w = dct.copy()
            return eng.decode_records_ex(linked[:nb], bsz, True, linked=True, window=w, window_len=65536)
        out["linked_ms"][str(nb)] = _measure(call, same(blocks[:nb]))
    if hasattr(eng, "counters") and "dxl_rounds_last" in eng.counters():
        out["linked_32_rounds"] = eng.counters()["dxl_rounds_last"]

    chains = [[np.ascontiguousarray(r) for r in eng.encode_records_ex(blocks[4 * k:4 * k + 4], bsz, True, linked=True, d=d)] for k in range(8)]

    def call_chains():
        wall = np.stack([dct] * 8).copy()
        got, _ = eng.decode_records_chains(chains, bsz, True, windows=wall, window_lens=np.full(8, 65536, dtype=np.int32))
        return got

    def check_chains(got):
        for k, (res, st, outs) in enumerate(got):
            assert not any(int(s) for s in st) and all(np.array_equal(o, s) for o, s in zip(outs, blocks[4 * k:4 * k + 4]))
    out["chains_8x4_ms"] = _measure(call_chains, check_chains)

    drecs = [np.ascontiguousarray(r) for r in eng.encode_records_ex(blocks[:16], bsz, True, linked=False, d=d)]
    out["dict_records_16_ms"] = _measure(lambda: eng.decode_records_ex(drecs, bsz, True, linked=False, d=d), same(blocks[:16]))
    bound = bsz + bsz // 255 + 16
    res, comps = eng.compress_batch_dict(blocks[:16], [bound] * 16, d)
    comps = [np.ascontiguousarray(c[:int(r)]) for c, r in zip(comps, res)]
    out["dict_batch_ms"] = {}
    for nb in (1, 16):
        out["dict_batch_ms"][str(nb)] = _measure(lambda nb=nb: eng.decompress_batch_dict(comps[:nb], [bsz + 8] * nb, d),
                                                 lambda r, nb=nb: same(blocks[:nb])((r[0], [o[:bsz] for o in r[1]])))
    indep = [np.ascontiguousarray(r) for r in eng.encode_records(blocks, bsz, True)]
    out["indep_ms"] = {}
    for nb in (1, 4, 16, 32):
        out["indep_ms"][str(nb)] = _measure(lambda nb=nb: eng.decode_records(indep[:nb], bsz, True), same(blocks[:nb]))
    if hasattr(eng, "counters"):
        out["counters"] = eng.counters()
    print(json.dumps(out))
    eng.dict_destroy(d)
    eng.close()


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        return child(args[1])
    passes = 2
    if "--passes" in args:
        i = args.index("--passes"); passes = int(args[i + 1]); del args[i:i + 2]
    if not args:
        sys.exit(__doc__)
    for p in range(passes):
        for tree in args:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree], capture_output=True, text=True, timeout=420)
            if r.returncode != 0:                                            # nothing more is started behind a failed run
                sys.exit("run of %s failed (%d): %s" % (tree, r.returncode, r.stderr[-2000:]))
            line = json.loads(r.stdout.strip().splitlines()[-1]); line["pass"] = p
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
