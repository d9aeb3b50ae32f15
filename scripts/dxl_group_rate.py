"""A long linked chain in one decode call (launch_decode's groups of blocks): 4 MiB blocks of synthetic text as one
linked frame with a 64 KiB dictionary, block checksums on, through decode_records_ex over host buffers (staging copies and PCIe
included, warm), as scripts/dxl_rate.py measures the few-block path.
    python scripts/dxl_group_rate.py [NAME=]TREE [[NAME=]TREE ...] [--passes N] [--groups 16,32,64,128] [--cliff NAME]
runs the trees in alternating child processes (each loads plz4_amd from its tree) and prints one JSON line per run:
  chain_ms[nb]          ms of a chain of nb blocks in one call (32 and 256; a tree without groups runs 32 only)
  group_ms / group_dev_ms   the 256-block chain at PLZ4HIP_DXL_GROUP_BLOCKS=G through host buffers / the kernels alone (a child per G)
  dev_ms[nb]            the kernels alone, plz4hip_dev_decode_records_ex on a device-resident body (16 and 256 blocks)
  cliff_130_ms          --cliff NAME: that tree's 130-block chain without groups, ONE run under its own time limit (t_wave)"""
import json, os, subprocess, sys, time


def _measure(call, check, budget=1.0):
    check(call())                                                            # warm, and the result is right
    t0 = time.perf_counter(); call(); t1 = time.perf_counter() - t0
    reps = max(1, min(50, int(round(budget / max(t1, 1e-4)))))
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); call(); ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return {"ms": round(ts[len(ts) // 2], 3), "min": round(ts[0], 3), "max": round(ts[-1], 3), "reps": reps}


def child(arg, what):
    name, _, tree = arg.rpartition("=")
    sys.path.insert(0, tree)
    import numpy as np
    from plz4_amd import synth
    from plz4_amd._native import Engine
    bsz = 4 << 20
    eng = Engine(0)
    grouped = hasattr(eng, "dev_decode_records_ex")
    nmax = 130 if what == "cliff" else (256 if grouped else 32)
    pool = synth.text(32 * bsz)
    blocks = [np.ascontiguousarray(pool[(i % 32) * bsz:(i % 32 + 1) * bsz]) for i in range(nmax)]
    dct = np.ascontiguousarray(synth.text(65536, seed=77))
    d = eng.dict_create(dct)
    out = {"tree": name or tree, "what": what, "group_blocks": os.environ.get("PLZ4HIP_DXL_GROUP_BLOCKS", "default")}
    linked = [np.ascontiguousarray(r) for r in eng.encode_records_ex(blocks, bsz, True, linked=True, d=d)]

    def host_call(nb):
        w = dct.copy()
        return eng.decode_records_ex(linked[:nb], bsz, True, linked=True, window=w, window_len=65536)

    def same(nb):
        def check(r):
            assert not any(int(s) for s in r[1]) and all(np.array_equal(o, s) for o, s in zip(r[2], blocks[:nb]))
        return check

    def dev_measure(nbs):
        import torch
        dev = torch.device("cuda:0")
        res = {}
        for nb in nbs:
            off = np.zeros(nb + 1, np.int64); off[1:] = np.cumsum([r.size for r in linked[:nb]])
            d_body = torch.from_numpy(np.concatenate(linked[:nb] + [np.zeros(64, np.uint8)])).to(dev)
            d_off = torch.from_numpy(off).to(dev)
            stride = bsz + 64
            d_out = torch.zeros(nb * stride + 64, dtype=torch.uint8, device=dev)
            d_res = torch.zeros(nb, dtype=torch.int32, device=dev); d_st = torch.zeros(nb, dtype=torch.int32, device=dev)
            w = np.zeros((1, 131072), np.uint8); w[0, :65536] = dct
            d_w0 = torch.from_numpy(w).to(dev); d_w = d_w0.clone(); d_wl = torch.zeros(1, dtype=torch.int32, device=dev)
            s = torch.cuda.current_stream().cuda_stream

            def call():
                d_w.copy_(d_w0); d_wl.fill_(65536)
                eng.dev_decode_records_ex(d_body.data_ptr(), d_off.data_ptr(), nb, bsz, True, d_out.data_ptr(), stride, bsz + 8,
                                          d_res.data_ptr(), d_st.data_ptr(), linked=True, windows_ptr=d_w.data_ptr(),
                                          window_len_ptr=d_wl.data_ptr(), stream=s)
                torch.cuda.synchronize()
                return d_st, d_out

            def check(r):
                assert int(r[0].abs().sum().item()) == 0
                o = r[1].cpu().numpy()
                assert all(np.array_equal(o[i * stride:i * stride + bsz], blocks[i]) for i in range(nb))
            res[str(nb)] = _measure(call, check, budget=2.0)
            del d_body, d_out
        return res

    if what == "cliff":
        t0 = time.perf_counter(); r = host_call(130); out["cliff_130_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        same(130)(r)
    elif what == "group":
        out["group_ms"] = _measure(lambda: host_call(256), same(256), budget=2.0)
        out["group_dev_ms"] = dev_measure((256,))["256"]
    else:
        out["chain_ms"] = {}
        for nb in (32, 256) if grouped else (32,):
            out["chain_ms"][str(nb)] = _measure(lambda nb=nb: host_call(nb), same(nb), budget=2.0)
        if grouped:
            out["dev_ms"] = dev_measure((16, 256))
    if hasattr(eng, "counters"):
        out["counters"] = eng.counters()
    print(json.dumps(out))
    eng.dict_destroy(d)
    eng.close()


def _run(tree, what, env=None, timeout=420):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree, what], capture_output=True, text=True, timeout=timeout,
                       env=dict(os.environ, **(env or {})))
    if r.returncode != 0:                                                    # nothing more is started behind a failed run
        sys.exit("run of %s (%s) failed (%d): %s" % (tree, what, r.returncode, r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        return child(args[1], args[2])
    passes, groups, cliff = 2, [], None
    for flag in ("--passes", "--groups", "--cliff"):
        if flag in args:
            i = args.index(flag); v = args[i + 1]; del args[i:i + 2]
            if flag == "--passes": passes = int(v)
            elif flag == "--groups": groups = [int(x) for x in v.split(",")]
            else: cliff = v
    if not args:
        sys.exit(__doc__)
    for p in range(passes):
        for tree in args:
            line = _run(tree, "chain"); line["pass"] = p
            print(json.dumps(line), flush=True)
    for g in groups:                                                         # the last tree named is the one with groups
        line = _run(args[-1], "group", {"PLZ4HIP_DXL_GROUP_BLOCKS": str(g)})
        print(json.dumps(line), flush=True)
    if cliff:
        tree = next(t for t in args if t.rpartition("=")[0] == cliff or t == cliff)
        print(json.dumps(_run(tree, "cliff", {"PLZ4HIP_DXL_GROUP_BLOCKS": "0"}, timeout=120)), flush=True)


if __name__ == "__main__":
    main()
