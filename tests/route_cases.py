"""The calls of tests/test_gpu_routes.py: the smallest shapes that reach each route of plz4_amd/csrc/route.h.  A case names its
call, the environment switches of the call and the question the test puts to the CPU build of the route function.  Run as a
program -- `python route_cases.py NAME` in a fresh process whose environment holds the switches -- it makes the call, compares the
bytes with the oracle's / the real liblz4's and prints one JSON line: {"parity": bool, "counters": the deltas of
plz4hip_ctx_counters, "shape": what only the call knows of its shape}.  Test infrastructure."""
import json
import os
import sys

import numpy as np

M4 = 1 << 22
KIND = {}                                                                       # call -> function(eng, orc, ref, **args) -> parity
SEEN = {}                                                                       # what the call learns of its shape: the compressed size


def call(f):
    KIND[f.__name__] = f
    return f


def _text(n, seed):
    from plz4_amd import synth
    return synth.text(n, seed=seed)


def _blocks(plain, bsz):
    return [np.ascontiguousarray(plain[o:o + bsz]) for o in range(0, plain.size, bsz)]


@call
def l1_plain(eng, orc, ref):
    srcs = _blocks(_text(2 * 66000, 1), 66000)
    got = eng.encode_records(srcs, 66000, True)
    return all(np.array_equal(g, orc.block_record(s, 66000, True)) for g, s in zip(got, srcs))


@call
def l1_linked_host(eng, orc, ref):
    from test_gpu_dev_encode_ex import _want_linked
    plain = _text(2 * 66000, 2)
    got = eng.encode_records_ex(_blocks(plain, 66000), 66000, True, linked=True)
    return [g.tobytes() for g in got] == _want_linked(orc, plain, 66000, True)


@call
def l1_linked_body(eng, orc, ref):
    from test_gpu_dev_encode_ex import _call, _want_linked
    plain = _text(2 * 66000, 2)
    want = _want_linked(orc, plain, 66000, True)
    recs, rl, off, _, _ = _call(eng, plain, 66000, True, "body", linked=True)
    return recs == want and [int(x) for x in off] == [0] + list(np.cumsum([len(w) for w in want]))


@call
def hc_dict_small(eng, orc, ref, level):
    import hcdict
    import hcx_cases as hc
    blocks = _blocks(_text(12 * 4096, 3), 4096)
    want, _ = hcdict.ref_records(ref, orc, blocks, 4096, level, False, hc.TEXT_DICT, checksum=True)
    d = eng.dict_create(hc.TEXT_DICT)
    got = eng.encode_records_ex(blocks, 4096, True, linked=False, d=d, level=level)
    return [g.tobytes() for g in got] == want


@call
def hc_plain(eng, orc, ref, level, nb):
    import hcdict
    bsz = 128 << 10
    blocks = _blocks(_text(nb * bsz, 4), bsz)
    want, _ = hcdict.ref_records(ref, orc, blocks, bsz, level, False, None, checksum=True)
    got = eng.encode_records(blocks, bsz, True, level=level)
    return [g.tobytes() for g in got] == want


@call
def dx_raw(eng, orc, ref):
    srcs = _blocks(_text(2 * 66000, 5), 66000)
    comp = [orc.compress_fast(s, orc.bound(s.size))[1] for s in srcs]
    assert all(c.size >= 16384 for c in comp)
    SEEN["maxIn"] = max(c.size for c in comp)
    res, outs = eng.decompress_batch([np.ascontiguousarray(c) for c in comp], [66000, 66000])
    return all(int(r) == s.size and np.array_equal(o, s) for r, o, s in zip(res, outs, srcs))


@call
def dx_linked_chain(eng, orc, ref):
    from test_gpu_dev_encode_ex import _want_linked
    plain = _text(6 * 65536, 6)
    recs = [np.frombuffer(r, np.uint8).copy() for r in _want_linked(orc, plain, 65536, True)]
    assert all(r.size >= 16384 for r in recs)
    res, st, outs, _ = eng.decode_records_ex(recs, 65536, True, linked=True, window=np.zeros(65536, np.uint8), window_len=0)
    return not any(st) and np.array_equal(np.concatenate(outs), plain)


@call
def dx_big(eng, orc, ref):
    n = M4 + 4096
    plain = _text(n, 7)
    r, comp = orc.compress_fast(plain, orc.bound(n))
    assert comp.size >= 16384
    SEEN["maxIn"] = comp.size
    res, outs = eng.decompress_batch([np.ascontiguousarray(comp)], [n])
    return int(res[0]) == n and np.array_equal(outs[0], plain)


def L1(nb, maxLen, hist=0, l1x=0, body=0):
    return ("l1", dict(nb=nb, maxLen=maxLen, raw=0, mid=0, rider=0, hist=hist, l1x=l1x, body=body, ctx=0))


def HC(level, nb, maxLen, hcEx=0, dict_=0):
    return ("hc", dict(level=level, nb=nb, maxLen=maxLen, raw=0, hcEx=hcEx, dict=dict_, dictCtx=dict_, linked=0, hcxStart=dict_))


def DX(nb, maxIn, maxOut, records=0, hist=0, chain=0):
    return ("dx", dict(nb=nb, maxIn=maxIn, maxOut=maxOut, records=records, hist=hist, window=chain, nChains=chain, longest=nb * chain, hostFirst=chain))


# name: (call, its arguments, the switches, the question: function and shape)
CASES = {}
for env in ({}, {"PLZ4HIP_FX_MAX_BLOCKS": "0"}, {"PLZ4HIP_L1_FUSED": "1"}):
    CASES["l1_plain" + "".join("-%s=%s" % kv for kv in env.items())] = ("l1_plain", {}, env, L1(2, 66000))
for env in ({}, {"PLZ4HIP_FX_LINKED": "0"}, {"PLZ4HIP_FX_LINKED": "0", "PLZ4HIP_L1X": "0"}, {"PLZ4HIP_L1_FUSED": "1"}):
    tag = "".join("-%s=%s" % kv for kv in env.items())
    CASES["l1_linked_host" + tag] = ("l1_linked_host", {}, env, L1(2, 66000, hist=1))
    CASES["l1_linked_body" + tag] = ("l1_linked_body", {}, env, L1(2, 66000, hist=1, l1x=1, body=1))
for level in (2, 9):
    for env in ({}, {"PLZ4HIP_HCX": "0"}):
        CASES["hc_dict_small-%d%s" % (level, "-HCX=0" if env else "")] = ("hc_dict_small", {"level": level}, env, HC(level, 12, 4096, 1, 1))
for level, env in ((2, {}), (9, {}), (12, {}), (12, {"PLZ4HIP_HC12_SEG_OFF": "1"})):
    CASES["hc_plain-%d%s" % (level, "-SEG_OFF" if env else "")] = ("hc_plain", {"level": level, "nb": 3}, env, HC(level, 3, 128 << 10))
CASES["hc_plain-9-overlap"] = ("hc_plain", {"level": 9, "nb": 6}, {"PLZ4HIP_HC_OVERLAP_MIN": "2"}, HC(9, 6, 128 << 10))
CASES["hc_plain-9-LAZY_OFF"] = ("hc_plain", {"level": 9, "nb": 6}, {"PLZ4HIP_HC_LAZY_OFF": "1"}, HC(9, 6, 128 << 10))
for env in ({}, {"PLZ4HIP_DX_MAX_BLOCKS": "0"}):
    CASES["dx_raw" + ("-MAX=0" if env else "")] = ("dx_raw", {}, env, DX(2, 0, 66000))           # (maxIn: the compressed size, from the call)
CASES["dx_linked_chain"] = ("dx_linked_chain", {}, {"PLZ4HIP_DXL_GROUP_BLOCKS": "2"}, DX(6, 65536, 65536 + 8, records=1, hist=2, chain=1))
for env in ({}, {"PLZ4HIP_DX_BIG": "0"}):
    CASES["dx_big" + ("-BIG=0" if env else "")] = ("dx_big", {}, env, DX(1, 0, M4 + 4096))


def main(name):
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    from orclib import Oracle, Ref
    from plz4_amd._native import Engine
    kind, args, _, _ = CASES[name]
    eng = Engine(0)
    c0 = eng.counters()
    parity = bool(KIND[kind](eng, Oracle(), Ref() if Ref.available() else None, **args))
    c1 = eng.counters()
    eng.close()
    print(json.dumps({"parity": parity, "counters": {k: c1[k] - c0[k] for k in c1}, "shape": SEEN}))


if __name__ == "__main__":
    main(sys.argv[1])
