"""The calls of tests/test_gpu_block_io.py: one list of blocks through every kernel that shares the priming rule and the record writer
of plz4_amd/csrc/lz4_block_io.inl, each on the route that launches it.  Run as a program -- `python block_io_cases.py NAME` in a
fresh process whose environment holds the route's switches -- it makes the case's calls with block checksums on and off, compares
every byte and result with the oracle's / the real liblz4's and prints one JSON line: {"failed": [what differed], "stored": whether
every record of the random block was a stored one, "counters": the deltas of plz4hip_ctx_counters}.  Test infrastructure."""
import json
import os
import sys

import numpy as np

BSZ = 64 << 10
RANDOM = 4                                                                      # the list's block that does not compress


def blocks():
    from plz4_amd import synth
    text = synth.text(4 * BSZ, seed=61)
    rnd = np.random.default_rng(62).integers(0, 256, BSZ, dtype=np.uint8)
    return [np.ascontiguousarray(b) for b in (text[:0], text[100:113], text[1000:1000 + 4096], text[9000:9000 + 4097], rnd, text[2 * BSZ:3 * BSZ])]


def small_blocks():
    """The list's blocks a dictionary context serves by lookup, and one of them that does not compress."""
    return blocks()[:3] + [np.ascontiguousarray(blocks()[RANDOM][:4096])]


def dictionary():
    from plz4_amd import synth
    return np.ascontiguousarray(synth.text(BSZ, seed=63))


class Run:
    def __init__(self, eng, orc, ref):
        self.eng, self.orc, self.ref, self.failed, self.stored = eng, orc, ref, [], []

    def records(self, what, got, want, random_at=RANDOM):
        got, want = [g.tobytes() for g in got], [w if isinstance(w, bytes) else w.tobytes() for w in want]
        if got != want:
            self.failed.append(what + ": blocks " + ",".join(str(i) for i, (g, w) in enumerate(zip(got, want)) if g != w))
        if random_at is not None:
            self.stored.append(bool(got[random_at][3] & 0x80))

    def raw(self, what, res, outs, want):
        bad = [i for i, (r, o, (wr, wo)) in enumerate(zip(res, outs, want)) if int(r) != wr or o.tobytes() != wo[:max(wr, 0)].tobytes()]
        if bad:
            self.failed.append(what + ": blocks " + ",".join(map(str, bad)))

    def l1_record(self, r, c, b, cs):
        payload, word = (b, 0x80000000 | b.size) if r == 0 else (c[:r], r)
        rec = np.uint32(word).tobytes() + payload.tobytes()
        return rec + (np.uint32(self.orc.xxh32(payload)).tobytes() if cs else b"")

    def want_linked(self, bl, cs, dctx=None):
        out, prev = [], None
        for b in bl:
            tail = None if prev is None else prev[-65536:].copy()
            r, c = self.orc.compress_linked(b, BSZ, tail, dctx if tail is None else None)
            out.append(self.l1_record(r, c, b, cs)); prev = b
        return out


def fused(run):
    """k_encode_rec / k_encode_raw"""
    bl = blocks()
    for cs in (False, True):
        run.records("records cs=%d" % cs, run.eng.encode_records(bl, BSZ, cs), [run.orc.block_record(b, BSZ, cs) for b in bl])
    caps = [run.orc.bound(b.size) for b in bl]
    res, outs = run.eng.compress_batch(bl, caps)
    run.raw("raw", res, outs, [run.orc.compress_fast(b, c) for b, c in zip(bl, caps)])


def dict_kernels(run):
    """k_encode_rec_dict (linked, under a dictionary, both) / k_encode_raw_dict"""
    bl, dct = blocks(), dictionary()
    dctx, d = run.orc.dict_ctx(dct), run.eng.dict_create(dct)
    for cs in (False, True):
        run.records("linked cs=%d" % cs, run.eng.encode_records_ex(bl, BSZ, cs, linked=True), run.want_linked(bl, cs))
        run.records("linked+dict cs=%d" % cs, run.eng.encode_records_ex(bl, BSZ, cs, linked=True, d=d), run.want_linked(bl, cs, dctx))
        run.records("dict cs=%d" % cs, run.eng.encode_records_ex(bl, BSZ, cs, linked=False, d=d),
                    [run.l1_record(*run.orc.compress_indie_dict(b, BSZ, dctx), b, cs) for b in bl])
    caps = [run.orc.bound(b.size) for b in bl]
    res, outs = run.eng.compress_batch_dict(bl, caps, d)
    run.raw("raw dict", res, outs, [run.orc.compress_indie_dict(b, c, dctx) for b, c in zip(bl, caps)])


def fxl_small(run):
    """k_fxl_small behind the few-block route: its record and raw branches, and into a frame body.  The route takes calls whose
    largest block has at least 65547 bytes (kFxMinLen), so the list gets one such block and the records that size (the random
    block still does not fit in it)."""
    from plz4_amd import synth
    from test_gpu_dev_encode_ex import _call
    bsz = 65547
    big = np.ascontiguousarray(synth.text(bsz, seed=64))
    bl, dct = blocks() + [big], dictionary()
    dctx, d = run.orc.dict_ctx(dct), run.eng.dict_create(dct)
    plain = np.concatenate([big, bl[2]])                                 # (device-resident plaintext: a full block, then one of 4096 bytes)
    for cs in (False, True):
        run.records("dict cs=%d" % cs, run.eng.encode_records_ex(bl, bsz, cs, linked=False, d=d),
                    [run.l1_record(*run.orc.compress_indie_dict(b, bsz, dctx), b, cs) for b in bl])
        want = [run.l1_record(*run.orc.compress_indie_dict(b, bsz, dctx), b, cs) for b in (big, bl[2])]
        recs, rl, off, _, _ = _call(run.eng, plain, bsz, cs, "body", linked=False, d=d, gap=65536)   # (scratch in front of every block)
        if recs != want or [int(x) for x in off] != [0] + list(np.cumsum([len(w) for w in want])) or [int(x) for x in rl] != [len(w) for w in want]:
            run.failed.append("body cs=%d" % cs)
    caps = [run.orc.bound(b.size) for b in bl]
    res, outs = run.eng.compress_batch_dict(bl, caps, d)
    run.raw("raw dict", res, outs, [run.orc.compress_indie_dict(b, c, dctx) for b, c in zip(bl, caps)])


def one_thread(run, level):
    """k_encode_rec_hc / k_encode_raw_hc: independent blocks, linked blocks, under a dictionary"""
    import hcdict
    bl, dct = blocks(), dictionary()
    d = run.eng.dict_create(dct)
    keep, daddr = run.ref.new_dict_ctx_hc(dct, level)
    for cs in (False, True):
        run.records("records cs=%d" % cs, run.eng.encode_records(bl, BSZ, cs, level=level), hcdict.ref_records(run.ref, run.orc, bl, BSZ, level, False, None, cs)[0])
        for linked in (False, True):
            run.records("dict linked=%d cs=%d" % (linked, cs), run.eng.encode_records_ex(bl, BSZ, cs, linked=linked, d=d, level=level),
                        hcdict.ref_records(run.ref, run.orc, bl, BSZ, level, linked, dct, cs)[0])
    caps = [run.orc.bound(b.size) for b in bl]
    res, outs = run.eng.compress_batch(bl, caps, level=level)
    run.raw("raw", res, outs, [run.ref.compress_hc(b, c, level) for b, c in zip(bl, caps)])
    comp = run.ref.stream_ctx_hc(level, daddr)
    res, outs = run.eng.compress_batch_dict(bl, caps, d, level=level)
    run.raw("raw dict", res, outs, [comp(b, c) for b, c in zip(bl, caps)])


def hcx_only(run, level):
    """k_hcx<kRaw, level 2>: a call of nothing but blocks of at most 4 KiB under a dictionary"""
    import hcdict
    bl, dct = small_blocks(), dictionary()
    d = run.eng.dict_create(dct)
    keep, daddr = run.ref.new_dict_ctx_hc(dct, level)
    for cs in (False, True):
        run.records("records cs=%d" % cs, run.eng.encode_records_ex(bl, 4096, cs, linked=False, d=d, level=level),
                    hcdict.ref_records(run.ref, run.orc, bl, 4096, level, False, dct, cs)[0], random_at=3)
    caps = [run.orc.bound(b.size) for b in bl]
    comp = run.ref.stream_ctx_hc(level, daddr)
    res, outs = run.eng.compress_batch_dict(bl, caps, d, level=level)
    run.raw("raw dict", res, outs, [comp(b, c) for b, c in zip(bl, caps)])


def hc12_parse(run):
    """k_hc12_parse, records and raw blocks"""
    import hcdict
    bl = blocks()
    for cs in (False, True):
        run.records("records cs=%d" % cs, run.eng.encode_records(bl, BSZ, cs, level=12), hcdict.ref_records(run.ref, run.orc, bl, BSZ, 12, False, None, cs)[0])
    caps = [run.orc.bound(b.size) for b in bl]
    res, outs = run.eng.compress_batch(bl, caps, level=12)
    run.raw("raw", res, outs, [run.ref.compress_hc(b, c, 12) for b, c in zip(bl, caps)])


# name: (call, its arguments, the switches, the counters that move -- every other counted one stays)
CASES = {
    "fused": (fused, {}, {"PLZ4HIP_L1_FUSED": "1"}, ()),
    "dict_kernels": (dict_kernels, {}, {"PLZ4HIP_L1_FUSED": "1"}, ()),
    "fxl_small": (fxl_small, {}, {}, ("fx_blocks", "fxl_blocks")),
    "one_thread-9": (one_thread, {"level": 9}, {"PLZ4HIP_HC_LAZY_OFF": "1", "PLZ4HIP_HC_EXT_OFF": "1", "PLZ4HIP_HCX": "0"}, ()),
    "hcx_only-2": (hcx_only, {"level": 2}, {}, ("hcx_blocks",)),
    "hcx_only-9": (hcx_only, {"level": 9}, {}, ("hcx_blocks",)),
    "hc12_parse": (hc12_parse, {}, {"PLZ4HIP_HC12_SEG_OFF": "1"}, ()),
}


def main(name):
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    from orclib import Oracle, Ref
    from plz4_amd._native import Engine
    f, args, _, _ = CASES[name]
    eng = Engine(0)
    run = Run(eng, Oracle(), Ref() if Ref.available() else None)
    c0 = eng.counters()
    f(run, **args)
    c1 = eng.counters()
    eng.close()
    print(json.dumps({"failed": run.failed, "stored": bool(run.stored) and all(run.stored), "counters": {k: c1[k] - c0[k] for k in c1}}))


if __name__ == "__main__":
    main(sys.argv[1])
