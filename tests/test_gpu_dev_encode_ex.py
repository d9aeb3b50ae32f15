"""Linked and dictionary frames from device-resident plaintext through the C ABI (plz4hip_dev_encode_records_ex /
plz4hip_dev_encode_body_ex): every record must be the oracle's stream emulation (compress_linked / compress_indie_dict) in
blk.CompressToBlk's framing, byte for byte, on the bulk route (k_l1x_parse + the kSeg emit stage; PLZ4HIP_FX_LINKED=0 keeps a call
of few blocks there), on the few-block route (fxl_blocks of plz4hip_ctx_counters moves) and on the one-kernel encoder
(PLZ4HIP_L1X=0); the HC levels against the real liblz4's linked stream.  A linked call over contiguous plaintext leaves the
plaintext as it was.  The environment switches are read per call."""
import numpy as np
import pytest

import hcdict
from plz4_amd import synth
from test_gpu_fxl_encode import _record

pytestmark = pytest.mark.gpu
PAD = 65536                                                             # the caller's scratch in front of block 0
POISON = 0xA7


@pytest.fixture(scope="module")
def eng():
    from plz4_amd._native import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def text():
    return {k: synth.make(k, (5 * 256 << 10) + 70000, 1 << 16, seed=11 + i) for i, k in enumerate("TM")}


def _call(eng, plain, bsz, cs, form, linked=True, d=None, prev_tail=None, in_place=None, tail_at=None, gap=0, level=1, body_cap=None,
          stream=None):
    """One call on a fresh device buffer: PAD bytes of scratch, then block i at PAD + i * (bsz + gap).  prev_tail: host bytes put in
    a device buffer of their own; in_place: block 0 is block `in_place` of `plain` and prevTail the 64 KiB in front of it; tail_at =
    (back, n): prev_tail's n bytes are put `back` bytes in front of src, inside the scratch, and prevTail points there.
    Returns (records as bytes, recLen, recOff or None, the buffer afterwards, the buffer as it was)."""
    import torch
    dev = torch.device("cuda:0")
    total = plain.size
    nb = -(-total // bsz)
    stride = bsz + gap
    host = np.full(PAD + max(nb, 1) * stride + 256, POISON, np.uint8)
    for i in range(nb):
        b = plain[i * bsz:(i + 1) * bsz]
        host[PAD + i * stride:PAD + i * stride + b.size] = b
    d_src = torch.from_numpy(host).to(dev)
    base = d_src.data_ptr() + PAD
    nbytes, tail_ptr, tail_len, keep = total, None, -1, None
    if in_place is not None:
        assert gap == 0
        base += in_place * bsz; nbytes -= in_place * bsz; nb -= in_place
        tail_ptr, tail_len = base - 65536, 65536
    elif tail_at is not None:
        back, tn = tail_at
        d_src[PAD - back:PAD - back + tn] = torch.from_numpy(prev_tail[:tn]).to(dev)
        host[PAD - back:PAD - back + tn] = prev_tail[:tn]
        tail_ptr, tail_len = base - back, tn
    elif prev_tail is not None:
        keep = torch.from_numpy(np.concatenate([prev_tail, np.zeros(16, np.uint8)])).to(dev)
        tail_ptr, tail_len = keep.data_ptr(), prev_tail.size
    d_len = torch.full((max(nb, 1),), -7, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream.cuda_stream
    if form == "records":
        sstride = eng.stage_stride(bsz)
        d_stage = torch.zeros(max(nb, 1) * sstride + 64, dtype=torch.uint8, device=dev)
        eng.dev_encode_records_ex(base, nbytes, stride, bsz, cs, d_stage.data_ptr(), d_len.data_ptr(), linked=linked, d=d,
                                  prev_tail_ptr=tail_ptr, prev_tail_len=tail_len, stream=s, level=level)
        torch.cuda.synchronize()
        rl, st = d_len.cpu().numpy()[:nb], d_stage.cpu().numpy()
        recs = [st[i * sstride:i * sstride + int(rl[i])].tobytes() for i in range(nb)]
        off = None
    else:
        cap = nb * (bsz + 8) + 64 if body_cap is None else body_cap
        d_body = torch.full((cap + 64,), 0x5C, dtype=torch.uint8, device=dev)
        d_off = torch.full((nb + 1,), -7, dtype=torch.int64, device=dev)
        eng.dev_encode_body_ex(base, nbytes, stride, bsz, cs, d_body.data_ptr(), cap, d_off.data_ptr(), d_len.data_ptr(), linked=linked,
                               d=d, prev_tail_ptr=tail_ptr, prev_tail_len=tail_len, stream=s, level=level)
        torch.cuda.synchronize()
        rl, off, body = d_len.cpu().numpy()[:nb], d_off.cpu().numpy(), d_body.cpu().numpy()
        assert np.all(body[cap:] == 0x5C)                               # (nothing beyond the body's room)
        recs = [body[int(off[i]):int(off[i]) + int(rl[i])].tobytes() if int(off[i]) + int(rl[i]) <= cap else None for i in range(nb)]
    return recs, rl, off, d_src.cpu().numpy(), host


def _untouched(after, before):
    """Outside the 64 KiB in front of block 0 the call has written no byte of src."""
    assert np.array_equal(after[PAD:], before[PAD:])


def _want_linked(orc, plain, bsz, cs, dctx=None, prev_tail=None):
    out, prev = [], None
    for o in range(0, plain.size, bsz):
        b = plain[o:o + bsz].copy()
        tail = prev_tail if o == 0 else prev[-65536:]
        r, c = orc.compress_linked(b, bsz, None if tail is None else tail.copy(), dctx if tail is None else None)
        out.append(_record(orc, r, c, b, cs)); prev = b
    return out


def _check_forms(eng, plain, bsz, cs, want, **kw):
    """Both forms of one call against `want`: records; body = their concatenation, recOff = their prefix sums, recLen their lengths."""
    recs, rl, _, after, before = _call(eng, plain, bsz, cs, "records", **kw)
    assert recs == want, ("records", bsz, cs, plain.size, kw.keys())
    assert [int(x) for x in rl] == [len(w) for w in want]
    if kw.get("gap", 0) == 0:
        _untouched(after, before)
    recs, rl, off, after, before = _call(eng, plain, bsz, cs, "body", **kw)
    assert recs == want, ("body", bsz, cs, plain.size, kw.keys())
    assert [int(x) for x in rl] == [len(w) for w in want]
    assert [int(x) for x in off] == [0] + list(np.cumsum([len(w) for w in want]))
    if kw.get("gap", 0) == 0:
        _untouched(after, before)


STARTS = ["fresh", "dict70000", "dict30000", "dict5", "tail0", "tail7", "tail8", "tail65536"]


def _start(orc, eng, start):
    """(dctx, dict handle, prev_tail) of block 0."""
    user = synth.text(70000, seed=42)
    if start.startswith("dict"):
        dct = np.ascontiguousarray(user[:int(start[4:])])
        return orc.dict_ctx(dct), eng.dict_create(dct), None
    if start.startswith("tail"):
        n = int(start[4:])
        return None, None, np.ascontiguousarray(synth.make("M", 70000, 1 << 16, seed=5)[70000 - n:]).copy()
    return None, None, None


def _fxl(eng, c0):
    return eng.counters()["fxl_blocks"] - c0["fxl_blocks"]


def _l1x(eng, c0):
    """blocks the bulk staged route parsed (k_l1x_parse), which the one-kernel encoder's bytes cannot be told from"""
    return eng.counters()["l1x_blocks"] - c0["l1x_blocks"]


# ---- 1. linked, contiguous, records and body form; 3. the source untouched --------------------------------------------------------
@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("bsz", [64 << 10, 256 << 10])
def test_gpu_dev_linked_contiguous_bulk(orc, eng, text, monkeypatch, bsz, start):
    """The shapes of tests/test_l1x_encode.py on the bulk route: fxl_blocks does not move."""
    monkeypatch.setenv("PLZ4HIP_FX_LINKED", "0")
    dctx, d, prev_tail = _start(orc, eng, start)
    c0 = eng.counters()
    it = parsed = 0
    for nb in (1, 2, 5):
        for last in (1, 12, 13, 4097, bsz):
            total = (nb - 1) * bsz + last
            plain = np.ascontiguousarray(text["TM"[it % 2]][70000:70000 + total]); it += 1
            for cs in (False, True):
                _check_forms(eng, plain, bsz, cs, _want_linked(orc, plain, bsz, cs, dctx, prev_tail), d=d, prev_tail=prev_tail)
            # (a block 0 of <= 4 KiB under a dictionary context of >= 8 bytes is not the parser's; two forms, checksums on and off)
            parsed += 4 * (nb - (start in ("dict70000", "dict30000") and min(total, bsz) <= 4096))
    assert _fxl(eng, c0) == 0 and _l1x(eng, c0) == parsed
    if d is not None:
        eng.dict_destroy(d)


@pytest.mark.parametrize("start", ["fresh", "dict70000", "tail65536"])
def test_gpu_dev_linked_contiguous_few_blocks(orc, eng, start):
    """1, 2 and 3 blocks at bsz 1 MiB, the last one of 100 000 / 262 161 / 131 072 bytes: the few-block route, fxl_blocks moves by the
    block count."""
    bsz = 1 << 20
    dctx, d, prev_tail = _start(orc, eng, start)
    data = synth.make("M", 2 * bsz + 131072, 1 << 16, seed=3)
    for total in (100000, bsz + 262161, 2 * bsz + 131072):
        plain = np.ascontiguousarray(data[:total])
        nb = -(-total // bsz)
        for cs in (False, True):
            c0 = eng.counters()
            _check_forms(eng, plain, bsz, cs, _want_linked(orc, plain, bsz, cs, dctx, prev_tail), d=d, prev_tail=prev_tail)
            assert _fxl(eng, c0) == 2 * nb and _l1x(eng, c0) == 0, (total, cs)      # (one call per form)
    if d is not None:
        eng.dict_destroy(d)


@pytest.mark.parametrize("bsz", [64 << 10, 256 << 10])
def test_gpu_dev_l1x_switch_gives_the_same_bytes(orc, eng, text, monkeypatch, bsz):
    """PLZ4HIP_L1X=0: the one-kernel encoder, records and body (through the ctx's staging area), the same bytes."""
    monkeypatch.setenv("PLZ4HIP_FX_LINKED", "0")
    monkeypatch.setenv("PLZ4HIP_L1X", "0")
    user = np.ascontiguousarray(synth.text(70000, seed=42))
    dctx, d = orc.dict_ctx(user), eng.dict_create(user)
    plain = np.ascontiguousarray(text["T"][70000:70000 + 4 * bsz + 4097])
    c0 = eng.counters()
    for cs in (False, True):
        _check_forms(eng, plain, bsz, cs, _want_linked(orc, plain, bsz, cs, dctx), d=d)
    assert _l1x(eng, c0) == 0 and _fxl(eng, c0) == 0
    monkeypatch.setenv("PLZ4HIP_L1X", "1")
    _check_forms(eng, plain, bsz, True, _want_linked(orc, plain, bsz, True, dctx), d=d)
    assert _l1x(eng, c0) == 2 * 5
    eng.dict_destroy(d)


# ---- 2. continuing a frame ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["bulk", "few"])
def test_gpu_dev_linked_continues_a_frame(orc, eng, text, monkeypatch, route):
    """Blocks [0, k) then [k, n) of one buffer, prevTail the 64 KiB in front of block k where they lie (nothing is copied, nothing
    written) and once more from a buffer of its own: the bytes of the one call."""
    if route == "bulk":
        monkeypatch.setenv("PLZ4HIP_FX_LINKED", "0")
    bsz, n, k = 256 << 10, 5, 2
    plain = np.ascontiguousarray(text["M"][70000:70000 + (n - 1) * bsz + 4097])
    want = _want_linked(orc, plain, bsz, True)
    for form in ("records", "body"):
        first, _, _, after, before = _call(eng, np.ascontiguousarray(plain[:k * bsz]), bsz, True, form)
        _untouched(after, before)
        recs, _, off, after, before = _call(eng, plain, bsz, True, form, in_place=k)
        assert np.array_equal(after, before)                              # (not even the scratch in front of block 0 of the buffer)
        assert first + recs == want, (route, form)
        if off is not None:
            assert [int(x) for x in off] == [0] + list(np.cumsum([len(w) for w in want[k:]]))
        tail = np.ascontiguousarray(plain[k * bsz - 65536:k * bsz]).copy()
        recs, _, _, after, before = _call(eng, np.ascontiguousarray(plain[k * bsz:]), bsz, True, form, prev_tail=tail)
        _untouched(after, before)
        assert first + recs == want, (route, form, "own buffer")


# ---- 4. dictionary, independent blocks, gapped stride; linked blocks on the gapped stride ------------------------------------------------
@pytest.mark.parametrize("route", ["bulk", "few"])
@pytest.mark.parametrize("dlen", [70000, 30000, 5])
def test_gpu_dev_dictionary_independent_gapped(orc, eng, monkeypatch, route, dlen):
    """Every block against the dictionary: blocks of 5, 4096, 4097, 65 547 and 200 000 bytes (two whole ones and a shorter one per
    call) and the empty call, 64 KiB + 48 of scratch in front of every block; the blocks <= 4 KiB under the context keep their
    two-table encoder, in the body form too."""
    if route == "bulk":
        monkeypatch.setenv("PLZ4HIP_FX_LINKED", "0")
    user = np.ascontiguousarray(synth.text(70000, seed=99)[:dlen])
    data = synth.text(500000 + 4096, seed=7)
    dctx, d = orc.dict_ctx(user), eng.dict_create(user)
    for n in (5, 4096, 4097, 65547, 200000):
        for last in sorted({n, n // 2 + 1, min(n, 4096)}):
            plain = np.ascontiguousarray(data[:2 * n + last])
            for cs in (False, True):
                want = []
                for o in range(0, plain.size, n):
                    b = plain[o:o + n].copy()
                    r, c = orc.compress_indie_dict(b, n, dctx)
                    want.append(_record(orc, r, c, b, cs))
                _check_forms(eng, plain, n, cs, want, linked=False, d=d, gap=65536 + 48)
    recs, rl, off, _, _ = _call(eng, data[:0], 4096, True, "body", linked=False, d=d, gap=65536)
    assert recs == [] and int(off[0]) == 0
    eng.dict_destroy(d)


def test_gpu_dev_linked_gapped(orc, eng, text, monkeypatch):
    """Linked blocks on the gapped stride: the engine copies every block's tail from its predecessor into the gap."""
    bsz = 64 << 10
    user = np.ascontiguousarray(synth.text(70000, seed=42))
    dctx, d = orc.dict_ctx(user), eng.dict_create(user)
    plain = np.ascontiguousarray(text["M"][70000:70000 + 4 * bsz + 13])
    for route in ("bulk", "fused"):
        if route == "fused":
            monkeypatch.setenv("PLZ4HIP_L1X", "0")
        _check_forms(eng, plain, bsz, True, _want_linked(orc, plain, bsz, True, dctx), d=d, gap=65536)
    eng.dict_destroy(d)


# ---- 5. full size -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["bulk", "few"])
@pytest.mark.parametrize("kind", ["T", "M"])
def test_gpu_dev_linked_full_size_blocks(orc, eng, monkeypatch, kind, route):
    """3 x 4 MiB linked blocks behind a 64 KiB dictionary: indices above 2^22, on both routes."""
    if route == "bulk":
        monkeypatch.setenv("PLZ4HIP_FX_LINKED", "0")
    bsz = 4 << 20
    user = np.ascontiguousarray(synth.text(65536, seed=77))
    plain = synth.make(kind, 3 * bsz, bsz, seed=21)
    dctx, d = orc.dict_ctx(user), eng.dict_create(user)
    c0 = eng.counters()
    _check_forms(eng, plain, bsz, True, _want_linked(orc, plain, bsz, True, dctx), d=d)
    assert (_fxl(eng, c0), _l1x(eng, c0)) == ((6, 0) if route == "few" else (0, 6))
    eng.dict_destroy(d)


# ---- 6. bodyCap too small ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["bulk", "few", "fused"])
def test_gpu_dev_body_cap_too_small(orc, eng, text, monkeypatch, route):
    if route != "few":
        monkeypatch.setenv("PLZ4HIP_FX_LINKED", "0")
    if route == "fused":
        monkeypatch.setenv("PLZ4HIP_L1X", "0")
    bsz = 256 << 10
    plain = np.ascontiguousarray(text["T"][70000:70000 + 4 * bsz + 4097])
    want = _want_linked(orc, plain, bsz, True)
    sizes = [len(w) for w in want]
    cap = sum(sizes[:3]) + sizes[3] // 2                                  # (three records fit, the fourth does not, the fifth would)
    recs, rl, off, after, before = _call(eng, plain, bsz, True, "body", body_cap=cap)
    assert int(off[-1]) == sum(sizes) > cap
    assert [int(x) for x in rl] == sizes and [int(x) for x in off] == [0] + list(np.cumsum(sizes))
    assert recs[:3] == want[:3] and recs[3] is None and recs[4] is None
    _untouched(after, before)


# ---- 7. HC levels -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [3, 9])
def test_gpu_dev_linked_hc_levels(orc, ref, eng, text, level):
    """Linked, 3 blocks of 64 KiB, contiguous: the real liblz4's linked HC stream, with and without a dictionary."""
    bsz = 64 << 10
    plain = np.ascontiguousarray(text["M"][70000:70000 + 3 * bsz])
    blocks = [plain[o:o + bsz].copy() for o in range(0, plain.size, bsz)]
    user = np.ascontiguousarray(synth.text(70000, seed=42))
    for dct in (None, user):
        d = eng.dict_create(dct) if dct is not None else None
        want, _ = hcdict.ref_records(ref, orc, blocks, bsz, level, True, dct, checksum=True)
        recs, rl, _, after, before = _call(eng, plain, bsz, True, "records", d=d, level=level)
        assert recs == want, (level, dct is not None)
        _untouched(after, before)
        if d is not None:
            eng.dict_destroy(d)


@pytest.mark.parametrize("dlen", [None, 5, 70000])
def test_gpu_dev_level2_both_forms(orc, ref, eng, text, dlen):
    """Level 2 (lz4mid behind the segment, the staged call) in records and body form against the real liblz4's streams: linked
    contiguous blocks, and independent blocks under the dictionary on the gapped stride.  A block <= 4 KiB that starts under an
    attached dictionary -- of any length: 5 bytes too -- is the one-thread parser's, which writes staged records: the body form
    refuses such a call (PLZ4HIP_E_UNSUPPORTED) and the records form gives the bytes."""
    from plz4_amd._native import EngineError
    dct = None if dlen is None else np.ascontiguousarray(synth.text(70000, seed=42)[:dlen])
    d = eng.dict_create(dct) if dct is not None else None

    def check(plain, bsz, linked, gap, body_ok):
        blocks = [plain[o:o + bsz].copy() for o in range(0, plain.size, bsz)]
        want, _ = hcdict.ref_records(ref, orc, blocks, bsz, 2, linked, dct, checksum=True)
        recs, rl, _, after, before = _call(eng, plain, bsz, True, "records", linked=linked, d=d, gap=gap, level=2)
        assert recs == want, (dlen, plain.size, bsz, linked)
        if not body_ok:
            with pytest.raises(EngineError) as ei:
                _call(eng, plain, bsz, True, "body", linked=linked, d=d, gap=gap, level=2)
            assert ei.value.code == -4
            return
        recs, rl, off, after, before = _call(eng, plain, bsz, True, "body", linked=linked, d=d, gap=gap, level=2)
        assert recs == want, ("body", dlen, plain.size, bsz, linked)
        assert [int(x) for x in rl] == [len(w) for w in want] and [int(x) for x in off] == [0] + list(np.cumsum([len(w) for w in want]))
        if gap == 0:
            _untouched(after, before)

    bsz = 64 << 10
    for total in (3 * bsz + 4097, 2 * bsz + 100, bsz):
        check(np.ascontiguousarray(text["M"][70000:70000 + total]), bsz, True, 0, True)
    check(np.ascontiguousarray(text["M"][70000:70000 + 4096]), bsz, True, 0, dct is None)      # (block 0 of 4 KiB: under the context)
    if dct is not None:
        for total, ok in ((2 * 8192 + 5000, True), (2 * 8192 + 100, False), (2 * 8192 + 4096, False)):
            check(np.ascontiguousarray(text["T"][70000:70000 + total]), 8192, False, 65536, ok)
        check(np.ascontiguousarray(text["T"][70000:70000 + 3 * 4096]), 4096, False, 65536, False)
        eng.dict_destroy(d)


def test_gpu_dev_prev_tail_inside_the_scratch(orc, eng, text, monkeypatch):
    """prevTail may lie in the 64 KiB in front of src when it does not overlap the bytes it is laid at, [src - prevTailLen, src)
    (the bytes of the call with the tail in a buffer of its own); one that overlaps them without ending at src is PLZ4HIP_E_ARG."""
    from plz4_amd._native import EngineError
    monkeypatch.setenv("PLZ4HIP_FX_LINKED", "0")
    bsz = 64 << 10
    plain = np.ascontiguousarray(text["T"][70000:70000 + 2 * bsz + 13])
    tail = np.ascontiguousarray(synth.make("M", 70000, 1 << 16, seed=5)[-30000:]).copy()
    want = _want_linked(orc, plain, bsz, True, None, tail)
    for form in ("records", "body"):
        recs, _, _, after, before = _call(eng, plain, bsz, True, form, prev_tail=tail, tail_at=(65536, 30000))
        assert recs == want, form
        _untouched(after, before)
        for back in (40000, 30001, 29999, 100):
            with pytest.raises(EngineError) as ei:
                _call(eng, plain, bsz, True, form, prev_tail=tail, tail_at=(back, 30000))
            assert ei.value.code == -1, (form, back)
        recs, _, _, _, _ = _call(eng, plain, bsz, True, form, prev_tail=tail, tail_at=(30000, 30000))       # (ends at src: in place)
        assert recs == want, (form, "in place")


# ---- 8. argument errors -----------------------------------------------------------------------------------------------------------------
def test_gpu_dev_encode_ex_argument_errors(eng, text):
    from plz4_amd._native import EngineError
    bsz = 64 << 10
    plain = np.ascontiguousarray(text["T"][:2 * bsz])
    d = eng.dict_create(np.ascontiguousarray(synth.text(70000, seed=42)))
    tail = np.zeros(65537, np.uint8)
    bad = [dict(linked=False, d=d),                                       # a dictionary, independent blocks, contiguous stride
           dict(linked=True, gap=1), dict(linked=True, gap=65535),        # a stride strictly between bsz and bsz + 65536
           dict(linked=True, prev_tail=tail),                             # prevTailLen 65 537
           dict(linked=False, d=None), dict(linked=False, d=None, gap=65536)]   # nothing outside the block at all
    for kw in bad:
        for form in ("records", "body"):
            with pytest.raises(EngineError) as ei:
                _call(eng, plain, bsz, True, form, **kw)
            assert ei.value.code == -1, (kw.keys(), form)
    with pytest.raises(EngineError) as ei:
        _call(eng, plain, bsz, True, "body", level=3)
    assert ei.value.code == -4
    eng.dict_destroy(d)


# ---- 9. two streams of one ctx, then the linked decode of the body --------------------------------------------------------------------------
def test_gpu_dev_two_streams_and_decode(orc, eng, text, monkeypatch):
    """Two bulk calls enqueued on two streams of one ctx before anything is waited for; plz4hip_dev_decode_records_ex of one body
    gives the plaintext back."""
    import torch
    monkeypatch.setenv("PLZ4HIP_FX_LINKED", "0")
    dev = torch.device("cuda:0")
    bsz, nb = 256 << 10, 5
    plains = [np.ascontiguousarray(text[k][70000:70000 + nb * bsz]) for k in "TM"]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    keep = []
    for plain, st in zip(plains, streams):
        host = np.concatenate([np.full(PAD, POISON, np.uint8), plain, np.zeros(64, np.uint8)])
        d_src = torch.from_numpy(host).to(dev)
        cap = nb * (bsz + 8)
        d_body = torch.zeros(cap + 64, dtype=torch.uint8, device=dev)
        d_off = torch.zeros(nb + 1, dtype=torch.int64, device=dev); d_len = torch.zeros(nb, dtype=torch.int32, device=dev)
        keep.append((d_src, d_body, d_off, d_len, cap))
    torch.cuda.synchronize()
    for (d_src, d_body, d_off, d_len, cap), st in zip(keep, streams):
        eng.dev_encode_body_ex(d_src.data_ptr() + PAD, nb * bsz, bsz, bsz, True, d_body.data_ptr(), cap, d_off.data_ptr(), d_len.data_ptr(),
                               linked=True, stream=st.cuda_stream)
    torch.cuda.synchronize()
    for plain, (d_src, d_body, d_off, d_len, cap) in zip(plains, keep):
        want = b"".join(_want_linked(orc, plain, bsz, True))
        assert int(d_off[nb]) == len(want) and d_body.cpu().numpy()[:len(want)].tobytes() == want
    d_src, d_body, d_off, d_len, cap = keep[1]
    stride = (bsz + 8 + 64 + 15) // 16 * 16
    d_out = torch.zeros(nb * stride + 64, dtype=torch.uint8, device=dev)
    d_res = torch.full((nb,), -7, dtype=torch.int32, device=dev); d_st = torch.full((nb,), -7, dtype=torch.int32, device=dev)
    d_w = torch.zeros(131072, dtype=torch.uint8, device=dev); d_wl = torch.zeros(1, dtype=torch.int32, device=dev)
    eng.dev_decode_records_ex(d_body.data_ptr(), d_off.data_ptr(), nb, bsz, True, d_out.data_ptr(), stride, bsz + 8, d_res.data_ptr(), d_st.data_ptr(),
                              linked=True, windows_ptr=d_w.data_ptr(), window_len_ptr=d_wl.data_ptr(), stream=streams[0].cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert not d_st.cpu().numpy().any() and [int(x) for x in d_res.cpu().numpy()] == [bsz] * nb
    assert np.array_equal(np.concatenate([out[i * stride:i * stride + bsz] for i in range(nb)]), plains[1])
