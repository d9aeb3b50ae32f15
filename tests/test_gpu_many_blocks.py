"""One call of N = 66 049 blocks (tests/manyblocks.py) through every route of the C ABI, bit-exact against the reference.

The rest of the GPU suite looks at the edges of a block; this module looks at the edge of a CALL: a block count that does not fit
16 bits.  The emit stage of every staged encoder has the group's block count in gridDim.y (k_l1_sizes / k_l1_write, k_fxl_sizes /
k_fxl_write, k_hc_gather), the one-wave scans (k_scan, k_scan_from, k_out_len) see tens of thousands of entries, k_move_records runs
with the count in grid.x, k_l1_scan (4 blocks per workgroup) and k_l1_finish (16 per wave) get remainder groups, and levels 3..11
run builder-beside-walk at its default trigger (2048 blocks; nothing in the environment touches it here).  Every entry point must
return PLZ4HIP_OK, every block index is compared, and outputs are pre-filled with a pattern so that a record nobody wrote shows.
Comparisons are whole-array; the per-block search runs only to name the first bad block.

Measured on an MI355X (every engine call prints its own time; run with -s): seconds of the test / of its engine call(s), beside the
single-thread CPU time of the reference for the same leg (tests/manyblocks.py: the same 66 049 calls, no wrappers).
    leg                                   test     engine call       reference
    compress_batch level 1, bound / n     0.50 / 0.16   0.05 / 0.015     0.20
    compress_batch level 2                0.29     0.03              0.68
    compress_batch level 3                1.69     0.43 .. 1.40      0.68    (the first HC call allocates the workspaces)
    compress_batch level 9, bound / n     0.73 / 0.71   0.44 / 0.43      0.77 / 0.71
    compress_batch level 11               0.77     0.44              0.79
    compress_batch level 12               0.92 .. 2.95  0.45 .. 2.47     1.38    (above its reference when it allocates)
    decompress_batch (each capacity)      0.19     0.024             0.09 .. 0.14
    xxh32_batch                           0.03     0.013             0.04
    encode_records level 1 / 2 / 9        0.41 / 0.30 / 0.74   0.18 / 0.03 / 0.44   0.24 / 0.77 / 0.76
    decode_records, checksums on / off    0.43 / 0.38   0.17 / 0.18      0.31 / 0.19
    count sweep (encode + decode), each   0.29     0.03 + 0.03       prefixes of the above
    dev_encode_records + compact, 1 / 2   0.24 / 0.36   0.002 / 0.005    0.22 / 0.80
    dev_encode_body level 1 / 2, groups   0.08 / 0.09 / 0.06   0.004 / 0.005    (cached)
    dev_duplex_body + dev_decode_records  0.50     0.002 + 0.001     (cached)
    dev_compress 1 / 1 one-kernel / 9     0.16 / 0.29 / 0.77   0.001 / 0.001 / 0.42   0.20 / - / 0.86
    dev_encode_records_ex linked 1 / 9    0.18 / 0.90 .. 2.2   0.002 / 0.42 .. 1.7    0.45 / 1.24
    dev_decode_records_ex dict            0.55     0.001             0.92
    mgpu, all four calls                  0.49     0.02 + 0.02 + 0.01 + 0.01   (cached)
The block size stays at the 1 KiB the cases are built around: levels 3 and 12 and linked level 9 pass their reference's time only
in the call that allocates the HC workspace."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import manyblocks as mb
from manyblocks import N, BSZ, FILL, RAW_STRIDE, REC_STRIDE

pytestmark = pytest.mark.gpu
PAD = 65536
I32P = C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def eng():
    from plz4_amd._native import Engine
    for v in ("PLZ4HIP_HC_OVERLAP_OFF", "PLZ4HIP_HC_OVERLAP_MIN", "PLZ4HIP_HC_OVERLAP_GROUPS", "PLZ4HIP_L1_BUDGET_MIB", "PLZ4HIP_L1_FUSED",
              "PLZ4HIP_L1X", "PLZ4HIP_HC_LAZY_OFF", "PLZ4HIP_HOST_CHUNK_MB"):
        assert v not in os.environ, v                                    # (the default triggers are what this module is about)
    e = Engine(0)
    yield e
    e.close()


def _pp(addr):
    a = np.ascontiguousarray(addr, dtype=np.uint64)
    return (C.c_void_p * a.size).from_buffer(a)


def _ip(a):
    assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(I32P)


def _ok(e, rc, what):
    """e: an Engine or a MultiEngine."""
    last = e.L.plz4hip_mgpu_last_error if hasattr(e, "g") else e.L.plz4hip_last_error
    text = (last(e.h) or b"").decode() if rc else ""
    assert rc == 0, "%s returned %d (%s)" % (what, rc, text)


class _Clock:
    def __init__(self, what):
        self.what = what

    def __enter__(self):
        self.t = time.perf_counter(); return self

    def __exit__(self, *exc):
        print("[many blocks] %-52s engine call %.3f s" % (self.what, time.perf_counter() - self.t))


def _same(got, want, lens, what):
    bad = mb.first_bad_row(got, want, lens)
    assert bad is None, "%s: block %d of %d differs (%d bytes)" % (what, bad, got.shape[0], int(lens[bad]))


def _guard(got, lens, what):
    """Nothing written behind the first lens[i] bytes of row i."""
    m = ~mb.mask(lens, got.shape[1])
    if not np.all(got[m] == FILL):
        bad = np.flatnonzero(((got != FILL) & m).any(axis=1))
        pytest.fail("%s: block %d written behind its capacity" % (what, int(bad[0])))


# ---- host buffers, raw blocks

def _compress_batch(call, h, case, caps, level, what, count=N):
    out = mb.rows(count, RAW_STRIDE)
    res = np.full(count, -77, dtype=np.int32)
    caps = np.ascontiguousarray(caps[:count])
    with _Clock(what):
        rc = call(h, count, _pp(case.addr()[:count]), _ip(case.n[:count]), _pp(mb.Rows(out, res).addr()), _ip(caps), level, _ip(res))
    return rc, res, out


def _check_raw(rc_res_out, want, caps, what, e):
    rc, res, out = rc_res_out
    _ok(e, rc, what)
    want_res, want_rows = want
    assert np.array_equal(res, want_res), "%s: result of block %d" % (what, int(np.flatnonzero(res != want_res)[0]))
    _same(out, want_rows.a, want_res, what)
    _guard(out, caps, what)


@pytest.mark.parametrize("cap_kind", ["bound", "n"])
def test_host_compress_level1(eng, ref, cap_kind):
    """plz4hip_compress_batch, level 1 == LZ4_compress_fast, result and bytes, at cap = bound and at cap = n."""
    caps = mb.raw_caps(cap_kind)
    what = "compress_batch level 1 cap=" + cap_kind
    _check_raw(_compress_batch(eng.L.plz4hip_compress_batch, eng.h, mb.ragged(), caps, 1, what), mb.want_raw(1, cap_kind), caps, what, eng)


@pytest.mark.parametrize("level,cap_kind", [(2, "bound"), (3, "bound"), (9, "bound"), (9, "n"), (11, "bound"), (12, "bound")])
def test_host_compress_hc(eng, ref, level, cap_kind):
    """plz4hip_compress_batch at the HC levels == LZ4_compress_HC: level 2 (the staged call with the level-2 walk), 3 (the chain
    alone), 9 (the lists), 11 (the optimal parser in segments) -- these three through builder-beside-walk at its default trigger of
    2048 blocks, in four or more groups of doubling size -- and 12 (the three-phase kernels)."""
    caps = mb.raw_caps(cap_kind)
    what = "compress_batch level %d cap=%s" % (level, cap_kind)
    _check_raw(_compress_batch(eng.L.plz4hip_compress_batch, eng.h, mb.ragged(), caps, level, what), mb.want_raw(level, cap_kind), caps, what, eng)


def _decompress_batch(call, h, comp, caps, what, count=N):
    out = mb.rows(count, REC_STRIDE)
    res = np.full(count, -77, dtype=np.int32)
    caps = np.ascontiguousarray(caps[:count])
    with _Clock(what):
        rc = call(h, count, _pp(comp.addr()[:count]), _ip(comp.n[:count]), _pp(mb.Rows(out, res).addr()), _ip(caps), _ip(res))
    return rc, res, out


@pytest.mark.parametrize("extra", [0, 8])
def test_host_decompress(eng, ref, extra):
    """plz4hip_decompress_batch of the reference's blocks, every 101st damaged (a flipped byte / a byte cut off), capacity n + extra
    and n - 1 for every 97th: LZ4_decompress_safe's return codes, and its bytes wherever it returns them."""
    caps = mb.decode_caps(extra)
    what = "decompress_batch cap=n+%d" % extra
    rc, res, out = _decompress_batch(eng.L.plz4hip_decompress_batch, eng.h, mb.damaged_blocks(), caps, what)
    _ok(eng, rc, what)
    want_res, want_rows = mb.want_decode(extra)
    assert np.array_equal(res, want_res), "%s: code of block %d" % (what, int(np.flatnonzero(res != want_res)[0]))
    _same(out, want_rows.a, want_rows.n, what)
    _guard(out, caps, what)


def test_host_xxh32(eng, orc):
    case = mb.ragged()
    got = np.zeros(N, dtype=np.uint32)
    with _Clock("xxh32_batch"):
        rc = eng.L.plz4hip_xxh32_batch(eng.h, N, _pp(case.addr()), _ip(case.n), got.ctypes.data_as(C.POINTER(C.c_uint32)))
    _ok(eng, rc, "xxh32_batch")
    want = mb.want_xxh32()
    assert np.array_equal(got, want), int(np.flatnonzero(got != want)[0])


# ---- host buffers, records

def _encode_records(call, h, case, level, what, count=N):
    out = mb.rows(count, REC_STRIDE)
    ln = np.full(count, -77, dtype=np.int32)
    with _Clock(what):
        rc = call(h, count, _pp(case.addr()[:count]), _ip(case.n[:count]), BSZ, level, 1, _pp(mb.Rows(out, ln).addr()), _ip(ln))
    return rc, ln, out


def _check_records(rc_ln_out, want, what, e, count=N):
    rc, ln, out = rc_ln_out
    _ok(e, rc, what)
    assert np.array_equal(ln, want.n[:count]), "%s: length of record %d" % (what, int(np.flatnonzero(ln != want.n[:count])[0]))
    _same(out, want.a[:count], want.n[:count], what)
    _guard(out, np.full(count, BSZ + 8, dtype=np.int32), what)


def _decode_records(call, h, recs, checksum, what, count=N):
    out = mb.rows(count, REC_STRIDE)
    res = np.full(count, -77, dtype=np.int32); st = np.full(count, -77, dtype=np.int32)
    with _Clock(what):
        rc = call(h, count, _pp(recs.addr()[:count]), _ip(recs.n[:count]), BSZ, int(checksum), _pp(mb.Rows(out, res).addr()), _ip(res), _ip(st))
    return rc, res, st, out


def _check_decoded(rc_res_st_out, want_res, want_st, want_out, what, e, count=N):
    rc, res, st, out = rc_res_st_out
    _ok(e, rc, what)
    assert np.array_equal(st, want_st[:count]), "%s: status of block %d" % (what, int(np.flatnonzero(st != want_st[:count])[0]))
    assert np.array_equal(res, want_res[:count]), "%s: result of block %d" % (what, int(np.flatnonzero(res != want_res[:count])[0]))
    _same(out, want_out.a[:count], want_out.n[:count], what)
    _guard(out, np.full(count, BSZ + 8, dtype=np.int32), what)


@pytest.mark.parametrize("level", [1, 2, 9])
def test_host_encode_records(eng, ref, orc, level):
    """plz4hip_encode_records(bsz = 1024, block checksums) == blk.CompressToBlk over the reference's encoder: orc.block_record at
    level 1, LZ4_compress_HC at cap = bsz in the same framing at levels 2 and 9.  A content-hash stream rides along at every level:
    it ends up holding xxh32 of the whole plaintext in block order."""
    case = mb.ragged()
    what = "encode_records level %d" % level
    h = eng.hash_create()
    try:
        eng.set_content_hash(h)
        got = _encode_records(eng.L.plz4hip_encode_records, eng.h, case, level, what)
        eng.set_content_hash(None)
        assert eng.hash_sum(h) == mb.content_hash(mb.plaintext_rows("ragged"), case.n), "content hash of the encode call"
    finally:
        eng.set_content_hash(None); eng.hash_destroy(h)
    _check_records(got, mb.want_records(level), what, eng)


@pytest.mark.parametrize("checksum", [True, False])
def test_host_decode_records(eng, ref, orc, checksum):
    """plz4hip_decode_records of the level-1 records, every 89th damaged: a payload byte (hash mismatch: status 1, result 0), the
    size word above bsz + 8 (status 2, result 0), and -- without block checksums -- a payload byte that only liblz4 can object to
    (its code, status 3 when negative; a stored block is copied as it is).  The content-hash stream attached to the call holds the
    blocks with result > 0, in block order."""
    recs, want_res, want_st, want_out = mb.damaged_records(checksum)
    what = "decode_records checksums %s" % ("on" if checksum else "off")
    h = eng.hash_create()
    try:
        eng.set_content_hash(h)
        got = _decode_records(eng.L.plz4hip_decode_records, eng.h, recs, checksum, what)
        eng.set_content_hash(None)
        _check_decoded(got, want_res, want_st, want_out, what, eng)
        assert eng.hash_sum(h) == mb.content_hash(want_out, want_res), "content hash of the decode call"
    finally:
        eng.set_content_hash(None); eng.hash_destroy(h)


@pytest.mark.parametrize("count", [65535, 65536, 65537])
def test_host_records_count_sweep(eng, orc, count):
    """Either side of 2^16: encode_records + decode_records of the first `count` blocks (the expected values are prefixes)."""
    what = "encode_records level 1, %d blocks" % count
    _check_records(_encode_records(eng.L.plz4hip_encode_records, eng.h, mb.ragged(), 1, what, count), mb.want_records(1), what, eng, count)
    recs = mb.want_records(1)
    plain = mb.plaintext_rows("ragged")
    what = "decode_records, %d blocks" % count
    _check_decoded(_decode_records(eng.L.plz4hip_decode_records, eng.h, recs, True, what, count), plain.n, np.zeros(N, dtype=np.int32), plain,
                   what, eng, count)


# ---- device-resident, contiguous form, one stream

class _Dev:
    """The contiguous form on the device behind PAD bytes of scratch, and what the calls below need beside it."""

    def __init__(self):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda:0")
        self.plain = mb.contiguous()
        host = np.full(PAD + self.plain.size + 64, FILL, dtype=np.uint8)
        host[PAD:PAD + self.plain.size] = self.plain
        self.d_buf = torch.from_numpy(host).to(self.dev)
        self.src = self.d_buf.data_ptr() + PAD
        self.stream = torch.cuda.current_stream().cuda_stream

    def full(self, n, value, dtype):
        return self.torch.full((n,), value, dtype=dtype, device=self.dev)

    def put(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def sync(self):
        self.torch.cuda.synchronize()

    def untouched(self):
        assert np.array_equal(self.d_buf[PAD:PAD + self.plain.size].cpu().numpy(), self.plain), "the call wrote into its plaintext"


@pytest.fixture(scope="module")
def dv():
    return _Dev()


def _check_stage(dv, d_stage, d_len, want, what):
    ln = d_len.cpu().numpy()
    assert np.array_equal(ln, want.n), "%s: length of record %d" % (what, int(np.flatnonzero(ln != want.n)[0]))
    _same(d_stage.cpu().numpy().reshape(N, REC_STRIDE), want.a, want.n, what)


def _check_body(dv, d_body, d_off, d_len, want, what):
    body, off = mb.body_of(want)
    got_off = d_off.cpu().numpy()
    assert np.array_equal(d_len.cpu().numpy(), want.n), what + ": recLen"
    assert np.array_equal(got_off, off), "%s: recOff[%d]" % (what, int(np.flatnonzero(got_off != off)[0]))
    got = d_body.cpu().numpy()
    if not np.array_equal(got[:body.size], body):
        at = int(np.flatnonzero(got[:body.size] != body)[0])
        pytest.fail("%s: body differs at byte %d, record %d" % (what, at, int(np.searchsorted(off, at, side="right")) - 1))
    assert np.all(got[body.size:] == FILL), what + ": bytes behind the body"


@pytest.mark.parametrize("level", [1, 2])
def test_dev_encode_records_and_compact(eng, dv, ref, orc, level):
    """plz4hip_dev_encode_records + plz4hip_dev_compact_records (k_scan over N lengths, k_move_records with N in grid.x): recLen,
    recOff[N] and the body are the reference's records back to back."""
    torch = dv.torch
    want = mb.want_records(level, "contiguous")
    assert eng.stage_stride(BSZ) == REC_STRIDE
    d_stage = dv.full(N * REC_STRIDE, FILL, torch.uint8); d_len = dv.full(N, -77, torch.int32)
    d_off = dv.full(N + 1, -77, torch.int64); d_body = dv.full(N * (BSZ + 8) + 64, FILL, torch.uint8)
    what = "dev_encode_records + dev_compact_records level %d" % level
    with _Clock(what):
        _ok(eng, eng.L.plz4hip_dev_encode_records(eng.h, dv.src, dv.plain.size, BSZ, level, 1, d_stage.data_ptr(), d_len.data_ptr(), dv.stream), what)
        _ok(eng, eng.L.plz4hip_dev_compact_records(eng.h, d_stage.data_ptr(), REC_STRIDE, d_len.data_ptr(), N, d_off.data_ptr(), d_body.data_ptr(),
                                                  d_body.numel(), dv.stream), what)
        dv.sync()
    _check_stage(dv, d_stage, d_len, want, what)
    _check_body(dv, d_body, d_off, d_len, want, what)
    dv.untouched()


def _encode_body(e, dv, level, what):
    torch = dv.torch
    d_len = dv.full(N, -77, torch.int32); d_off = dv.full(N + 1, -77, torch.int64); d_body = dv.full(N * (BSZ + 8) + 64, FILL, torch.uint8)
    with _Clock(what):
        _ok(e, e.L.plz4hip_dev_encode_body(e.h, dv.src, dv.plain.size, BSZ, level, 1, d_body.data_ptr(), d_body.numel(), d_off.data_ptr(),
                                          d_len.data_ptr(), dv.stream), what)
        dv.sync()
    return d_body, d_off, d_len


@pytest.mark.parametrize("level", [1, 2])
def test_dev_encode_body(eng, dv, ref, orc, level):
    """plz4hip_dev_encode_body: the records straight into the frame body, their places from k_scan_from over N lengths."""
    what = "dev_encode_body level %d" % level
    _check_body(dv, *_encode_body(eng, dv, level, what), mb.want_records(level, "contiguous"), what)
    dv.untouched()


def test_dev_encode_body_in_groups(dv, orc, monkeypatch, capfd):
    """The same call on a level-1 workspace of 50 MiB: at 2.9 KiB of workspace per 1 KiB block that is four groups, and the body
    scan continues from group to group (k_scan_from with first = 0 behind the first one)."""
    from plz4_amd._native import Engine
    monkeypatch.setenv("PLZ4HIP_L1_BUDGET_MIB", "50")
    monkeypatch.setenv("PLZ4HIP_VERBOSE", "1")
    e = Engine(0)
    try:
        what = "dev_encode_body level 1, 50 MiB of workspace"
        got = _encode_body(e, dv, 1, what)
        text = capfd.readouterr().err
        line = [ln for ln in text.splitlines() if "level 1, %d blocks" % N in ln and "groups of" in ln]
        assert line, text[-500:]
        per = int(line[0].split("groups of")[1].split()[0])
        assert 1 <= per and (N + per - 1) // per >= 3, line[0]
        _check_body(dv, *got, mb.want_records(1, "contiguous"), what)
    finally:
        e.close()


def test_dev_duplex_body_and_decode(eng, dv, orc):
    """plz4hip_dev_duplex_body: encode all N blocks while decoding the body the call before wrote -- both sides at N; then
    plz4hip_dev_decode_records on a body tensor of exactly the body's length."""
    torch = dv.torch
    want = mb.want_records(1, "contiguous")
    body, off = mb.body_of(want)
    plain = mb.plaintext_rows("contiguous")
    what = "dev_encode_body level 1 (the duplex call's decode input)"
    d_body0, d_off0, d_len0 = _encode_body(eng, dv, 1, what)
    _check_body(dv, d_body0, d_off0, d_len0, want, what)
    d_len = dv.full(N, -77, torch.int32); d_off = dv.full(N + 1, -77, torch.int64); d_body = dv.full(N * (BSZ + 8) + 64, FILL, torch.uint8)
    d_out = dv.full(N * REC_STRIDE, FILL, torch.uint8); d_res = dv.full(N, -77, torch.int32); d_st = dv.full(N, -77, torch.int32)
    what = "dev_duplex_body"
    with _Clock(what):
        _ok(eng, eng.L.plz4hip_dev_duplex_body(eng.h, dv.src, dv.plain.size, BSZ, 1, d_body.data_ptr(), d_body.numel(), d_off.data_ptr(), d_len.data_ptr(),
                                              d_body0.data_ptr(), d_off0.data_ptr(), N, BSZ, 1, d_out.data_ptr(), REC_STRIDE, BSZ + 8,
                                              d_res.data_ptr(), d_st.data_ptr(), dv.stream), what)
        dv.sync()
    _check_body(dv, d_body, d_off, d_len, want, what)

    def check_decode(what):
        assert int(d_st.abs().sum().item()) == 0, what + ": status"
        assert np.array_equal(d_res.cpu().numpy(), plain.n), what + ": result"
        out = d_out.cpu().numpy().reshape(N, REC_STRIDE)
        _same(out, plain.a, plain.n, what)
        _guard(out, np.full(N, BSZ + 8, dtype=np.int32), what)

    check_decode(what)
    d_exact = dv.put(body)                                                  # exactly the body: nothing behind the last record
    assert d_exact.numel() == int(off[-1])
    d_offx = dv.put(off)
    d_out.fill_(FILL); d_res.fill_(-77); d_st.fill_(-77)
    what = "dev_decode_records"
    with _Clock(what):
        _ok(eng, eng.L.plz4hip_dev_decode_records(eng.h, d_exact.data_ptr(), d_offx.data_ptr(), N, BSZ, 1, d_out.data_ptr(), REC_STRIDE, BSZ + 8,
                                                 d_res.data_ptr(), d_st.data_ptr(), dv.stream), what)
        dv.sync()
    check_decode(what)


@pytest.mark.parametrize("level,max_len", [(1, BSZ), (1, 0), (9, BSZ)])
def test_dev_compress_and_decompress(eng, dv, ref, level, max_len):
    """plz4hip_dev_compress with the lengths on the device: level 1 staged (the true maxLen), level 1 one-kernel (maxLen = 0), level
    9; with a maxLen, one block whose device-side length is maxLen + 1 comes back as PLZ4HIP_E_ARG with nothing written behind its
    capacity (the kernels see it as an empty block, so its first byte may change), and its neighbours as ever.  plz4hip_dev_decompress takes the blocks back to the plaintext (k_out_len has no part here; results on the device)."""
    torch = dv.torch
    want_res, want = mb.want_raw(level, "bound", "contiguous")
    want_res = want_res.copy()
    sizes = mb.contiguous_sizes()
    odd = 40001
    if max_len:
        sizes[odd] = max_len + 1
        want_res[odd] = -1                                                  # PLZ4HIP_E_ARG
    d_srclen = dv.put(sizes); d_cap = dv.put(mb.raw_caps("bound", "contiguous"))
    d_dst = dv.full(N * RAW_STRIDE, FILL, torch.uint8); d_res = dv.full(N, -77, torch.int32)
    what = "dev_compress level %d maxLen=%d" % (level, max_len)
    with _Clock(what):
        _ok(eng, eng.L.plz4hip_dev_compress(eng.h, N, dv.src, BSZ, d_srclen.data_ptr(), d_dst.data_ptr(), RAW_STRIDE, d_cap.data_ptr(), level, max_len,
                                           d_res.data_ptr(), dv.stream), what)
        dv.sync()
    res = d_res.cpu().numpy()
    assert np.array_equal(res, want_res), "%s: result of block %d" % (what, int(np.flatnonzero(res != want_res)[0]))
    out = d_dst.cpu().numpy().reshape(N, RAW_STRIDE)
    _same(out, want.a, want_res, what)
    _guard(out, mb.raw_caps("bound", "contiguous"), what)                    # (the refused block too: nothing behind its capacity)
    dv.untouched()
    # and back: the engine's own blocks (they are the reference's), lengths and capacities on the device
    good = mb.want_raw(level, "bound", "contiguous")[0]
    d_good = dv.put(good); d_n = dv.put(mb.contiguous_sizes())
    d_out = dv.full(N * REC_STRIDE, FILL, torch.uint8); d_res2 = dv.full(N, -77, torch.int32)
    if max_len:
        d_dst[odd * RAW_STRIDE:(odd + 1) * RAW_STRIDE] = dv.put(want.a[odd])
    what = "dev_decompress (level-%d blocks)" % level
    with _Clock(what):
        _ok(eng, eng.L.plz4hip_dev_decompress(eng.h, N, d_dst.data_ptr(), RAW_STRIDE, d_good.data_ptr(), d_out.data_ptr(), REC_STRIDE, d_n.data_ptr(),
                                             d_res2.data_ptr(), dv.stream), what)
        dv.sync()
    plain = mb.plaintext_rows("contiguous")
    assert np.array_equal(d_res2.cpu().numpy(), plain.n), what + ": result"
    out = d_out.cpu().numpy().reshape(N, REC_STRIDE)
    _same(out, plain.a, plain.n, what)
    _guard(out, plain.n, what)


# ---- history outside the block, device-resident

@pytest.mark.parametrize("level", [1, 9])
def test_dev_linked_records(eng, dv, ref, orc, level):
    """plz4hip_dev_encode_records_ex(linked = 1, contiguous plaintext, no dictionary): level 1 is the staged one-wave-per-block route
    (k_l1x_parse, then k_fxl_sizes / k_fxl_write with the group's block count in y), level 9 the HC design over segment + block.
    Expected: orc.compress_linked / liblz4's linked HC stream as tests/hcdict.py drives it."""
    torch = dv.torch
    want = mb.want_linked_records(level)
    d_stage = dv.full(N * REC_STRIDE, FILL, torch.uint8); d_len = dv.full(N, -77, torch.int32)
    before = eng.counters()["l1x_blocks"]
    what = "dev_encode_records_ex linked level %d" % level
    with _Clock(what):
        _ok(eng, eng.L.plz4hip_dev_encode_records_ex(eng.h, dv.src, dv.plain.size, BSZ, BSZ, level, 1, 1, None, None, -1, d_stage.data_ptr(),
                                                    d_len.data_ptr(), dv.stream), what)
        dv.sync()
    _check_stage(dv, d_stage, d_len, want, what)
    dv.untouched()
    if level == 1:
        assert eng.counters()["l1x_blocks"] > before                        # (the staged route took the call, not the one-kernel encoder)


def test_dev_dict_decode(eng, dv, orc):
    """plz4hip_dev_decode_records_ex(linked = 0, dict) over N independent blocks the oracle encoded under a dictionary
    (orc.compress_indie_dict) == orc.decompress_safe_dict of every payload."""
    torch = dv.torch
    recs, want_res, want_out = mb.want_dict_records()
    body, off = mb.body_of(recs)
    dct = mb.dictionary()
    d = eng.dict_create(dct)
    try:
        d_body = dv.put(body); d_off = dv.put(off)
        d_out = dv.full(N * REC_STRIDE, FILL, torch.uint8); d_res = dv.full(N, -77, torch.int32); d_st = dv.full(N, -77, torch.int32)
        what = "dev_decode_records_ex dict"
        with _Clock(what):
            _ok(eng, eng.L.plz4hip_dev_decode_records_ex(eng.h, d_body.data_ptr(), d_off.data_ptr(), N, BSZ, 1, 0, d, 1, None, None, None,
                                                        d_out.data_ptr(), REC_STRIDE, BSZ + 8, d_res.data_ptr(), d_st.data_ptr(), dv.stream), what)
            dv.sync()
        assert int(d_st.abs().sum().item()) == 0, what + ": status"
        assert np.array_equal(d_res.cpu().numpy(), want_res), what + ": result"
        out = d_out.cpu().numpy().reshape(N, REC_STRIDE)
        _same(out, want_out.a, want_out.n, what)
        _guard(out, np.full(N, BSZ + 8, dtype=np.int32), what)
    finally:
        eng.dict_destroy(d)


# ---- plz4hip_mgpu: block i on entry i mod 3

def test_mgpu_all_four_calls(ref, orc):
    """MultiEngine([0, 0, 0]): encode_records, decode_records, compress_batch and decompress_batch of all N blocks, 22 017 / 22 016
    / 22 016 to an entry, results back in block order."""
    from plz4_amd._native import MultiEngine
    m = MultiEngine([0, 0, 0])
    try:
        case = mb.ragged()
        what = "mgpu encode_records"
        _check_records(_encode_records(m.L.plz4hip_mgpu_encode_records, m.h, case, 1, what), mb.want_records(1), what, m)
        recs, want_res, want_st, want_out = mb.damaged_records(True)
        what = "mgpu decode_records"
        _check_decoded(_decode_records(m.L.plz4hip_mgpu_decode_records, m.h, recs, True, what), want_res, want_st, want_out, what, m)
        caps = mb.raw_caps("n")
        what = "mgpu compress_batch cap=n"
        _check_raw(_compress_batch(m.L.plz4hip_mgpu_compress_batch, m.h, case, caps, 1, what), mb.want_raw(1, "n"), caps, what, m)
        caps = mb.decode_caps(8)
        what = "mgpu decompress_batch"
        rc, res, out = _decompress_batch(m.L.plz4hip_mgpu_decompress_batch, m.h, mb.damaged_blocks(), caps, what)
        _ok(m, rc, what)
        want_res, want_rows = mb.want_decode(8)
        assert np.array_equal(res, want_res), "%s: code of block %d" % (what, int(np.flatnonzero(res != want_res)[0]))
        _same(out, want_rows.a, want_rows.n, what)
        _guard(out, caps, what)
    finally:
        m.close()
