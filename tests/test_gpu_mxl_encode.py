"""The few-block level-2 path on blocks with history outside the block, on the GPU (MxlFlavour of plz4_amd/csrc/lz4_mx_device.inl
behind launch_l1): level-2 calls of a handful of linked blocks and / or blocks under a dictionary have their LZ4MID walk cut across
the chip behind every block's external segment, and every entry point that takes the route must give the bytes of the real liblz4
driven as clz4.go drives it (tests/hcdict.py), exactly as one wave per block does.  Every case sets PLZ4HIP_MXL_MAX_BLOCKS itself
(the switches are read per call) and checks by the mxl_blocks delta of plz4hip_ctx_counters that the route took exactly the blocks
it should: a silent fallback fails the test."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import hcdict
from plz4_amd import synth
from test_gpu_dev_encode_ex import PAD, _call, _untouched, _want_linked

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
N = 200 * 1024 + 13
K256 = 256 << 10
BSZ = 4 << 20


def _bound(n):
    return n + n // 255 + 16


def _env(mp, limit="8", piece="8", warm="16"):
    mp.setenv("PLZ4HIP_MXL_MAX_BLOCKS", limit)
    if piece is not None:
        mp.setenv("PLZ4HIP_MX_PIECE_KIB", piece)
        mp.setenv("PLZ4HIP_MX_WARMUP_KIB", warm)


@pytest.fixture(scope="module")
def eng():
    from plz4_amd._native import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def dict64():
    d = np.ascontiguousarray(synth.text(65536, seed=77))
    d.setflags(write=False)
    return d


@pytest.fixture(scope="module")
def frame():
    """Four linked blocks: 256 KiB of text; 200 KiB + 13 that begin with a copy of the last 60 KiB of the block before them -- their
    segment -- and go on as text of the same vocabulary (the twin-of-segment block of tests/test_mxl_encode.py); 256 KiB of random
    bytes (comes back stored); 9 000 bytes (one piece).  Computed once, never written to."""
    t = synth.text(K256 + N, seed=61)
    b0 = np.ascontiguousarray(t[:K256])
    b1 = np.ascontiguousarray(np.concatenate([b0[-(60 << 10):], t[K256:K256 + N - (60 << 10)]]))
    out = [b0, b1, np.ascontiguousarray(synth.random_bytes(K256, seed=62)), np.ascontiguousarray(synth.text(9000, seed=63))]
    for b in out:
        b.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def plain():
    """Two blocks of 256 KiB and one of 200 KiB + 13, back to back."""
    p = np.ascontiguousarray(synth.make("M", 2 * K256 + N, 1 << 16, seed=64))
    p.setflags(write=False)
    return p


def _delta(eng, c0):
    c1 = eng.counters()
    return {k: c1[k] - c0[k] for k in ("mxl_blocks", "mx_blocks", "hcx_blocks", "fxl_blocks", "dxl_blocks")} | {"rounds": c1["mx_rounds_last"]}


def _cut(data, bsz):
    return [np.ascontiguousarray(data[o:o + bsz]) for o in range(0, data.size, bsz)]


# ---- 1. encode_records_ex, linked ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", [False, True])
@pytest.mark.parametrize("variant", ["plain", "dict", "prev_tail"])
def test_gpu_mxl_encode_records_ex_linked(ref, orc, eng, frame, dict64, monkeypatch, variant, cs):
    _env(monkeypatch)
    blocks = [b.copy() for b in frame]
    d = eng.dict_create(dict64.copy()) if variant == "dict" else None
    tail = None
    if variant == "prev_tail":                                            # (the frame goes on behind a block that was written before)
        before = np.ascontiguousarray(synth.text(100000, seed=65))
        tail = before[-65536:].copy()
        want, _ = hcdict.ref_records(ref, orc, [before] + blocks, K256, 2, True, None, checksum=cs)
        want = want[1:]
    else:
        want, _ = hcdict.ref_records(ref, orc, blocks, K256, 2, True, dict64.copy() if d is not None else None, checksum=cs)
    c0 = eng.counters()
    recs = eng.encode_records_ex(blocks, K256, cs, linked=True, d=d, prev_tail=tail, level=2)
    dl = _delta(eng, c0)
    assert dl["mxl_blocks"] == 4 and dl["mx_blocks"] == 4 and dl["hcx_blocks"] == 0 and dl["rounds"] >= 1, dl
    for i, (r, w) in enumerate(zip(recs, want)):
        assert r.tobytes() == w, (variant, cs, i)
    assert recs[2][3] & 0x80 and not recs[0][3] & 0x80                    # the random block is stored
    if d is not None:
        eng.dict_destroy(d)


# ---- 2. independent blocks against a dictionary -----------------------------------------------------------------------------------------
def test_gpu_mxl_encode_records_ex_dictionary_independent(ref, orc, eng, frame, dict64, monkeypatch):
    """One block of at most 4 KiB in the call: that one is k_hcx's, the others the route's."""
    _env(monkeypatch)
    blocks = [frame[1].copy(), np.ascontiguousarray(synth.text(4000, seed=66)), frame[0].copy()]
    d = eng.dict_create(dict64.copy())
    for cs in (False, True):
        want, _ = hcdict.ref_records(ref, orc, blocks, K256, 2, False, dict64.copy(), checksum=cs)
        c0 = eng.counters()
        recs = eng.encode_records_ex(blocks, K256, cs, linked=False, d=d, level=2)
        dl = _delta(eng, c0)
        assert dl["hcx_blocks"] == 1 and dl["mxl_blocks"] == 2 and dl["mx_blocks"] == 2, dl
        for i, (r, w) in enumerate(zip(recs, want)):
            assert r.tobytes() == w, (cs, i)
    eng.dict_destroy(d)


# ---- 3. compress_batch_dict ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 3])
def test_gpu_mxl_compress_batch_dict_capacities(ref, eng, frame, dict64, monkeypatch, nb):
    """Capacity bound, n and one below the compressed size (result 0); no byte behind dstCap is touched."""
    from plz4_amd._native import _i32, _i32p, _ptr_array
    _env(monkeypatch)
    srcs = [frame[1].copy(), frame[0].copy(), np.ascontiguousarray(synth.make("M", N, 1 << 14, seed=67))][:nb]
    keep, daddr = ref.new_dict_ctx_hc(dict64.copy(), 2)
    comp = ref.stream_ctx_hc(2, daddr)
    sizes = [comp(s, _bound(s.size))[0] for s in srcs]
    d = eng.dict_create(dict64.copy())
    for caps in ([_bound(s.size) for s in srcs], [s.size for s in srcs], [c - 1 for c in sizes]):
        dsts = [np.full(cap + 256, 0xA5, dtype=np.uint8) for cap in caps]
        res = np.full(nb, -7, dtype=np.int32)
        lens = _i32([s.size for s in srcs]); capa = _i32(caps)
        c0 = eng.counters()
        eng._chk(eng.L.plz4hip_compress_batch_dict(eng.h, nb, _ptr_array(srcs), _i32p(lens), _ptr_array(dsts), _i32p(capa), 2, d, _i32p(res)))
        dl = _delta(eng, c0)
        assert dl["mxl_blocks"] == nb and dl["mx_blocks"] == nb, dl
        for i, (s, cap, o) in enumerate(zip(srcs, caps, dsts)):
            want, wc = comp(s, cap)
            assert int(res[i]) == want == (0 if cap < sizes[i] else sizes[i]), (i, cap, int(res[i]), want)
            assert np.array_equal(o[:want], wc[:want]), (i, cap)
            assert np.all(o[cap:] == 0xA5), (i, cap)
    eng.dict_destroy(d)


# ---- 4. the device-resident calls ------------------------------------------------------------------------------------------------------------
def _check_forms(eng, plain, bsz, cs, want, **kw):
    """records and body form of one call against `want`; returns the source buffers (after, before) of both"""
    bufs = []
    for form in ("records", "body"):
        recs, rl, off, after, before = _call(eng, plain, bsz, cs, form, level=2, **kw)
        assert recs == want, (form, cs, kw.keys())
        assert [int(x) for x in rl] == [len(w) for w in want], form
        if off is not None:
            assert [int(x) for x in off] == [0] + list(np.cumsum([len(w) for w in want])), form
        bufs.append((after, before))
    return bufs


def test_gpu_mxl_dev_calls_linked_contiguous(ref, orc, eng, plain, monkeypatch):
    _env(monkeypatch)
    blocks = [b.copy() for b in _cut(plain, K256)]
    for cs in (False, True):
        want, _ = hcdict.ref_records(ref, orc, blocks, K256, 2, True, None, checksum=cs)
        c0 = eng.counters()
        bufs = _check_forms(eng, plain.copy(), K256, cs, want, linked=True)
        assert _delta(eng, c0)["mxl_blocks"] == 2 * 3
        for after, before in bufs:
            _untouched(after, before)                                     # (only the 64 KiB in front of block 0 are the engine's)


def test_gpu_mxl_dev_calls_dictionary_gapped(ref, orc, eng, plain, dict64, monkeypatch):
    """Independent blocks under the dictionary, 64 KiB + 48 of scratch in front of every block: outside the 64 KiB in front of each
    block no byte of src changes."""
    _env(monkeypatch)
    gap = 65536 + 48
    blocks = [b.copy() for b in _cut(plain, K256)]
    d = eng.dict_create(dict64.copy())
    want, _ = hcdict.ref_records(ref, orc, blocks, K256, 2, False, dict64.copy(), checksum=True)
    c0 = eng.counters()
    bufs = _check_forms(eng, plain.copy(), K256, True, want, linked=False, d=d, gap=gap)
    dl = _delta(eng, c0)
    assert dl["mxl_blocks"] == 2 * 3 and dl["hcx_blocks"] == 0, dl
    mine = np.ones(bufs[0][0].size, dtype=bool)                           # True: not the engine's to write
    for i in range(len(blocks)):
        at = PAD + i * (K256 + gap)
        mine[at - 65536:at] = False
    for after, before in bufs:
        assert np.array_equal(after[mine], before[mine])
    eng.dict_destroy(d)


# ---- 5. full size at the default cut ------------------------------------------------------------------------------------------------------------
def test_gpu_mxl_two_linked_4mib_blocks_at_the_default_cut(ref, orc, eng, dict64, monkeypatch):
    _env(monkeypatch, limit="16", piece=None)
    monkeypatch.delenv("PLZ4HIP_MX_PIECE_KIB", raising=False)
    monkeypatch.delenv("PLZ4HIP_MX_WARMUP_KIB", raising=False)
    blocks = _cut(np.ascontiguousarray(synth.text(2 * BSZ, seed=68)), BSZ)
    d = eng.dict_create(dict64.copy())
    want, _ = hcdict.ref_records(ref, orc, blocks, BSZ, 2, True, dict64.copy(), checksum=True)
    c0 = eng.counters()
    recs = eng.encode_records_ex(blocks, BSZ, True, linked=True, d=d, level=2)
    dl = _delta(eng, c0)
    assert dl["mxl_blocks"] == 2 and 1 <= dl["rounds"] <= 32, dl
    for i, (r, w) in enumerate(zip(recs, want)):
        assert r.tobytes() == w, i
    eng.dict_destroy(d)


# ---- 6. the limit ----------------------------------------------------------------------------------------------------------------------------------
def test_gpu_mxl_limit_plus_one_blocks(ref, orc, eng, plain, monkeypatch):
    """The limit at 2: a call of 3 blocks keeps one wave per block (counters unchanged), a call of 2 takes the pieces; equal bytes."""
    _env(monkeypatch, limit="2")
    blocks = [b.copy() for b in _cut(plain, K256)]
    want, _ = hcdict.ref_records(ref, orc, blocks, K256, 2, True, None, checksum=True)
    c0 = eng.counters()
    recs3 = eng.encode_records_ex(blocks, K256, True, linked=True, level=2)
    dl = _delta(eng, c0)
    assert dl["mxl_blocks"] == 0 and dl["mx_blocks"] == 0, dl
    c0 = eng.counters()
    recs2 = eng.encode_records_ex(blocks[:2], K256, True, linked=True, level=2)
    assert _delta(eng, c0)["mxl_blocks"] == 2
    assert [r.tobytes() for r in recs3] == want and [r.tobytes() for r in recs2] == want[:2]


_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from plz4_amd import synth
from plz4_amd._native import Engine
e = Engine(0)
k = 256 << 10
data = np.ascontiguousarray(synth.make("M", 2 * k + 200 * 1024 + 13, 1 << 16, seed=64))
blocks = [np.ascontiguousarray(data[o:o + k]) for o in range(0, data.size, k)]
d = e.dict_create(np.ascontiguousarray(synth.text(65536, seed=77)))
recs = e.encode_records_ex(blocks, k, True, linked=True, d=d, level=2)
res, outs = e.compress_batch_dict(blocks, [b.size + b.size // 255 + 16 for b in blocks], d, level=2)
np.save(sys.argv[2], np.concatenate(recs + outs))
print(json.dumps({"res": [int(r) for r in res], "counters": e.counters()}))
e.close()
"""


def test_gpu_mxl_off_gives_the_same_bytes(eng, plain, dict64, tmp_path, monkeypatch):
    """PLZ4HIP_MXL_MAX_BLOCKS=0 in a fresh child process: one wave per block, counter 0, the same bytes as the pieces give here."""
    _env(monkeypatch)
    blocks = [b.copy() for b in _cut(plain, K256)]
    d = eng.dict_create(dict64.copy())
    c0 = eng.counters()
    recs = eng.encode_records_ex(blocks, K256, True, linked=True, d=d, level=2)
    res, outs = eng.compress_batch_dict(blocks, [_bound(b.size) for b in blocks], d, level=2)
    assert _delta(eng, c0)["mxl_blocks"] == 6
    mine = np.concatenate(recs + outs)
    eng.dict_destroy(d)
    env = dict(os.environ, PLZ4HIP_MXL_MAX_BLOCKS="0")
    out = str(tmp_path / "off.npy")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, out], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got["counters"]["mxl_blocks"] == 0 and got["counters"]["mx_blocks"] == 0
    assert got["res"] == [int(r) for r in res]
    assert np.array_equal(np.load(out), mine)


# ---- 7. one ctx in sequence -------------------------------------------------------------------------------------------------------------------------
def test_gpu_mxl_one_ctx_in_sequence_and_workspace_given_back(ref, orc, plain, dict64, monkeypatch):
    """One ctx: mxl call, independent mx call, level-1 linked few-block call, level-9 dictionary call, few-block decode of the records
    just written back to the plaintext, trim, mxl call, close.  Every result right; after trim and after close the device memory is
    back (the tolerance of test_gpu_mx_one_ctx_in_sequence_and_workspace_given_back)."""
    import torch
    from plz4_amd._native import Engine
    _env(monkeypatch)
    monkeypatch.setenv("PLZ4HIP_MX_MAX_BLOCKS", "8")
    torch.cuda.init()
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    e = Engine(0)
    blocks = [b.copy() for b in _cut(plain, K256)]
    d = e.dict_create(dict64.copy())
    want2, _ = hcdict.ref_records(ref, orc, blocks, K256, 2, True, dict64.copy(), checksum=True)
    c0 = e.counters()
    recs = e.encode_records_ex(blocks, K256, True, linked=True, d=d, level=2)                 # the route
    assert [r.tobytes() for r in recs] == want2
    free1, _ = torch.cuda.mem_get_info()
    res, outs = e.compress_batch(blocks, [_bound(b.size) for b in blocks], level=2)          # independent blocks: mx
    for b, r, o in zip(blocks, res, outs):
        w, comp = ref.compress_hc(b, _bound(b.size), 2)
        assert int(r) == w and np.array_equal(o, comp[:w])
    recs1 = e.encode_records_ex(blocks, K256, True, linked=True, level=1)                     # level 1, linked, few blocks: fxl
    assert [r.tobytes() for r in recs1] == _want_linked(orc, plain, K256, True)
    want9, _ = hcdict.ref_records(ref, orc, blocks, K256, 9, True, dict64.copy(), checksum=True)
    recs9 = e.encode_records_ex(blocks, K256, True, linked=True, d=d, level=9)
    assert [r.tobytes() for r in recs9] == want9
    compressed = 0
    for written in (recs9, recs):                                          # the few-block decoder: linked, the window starts as the dictionary
        rd, st, dec, _ = e.decode_records_ex([r.copy() for r in written], K256, True, linked=True, window=dict64.copy(), window_len=65536)
        assert not any(int(x) for x in st) and [int(x) for x in rd] == [b.size for b in blocks]
        assert all(np.array_equal(x, b) for x, b in zip(dec, blocks))
        compressed += sum(not (r[3] & 0x80) for r in written)
    c1 = e.counters()
    moved = {k: c1[k] - c0[k] for k in ("mxl_blocks", "mx_blocks", "fxl_blocks", "dxl_blocks")}
    assert compressed == 6 and moved == {"mxl_blocks": 3, "mx_blocks": 6, "fxl_blocks": 3, "dxl_blocks": 6}, moved
    e.trim()
    torch.cuda.synchronize()
    free2, _ = torch.cuda.mem_get_info()
    assert free1 < free0                                                    # (the calls held their workspaces)
    assert free2 >= free0 - (64 << 20), (free0 >> 20, free1 >> 20, free2 >> 20)
    recs = e.encode_records_ex(blocks, K256, True, linked=True, d=d, level=2)
    assert [r.tobytes() for r in recs] == want2
    assert e.counters()["mxl_blocks"] - c0["mxl_blocks"] == 6
    e.dict_destroy(d)
    e.close()
    torch.cuda.synchronize()
    free3, _ = torch.cuda.mem_get_info()
    assert free3 >= free0 - (64 << 20), (free0 >> 20, free3 >> 20)


# ---- 8. two streams of one ctx ---------------------------------------------------------------------------------------------------------------------
def test_gpu_mxl_two_streams_of_one_ctx(ref, orc, eng, plain, monkeypatch):
    """Two dev_encode_records_ex calls enqueued on two streams before either is waited for: the second waits for the pieces'
    workspace on the device; both right."""
    import torch
    _env(monkeypatch)
    dev = torch.device("cuda:0")
    other = np.ascontiguousarray(synth.text(plain.size, seed=69))
    plains = [plain.copy(), other]
    nb = -(-plain.size // K256)
    sstride = eng.stage_stride(K256)
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    keep = []
    for p in plains:
        host = np.concatenate([np.full(PAD, 0xA7, np.uint8), p, np.zeros(256, np.uint8)])
        keep.append((torch.from_numpy(host).to(dev), torch.zeros(nb * sstride + 64, dtype=torch.uint8, device=dev),
                     torch.full((nb,), -7, dtype=torch.int32, device=dev)))
    torch.cuda.synchronize()
    c0 = eng.counters()
    for p, st, (d_src, d_stage, d_len) in zip(plains, streams, keep):
        eng.dev_encode_records_ex(d_src.data_ptr() + PAD, p.size, K256, K256, True, d_stage.data_ptr(), d_len.data_ptr(), linked=True,
                                  stream=st.cuda_stream, level=2)
    torch.cuda.synchronize()
    assert _delta(eng, c0)["mxl_blocks"] == 2 * nb
    for p, (d_src, d_stage, d_len) in zip(plains, keep):
        want, _ = hcdict.ref_records(ref, orc, [b.copy() for b in _cut(p, K256)], K256, 2, True, None, checksum=True)
        rl, stage = d_len.cpu().numpy(), d_stage.cpu().numpy()
        assert [stage[i * sstride:i * sstride + int(rl[i])].tobytes() for i in range(nb)] == want
