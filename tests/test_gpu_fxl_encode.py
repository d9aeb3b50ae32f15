"""The few-block level-1 path for blocks with history outside the block on the GPU (the kExt flavour of lz4_fx_device.inl behind
launch_l1): linked blocks and blocks under a dictionary context, a few of them per call, through the C ABI.  Every record / block
must be the oracle's stream emulation (compress_linked / compress_indie_dict), byte for byte, and the counter fxl_blocks of
plz4hip_ctx_counters shows that the path ran."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from plz4_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from plz4_amd._native import Engine
    e = Engine(0)
    yield e
    e.close()


def _record(orc, comp_ret, comp, src, checksum):
    """blk.CompressToBlk framing of one encoder result (blk.go:78-109)."""
    if comp_ret == 0:
        payload, word = src, 0x80000000 | src.size
    else:
        payload, word = comp, comp.size
    rec = np.uint32(word).tobytes() + payload.tobytes()
    if checksum:
        rec += np.uint32(orc.xxh32(payload)).tobytes()
    return rec


def _want_linked(orc, blocks, bsz, cs, dctx=None, prev=None):
    out = []
    for b in blocks:
        tail = None if prev is None else prev[-65536:].copy()
        r, c = orc.compress_linked(b, bsz, tail, dctx if prev is None else None)
        out.append(_record(orc, r, c, b, cs)); prev = b
    return out


def _blocks(sizes, seed):
    data = synth.make("M", sum(sizes), 1 << 16, seed=seed)
    out, o = [], 0
    for n in sizes:
        out.append(data[o:o + n].copy()); o += n
    return out


def _fxl(eng, c0):
    c1 = eng.counters()
    return c1["fxl_blocks"] - c0["fxl_blocks"], c1["fx_blocks"] - c0["fx_blocks"]


SIZES = {1: [262161], 3: [100000, 262161, 131072], 16: [100000 + 10135 * i for i in range(16)]}


@pytest.mark.parametrize("nb", [1, 3, 16])
@pytest.mark.parametrize("with_dict", [False, True])
def test_gpu_fxl_encode_records_ex(orc, eng, monkeypatch, nb, with_dict):
    """Linked records with and without a dictionary, checksums on and off, 4 KiB pieces; the batch again as two calls with the tail
    carried."""
    monkeypatch.setenv("PLZ4HIP_FX_PIECE_KIB", "4")
    bsz = 1 << 20
    user = synth.text(70000, seed=42)
    blocks = _blocks(SIZES[nb], seed=nb)
    dctx = orc.dict_ctx(user) if with_dict else None
    d = eng.dict_create(np.ascontiguousarray(user)) if with_dict else None
    for cs in (False, True):
        want = _want_linked(orc, blocks, bsz, cs, dctx)
        c0 = eng.counters()
        got = eng.encode_records_ex(blocks, bsz, cs, linked=True, d=d)
        fxl, fx = _fxl(eng, c0)
        assert fxl == nb and fx == nb, (fxl, fx)
        assert [g.tobytes() for g in got] == want, (nb, with_dict, cs)
    if nb > 1:
        cut = nb // 2
        c0 = eng.counters()
        got = eng.encode_records_ex(blocks[:cut], bsz, True, linked=True, d=d)
        got += eng.encode_records_ex(blocks[cut:], bsz, True, linked=True, d=d, prev_tail=blocks[cut - 1][-65536:].copy())
        assert _fxl(eng, c0)[0] == nb
        assert [g.tobytes() for g in got] == _want_linked(orc, blocks, bsz, True, dctx)
    if d is not None:
        eng.dict_destroy(d)


@pytest.mark.parametrize("dlen", [70000, 30000, 5])
def test_gpu_fxl_compress_batch_dict(orc, eng, dlen):
    """The block API with a dictionary: blocks on both sides of the 4 KiB switch (the small ones keep the two-table encoder, behind
    the emit stage) beside large ones in one call."""
    user = synth.text(70000, seed=99)[:dlen].copy()
    data = synth.text(300000, seed=7)
    dctx = orc.dict_ctx(user)
    d = eng.dict_create(np.ascontiguousarray(user))
    sizes = (0, 5, 4096, 4097, 65547, 200000)
    srcs = [data[:n].copy() for n in sizes]
    on_path = sum(1 for n in sizes if n > 4096) if dlen >= 8 else len(sizes)
    for caps in ([orc.bound(n) for n in sizes], [max(n, 1) for n in sizes], [max(n // 3, 1) for n in sizes]):
        c0 = eng.counters()
        res, outs = eng.compress_batch_dict(srcs, caps, d)
        assert _fxl(eng, c0)[0] == on_path
        for s, c, r, o in zip(srcs, caps, res, outs):
            a, da = orc.compress_indie_dict(s, c, dctx)
            assert int(r) == a and np.array_equal(o, da), (dlen, s.size, c)
    eng.dict_destroy(d)


@pytest.mark.parametrize("kind,nb", [("T", 1), ("T", 3), ("M", 3)])
def test_gpu_fxl_full_size_blocks(orc, eng, kind, nb):
    """Linked 4 MiB blocks behind a 64 KiB dictionary at the default pieces: indices above 2^22."""
    bsz = 4 << 20
    user = synth.text(65536, seed=77)
    data = synth.make(kind, nb * bsz, bsz, seed=21)
    blocks = [data[o:o + bsz].copy() for o in range(0, data.size, bsz)]
    dctx = orc.dict_ctx(user); d = eng.dict_create(np.ascontiguousarray(user))
    c0 = eng.counters()
    got = eng.encode_records_ex(blocks, bsz, True, linked=True, d=d)
    assert _fxl(eng, c0)[0] == nb
    assert [g.tobytes() for g in got] == _want_linked(orc, blocks, bsz, True, dctx), (kind, nb)
    eng.dict_destroy(d)


def test_gpu_fxl_groups_and_chunks(orc, monkeypatch):
    """A linked call cut into workspace groups (block g0 still gets the tail of block g0 - 1) and into staging chunks: the bytes of
    the call in one piece."""
    from plz4_amd._native import Engine
    bsz = 1 << 20
    user = synth.text(70000, seed=4)
    blocks = _blocks([262161 - 7 * i for i in range(6)], seed=31)
    whole = None
    for env in (None, ("PLZ4HIP_L1_BUDGET_MIB", "1"), ("PLZ4HIP_HOST_CHUNK_MB", "1")):
        if env:
            monkeypatch.setenv(*env)
        e = Engine(0)                                                       # (a fresh ctx: no workspace from an earlier call)
        d = e.dict_create(np.ascontiguousarray(user))
        c0 = e.counters()
        got = [g.tobytes() for g in e.encode_records_ex(blocks, bsz, True, linked=True, d=d)]
        assert _fxl(e, c0)[0] == len(blocks), env
        e.dict_destroy(d); e.close()
        if env:
            monkeypatch.delenv(env[0])
            assert got == whole, env
        else:
            whole = got
    assert whole == _want_linked(orc, blocks, bsz, True, orc.dict_ctx(user))


_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from plz4_amd import synth
from plz4_amd._native import Engine
e = Engine(0)
user = np.ascontiguousarray(synth.text(70000, seed=8))
d = e.dict_create(user)
data = synth.make("M", 3 * 262161 + 5000, 1 << 16, seed=9)
blocks = [data[o:o + 262161].copy() for o in range(0, data.size, 262161)]
recs = e.encode_records_ex(blocks, 1 << 20, True, linked=True, d=d)
res, outs = e.compress_batch_dict(blocks, [262161] * len(blocks), d)
np.save(sys.argv[2], np.concatenate(recs + outs))
print(json.dumps({"res": [int(r) for r in res], "counters": e.counters()}))
e.dict_destroy(d)
e.close()
"""


@pytest.mark.parametrize("switch", ["PLZ4HIP_FX_LINKED", "PLZ4HIP_FX_MAX_BLOCKS"])
def test_gpu_fxl_off_gives_the_same_bytes(eng, tmp_path, switch):
    """Either switch at 0 (in a child process): the one-wave kernels, the same bytes."""
    user = np.ascontiguousarray(synth.text(70000, seed=8))
    d = eng.dict_create(user)
    data = synth.make("M", 3 * 262161 + 5000, 1 << 16, seed=9)
    blocks = [data[o:o + 262161].copy() for o in range(0, data.size, 262161)]
    c0 = eng.counters()
    recs = eng.encode_records_ex(blocks, 1 << 20, True, linked=True, d=d)
    res, outs = eng.compress_batch_dict(blocks, [262161] * len(blocks), d)
    assert _fxl(eng, c0)[0] == 2 * len(blocks)
    eng.dict_destroy(d)
    mine = np.concatenate(recs + outs)
    out = str(tmp_path / "off.npy")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, out], env=dict(os.environ, **{switch: "0"}), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got["counters"]["fxl_blocks"] == 0
    assert got["res"] == [int(r) for r in res]
    assert np.array_equal(np.load(out), mine)


def test_gpu_fxl_one_ctx_call_mix(orc):
    """One ctx: a few-block linked encode, a bulk linked encode (more than 128 small blocks), the few-block linked decode of what
    was written, a few-block linked encode again; trim and close give the device memory back."""
    import torch
    from plz4_amd._native import Engine
    torch.cuda.init()
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    e = Engine(0)
    bsz = 256 << 10
    blocks = [np.ascontiguousarray(synth.text(bsz, seed=70 + i)) for i in range(4)]
    want = _want_linked(orc, blocks, bsz, True)
    c0 = e.counters()
    recs = e.encode_records_ex(blocks, bsz, True, linked=True)
    assert [r.tobytes() for r in recs] == want
    free1, _ = torch.cuda.mem_get_info()
    small = [np.ascontiguousarray(synth.text(8192, seed=90 + i)) for i in range(200)]
    srec = e.encode_records_ex(small, 64 << 10, True, linked=True)
    assert [r.tobytes() for r in srec] == _want_linked(orc, small, 64 << 10, True)
    window = np.zeros(65536, dtype=np.uint8)
    res, st, outs, _ = e.decode_records_ex([np.ascontiguousarray(r) for r in recs], bsz, True, linked=True, window=window, window_len=0)
    assert not any(st) and all(np.array_equal(b, o) for b, o in zip(blocks, outs))
    again = e.encode_records_ex(blocks, bsz, True, linked=True)
    assert [r.tobytes() for r in again] == want
    c1 = e.counters()
    assert c1["fxl_blocks"] - c0["fxl_blocks"] == 8 and c1["fx_blocks"] - c0["fx_blocks"] == 8, (c0, c1)
    assert c1["dxl_blocks"] - c0["dxl_blocks"] == 4, (c0, c1)
    e.trim()
    e.close()
    torch.cuda.synchronize()
    free2, _ = torch.cuda.mem_get_info()
    assert free1 < free0                                                  # (the call held its workspaces)
    assert free2 >= free0 - (64 << 20), (free0 >> 20, free1 >> 20, free2 >> 20)


def test_gpu_fxl_host_layer_linked_frame(orc):
    """A linked frame of 3 blocks through the host layer (one block per engine call, the tail carried): the oracle's frame, and it
    reads back."""
    from plz4_amd import host
    e = host.hip_engine(0)
    bsz = 256 << 10
    payload = synth.make("M", 2 * bsz + 100000, 1 << 16, seed=55)
    blocks = [payload[o:o + bsz].copy() for o in range(0, payload.size, bsz)]
    w = host.Writer(e, parallel=1, block_size=host.BlockIdx256KB, block_linked=True, block_checksum=True)
    assert w.write(payload.tobytes())[1] == 0 and not w.close()
    frame = w.output()
    want = orc.frame_header(5, linked=True, block_checksum=True, content_checksum=True) + b"".join(_want_linked(orc, blocks, bsz, True))
    want += b"\0\0\0\0" + np.uint32(orc.xxh32(payload)).tobytes()
    assert frame == want
    n, out, err = host.Reader(e, frame).write_to()
    assert not err and out == payload.tobytes()
    e.close()
