"""The few-block level-1 path on the GPU (plz4_amd/csrc/lz4_fx_device.inl, launch_l1): calls of a handful of 4 MiB blocks have
their parse cut across the chip, and every entry point that takes it must give LZ4_compress_fast's bytes / blk.CompressToBlk's
records, exactly as the one-wave parse does.  plz4hip_ctx_counters shows that the path ran."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from plz4_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BSZ = 4 << 20
KINDS = ("T", "M", "Z", "R")


def _srcs(nb, seed=0):
    return [np.ascontiguousarray(synth.make(KINDS[i % 4], BSZ, 1 << 16, seed=seed + 11 * i)) for i in range(nb)]


@pytest.fixture(scope="module")
def eng():
    from plz4_amd._native import Engine
    e = Engine(0)
    yield e
    e.close()


def _delta(eng, before):
    after = eng.counters()
    return {k: after[k] - before[k] for k in ("fx_blocks", "fx_pieces_again", "dx_blocks")} | {"rounds": after["fx_rounds_last"]}


@pytest.mark.gpu
@pytest.mark.parametrize("nb", [1, 3, 16])
def test_gpu_fx_compress_batch(orc, eng, nb):
    srcs = _srcs(nb, seed=nb)
    bound = orc.bound(BSZ)
    for caps in ([bound] * nb, [BSZ] * nb):
        c0 = eng.counters()
        res, outs = eng.compress_batch(srcs, caps)
        d = _delta(eng, c0)
        assert d["fx_blocks"] == nb and d["rounds"] >= 1, d
        for s, cap, r, o in zip(srcs, caps, res, outs):
            want, comp = orc.compress_fast(s, cap)
            assert int(r) == want and np.array_equal(o, comp[:want]), (nb, cap)


@pytest.mark.gpu
@pytest.mark.parametrize("cs", [False, True])
def test_gpu_fx_encode_records(orc, eng, cs):
    for nb in (1, 3, 16):
        srcs = _srcs(nb, seed=100 + nb)
        c0 = eng.counters()
        recs = eng.encode_records(srcs, BSZ, cs)
        assert _delta(eng, c0)["fx_blocks"] == nb
        for s, r in zip(srcs, recs):
            assert np.array_equal(r, orc.block_record(s, BSZ, cs)), (nb, cs)


@pytest.mark.gpu
def test_gpu_fx_device_resident_calls(orc, eng):
    """plz4hip_dev_compress (raw blocks, lengths on the device) and plz4hip_dev_encode_body (records back to back)."""
    import torch
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    for nb in (1, 3, 16):
        srcs = _srcs(nb, seed=200 + nb)
        data = np.concatenate(srcs)
        bound = orc.bound(BSZ)
        stride = BSZ + 64
        d_src = torch.zeros(nb * stride, dtype=torch.uint8, device=dev)
        for i, x in enumerate(srcs):
            d_src[i * stride:i * stride + BSZ] = torch.from_numpy(x).to(dev)
        d_len = torch.full((nb,), BSZ, dtype=torch.int32, device=dev)
        d_cap = torch.full((nb,), bound, dtype=torch.int32, device=dev)
        d_dst = torch.zeros(nb * (bound + 64), dtype=torch.uint8, device=dev)
        d_res = torch.zeros(nb, dtype=torch.int32, device=dev)
        c0 = eng.counters()
        eng._chk(eng.L.plz4hip_dev_compress(eng.h, nb, d_src.data_ptr(), stride, d_len.data_ptr(), d_dst.data_ptr(), bound + 64,
                                            d_cap.data_ptr(), 1, BSZ, d_res.data_ptr(), s))
        torch.cuda.synchronize()
        assert _delta(eng, c0)["fx_blocks"] == nb
        res = d_res.cpu().numpy(); out = d_dst.cpu().numpy()
        for i, x in enumerate(srcs):
            want, comp = orc.compress_fast(x, bound)
            assert int(res[i]) == want and np.array_equal(out[i * (bound + 64):i * (bound + 64) + want], comp[:want]), (nb, i)

        for cs in (False, True):
            want_body = np.concatenate([orc.block_record(x, BSZ, cs) for x in srcs])
            d_in = torch.from_numpy(data).to(dev)
            d_body = torch.zeros(want_body.size + 100, dtype=torch.uint8, device=dev)
            d_off = torch.full((nb + 1,), -1, dtype=torch.int64, device=dev)
            d_rl = torch.zeros(nb, dtype=torch.int32, device=dev)
            c0 = eng.counters()
            eng.dev_encode_body(d_in.data_ptr(), data.size, BSZ, cs, d_body.data_ptr(), d_body.numel(), d_off.data_ptr(), d_rl.data_ptr(), s)
            torch.cuda.synchronize()
            assert _delta(eng, c0)["fx_blocks"] == nb
            assert int(d_off[-1].item()) == want_body.size
            assert np.array_equal(d_body[:want_body.size].cpu().numpy(), want_body), (nb, cs)


@pytest.mark.gpu
def test_gpu_fx_many_rounds(orc, eng, monkeypatch):
    """Small pieces started with no warm-up: many rounds, pieces parsed again -- and still the same bytes."""
    monkeypatch.setenv("PLZ4HIP_FX_PIECE_KIB", "4")
    monkeypatch.setenv("PLZ4HIP_FX_WARMUP_KIB", "0")
    srcs = _srcs(3, seed=300) + [np.ascontiguousarray(synth.text(BSZ - 12345, seed=9))]
    c0 = eng.counters()
    res, outs = eng.compress_batch(srcs, [orc.bound(BSZ)] * 4)
    d = _delta(eng, c0)
    assert d["fx_blocks"] == 4 and d["rounds"] > 1 and d["fx_pieces_again"] > 0, d
    for s, r, o in zip(srcs, res, outs):
        want, comp = orc.compress_fast(s, orc.bound(BSZ))
        assert int(r) == want and np.array_equal(o, comp[:want])


_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from plz4_amd import synth
from plz4_amd._native import Engine
e = Engine(0)
srcs = [np.ascontiguousarray(synth.make(k, 4 << 20, 1 << 16, seed=400 + i)) for i, k in enumerate("TMZR")]
res, outs = e.compress_batch(srcs, [(4 << 20) + (4 << 20) // 255 + 16] * 4)
recs = e.encode_records(srcs, 4 << 20, True)
np.save(sys.argv[2], np.concatenate(outs + recs))
print(json.dumps({"res": [int(r) for r in res], "counters": e.counters()}))
e.close()
"""


@pytest.mark.gpu
def test_gpu_fx_off_gives_the_same_bytes(eng, tmp_path):
    """PLZ4HIP_FX_MAX_BLOCKS=0 (in a child process): the one-wave parse, the same bytes as the few-block path."""
    srcs = [np.ascontiguousarray(synth.make(k, BSZ, 1 << 16, seed=400 + i)) for i, k in enumerate("TMZR")]
    bound = BSZ + BSZ // 255 + 16
    res, outs = eng.compress_batch(srcs, [bound] * 4)
    recs = eng.encode_records(srcs, BSZ, True)
    mine = np.concatenate(outs + recs)
    env = dict(os.environ, PLZ4HIP_FX_MAX_BLOCKS="0")
    out = str(tmp_path / "off.npy")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, out], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got["counters"]["fx_blocks"] == 0
    assert got["res"] == [int(r) for r in res]
    assert np.array_equal(np.load(out), mine)


@pytest.mark.gpu
def test_gpu_fx_workspace_is_given_back(orc):
    """One ctx: a few-block encode, a bulk encode, a few-block decode, a few-block encode again; trim and destroy give the device
    memory back."""
    import torch
    from plz4_amd._native import Engine
    torch.cuda.init()
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    e = Engine(0)
    srcs = _srcs(4, seed=500)
    bound = orc.bound(BSZ)
    c0 = e.counters()
    res, outs = e.compress_batch(srcs, [bound] * 4)
    assert all(int(r) == orc.compress_fast(s, bound)[0] for s, r in zip(srcs, res))
    free1, _ = torch.cuda.mem_get_info()
    small = [np.ascontiguousarray(synth.text(60000, seed=600 + i)) for i in range(300)]      # the bulk path (many byU16 blocks)
    rs, _ = e.compress_batch(small, [orc.bound(60000)] * 300)
    assert all(int(r) == orc.compress_fast(s, orc.bound(60000))[0] for s, r in zip(small, rs))
    comps = [o.copy() for o in outs]
    rd, dec = e.decompress_batch(comps, [BSZ] * 4)
    assert all(int(r) == BSZ and np.array_equal(d, s) for r, d, s in zip(rd, dec, srcs))
    res2, outs2 = e.compress_batch(srcs, [bound] * 4)
    assert all(np.array_equal(a, b) for a, b in zip(outs, outs2))
    d = e.counters()
    assert d["fx_blocks"] - c0["fx_blocks"] == 8 and d["dx_blocks"] - c0["dx_blocks"] == 4, d
    e.trim()
    e.close()
    torch.cuda.synchronize()
    free2, _ = torch.cuda.mem_get_info()
    assert free1 < free0                                                  # (the call held its workspaces)
    assert free2 >= free0 - (64 << 20), (free0 >> 20, free1 >> 20, free2 >> 20)
