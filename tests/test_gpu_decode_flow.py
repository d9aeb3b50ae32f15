"""The crafted blocks of tests/decflow_cases.py on the device: as records through the bulk record decoder (k_decode_rec) and
through the decode side of a duplex call (k_l1_duplex), and as raw blocks through the raw decode entry.  19 seeds of every case
are well over 128 records, so the bulk kernels and not the few-block path take them.  Plaintext equal to the generator's,
statuses OK, and one damaged record per call reported as the oracle reports it."""
import numpy as np
import pytest

import decflow_cases
from plz4_amd import synth

BSZ = 64 << 10
NAMES = decflow_cases.NAMES
OK, CORRUPT = 0, 3


@pytest.fixture(scope="module")
def eng():
    from plz4_amd._native import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def blocks():
    out = [decflow_cases.block(name, seed) for seed in range(decflow_cases.SEEDS_GPU) for name in decflow_cases.NAMES]
    assert len(out) > 128 and all(p.size <= BSZ for _, p in out)
    assert np.array_equal(out[0][0], decflow_cases.block(NAMES[0], 0)[0])
    return out


def _damaged(i, comp):
    """block i of the fixture (seed-major, NAMES inside a seed), its HEAD match pointing before the output"""
    return decflow_cases.damaged(NAMES[i % len(NAMES)], comp)


def _records(blocks, bad):
    recs = []
    for i, (c, _) in enumerate(blocks):
        c = _damaged(i, c) if i == bad else c
        recs.append(np.concatenate([np.frombuffer(np.uint32(c.size).tobytes(), dtype=np.uint8), c]))
    return recs


def _check(orc, blocks, bad, res, st, out):
    for i, (c, p) in enumerate(blocks):
        if i == bad:
            want, _ = orc.decompress_safe(_damaged(i, c), BSZ)
            assert want < 0 and int(st[i]) == CORRUPT and int(res[i]) == want, (i, int(st[i]), int(res[i]), want)
        else:
            assert int(st[i]) == OK and int(res[i]) == p.size, (i, int(st[i]), int(res[i]), p.size)
            assert np.array_equal(out[i * BSZ:i * BSZ + p.size], p), i


def _device_args(blocks, bad):
    import torch
    dev = torch.device("cuda:0")
    recs = _records(blocks, bad)
    nb = len(recs)
    off = np.zeros(nb + 1, dtype=np.int64); off[1:] = np.cumsum([r.size for r in recs])
    d_body = torch.from_numpy(np.concatenate(recs)).to(dev)
    d_off = torch.from_numpy(off).to(dev)
    d_out = torch.zeros(nb * BSZ, dtype=torch.uint8, device=dev)
    d_res = torch.zeros(nb, dtype=torch.int32, device=dev)
    d_st = torch.full((nb,), -9, dtype=torch.int32, device=dev)
    return nb, d_body, d_off, d_out, d_res, d_st


@pytest.mark.gpu
def test_gpu_decode_flow_records(orc, eng, blocks):
    import torch
    bad = 7
    nb, d_body, d_off, d_out, d_res, d_st = _device_args(blocks, bad)
    c0 = eng.counters()
    eng.dev_decode_records(d_body.data_ptr(), d_off.data_ptr(), nb, BSZ, False, d_out.data_ptr(), BSZ, BSZ, d_res.data_ptr(), d_st.data_ptr(),
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert eng.counters()["dx_blocks"] == c0["dx_blocks"]             # (the bulk kernel took them)
    _check(orc, blocks, bad, d_res.cpu().numpy(), d_st.cpu().numpy(), d_out.cpu().numpy())


@pytest.mark.gpu
def test_gpu_decode_flow_duplex(orc, eng, blocks):
    """The same records on the decode side of a duplex call whose encode side parses as many 64 KiB text blocks."""
    import torch
    dev = torch.device("cuda:0")
    bad = 11
    nb, d_body, d_off, d_out, d_res, d_st = _device_args(blocks, bad)
    src = np.ascontiguousarray(synth.make("T", nb * BSZ, BSZ)[:nb * BSZ])
    d_src = torch.from_numpy(src).to(dev)
    stride = eng.stage_stride(BSZ)
    d_stage = torch.zeros(nb * stride, dtype=torch.uint8, device=dev)
    d_len = torch.zeros(nb, dtype=torch.int32, device=dev)
    eng.dev_duplex_records(d_src.data_ptr(), src.size, BSZ, True, d_stage.data_ptr(), d_len.data_ptr(), d_body.data_ptr(), d_off.data_ptr(),
                           nb, BSZ, False, d_out.data_ptr(), BSZ, BSZ, d_res.data_ptr(), d_st.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _check(orc, blocks, bad, d_res.cpu().numpy(), d_st.cpu().numpy(), d_out.cpu().numpy())
    lens = d_len.cpu().numpy(); stage = d_stage.cpu().numpy()
    for i in (0, nb // 2, nb - 1):                                     # (the encode side's records are the oracle's)
        assert np.array_equal(stage[i * stride:i * stride + int(lens[i])], orc.block_record(src[i * BSZ:(i + 1) * BSZ], BSZ, True)), i


@pytest.mark.gpu
def test_gpu_decode_flow_raw(orc, eng, blocks):
    bad = 3
    srcs = [_damaged(i, c) if i == bad else c for i, (c, _) in enumerate(blocks)]
    for spare in (0, 100):
        res, outs = eng.decompress_batch(srcs, [p.size + spare for _, p in blocks])
        for i, ((c, p), r, o) in enumerate(zip(blocks, res, outs)):
            if i == bad:
                want, _ = orc.decompress_safe(srcs[i], p.size + spare)
                assert want < 0 and int(r) == want, (i, int(r), want)
            else:
                assert int(r) == p.size and np.array_equal(o[:p.size], p), (i, int(r), p.size)
