"""The crafted blocks of tests/decsteps_cases.py and its random blocks on the device, in 64 KiB slots: as records through the bulk
record decoder (k_decode_rec), through the decode side of a duplex call (k_l1_duplex) and through the dictionary record decoder
(k_decode_rec_dict, the other kernel that runs wave_decode_block<true>); and the bench's 4 MiB T block through the first two.  Ten
seeds of every case and 300 random blocks are well over 128 records, so the bulk kernels and not the few-block path take them.
Plaintext equal to the generator's, statuses OK, sizes right."""
import numpy as np
import pytest

import decsteps_cases
from plz4_amd import synth

BSZ = 64 << 10
BIG = 4 << 20
N_BIG = 132
OK = 0


@pytest.fixture(scope="module")
def eng():
    from plz4_amd._native import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def blocks():
    out = [decsteps_cases.block(name, seed) for seed in range(decsteps_cases.SEEDS_GPU) for name in decsteps_cases.NAMES]
    out += [decsteps_cases.random_block(i) for i in range(decsteps_cases.N_RANDOM)]
    assert len(out) > 128 and all(p.size <= BSZ for _, p in out)
    return out


@pytest.fixture(scope="module")
def args(blocks):
    """the records on the device, shared by the three calls (read only), and the plaintext laid out in the output's slots"""
    import torch
    dev = torch.device("cuda:0")
    recs = [np.concatenate([np.frombuffer(np.uint32(c.size).tobytes(), dtype=np.uint8), c]) for c, _ in blocks]
    nb = len(recs)
    off = np.zeros(nb + 1, dtype=np.int64); off[1:] = np.cumsum([r.size for r in recs])
    want = np.zeros(nb * BSZ, dtype=np.uint8)
    for i, (_, p) in enumerate(blocks):
        want[i * BSZ:i * BSZ + p.size] = p
    sizes = np.array([p.size for _, p in blocks], dtype=np.int32)
    return nb, torch.from_numpy(np.concatenate(recs)).to(dev), torch.from_numpy(off).to(dev), want, sizes


def _outputs(nb, stride):
    import torch
    dev = torch.device("cuda:0")
    return (torch.zeros(nb * stride, dtype=torch.uint8, device=dev), torch.zeros(nb, dtype=torch.int32, device=dev),
            torch.full((nb,), -9, dtype=torch.int32, device=dev))


def _check(want, sizes, d_out, d_res, d_st):
    st = d_st.cpu().numpy(); res = d_res.cpu().numpy()
    assert np.array_equal(st, np.full(st.size, OK, dtype=np.int32)), np.flatnonzero(st != OK)[:8]
    assert np.array_equal(res, sizes), np.flatnonzero(res != sizes)[:8]
    out = d_out.cpu().numpy().reshape(-1, BSZ)
    inside = np.arange(BSZ)[None, :] < sizes[:, None]                  # (what lies behind a block's end in its slot is not compared)
    bad = np.argwhere((out != want.reshape(-1, BSZ)) & inside)
    assert bad.size == 0, "block %d, byte %d; %d bytes differ" % (bad[0][0], bad[0][1], len(bad))


@pytest.mark.gpu
def test_gpu_decode_steps_records(eng, args):
    import torch
    nb, d_body, d_off, want, sizes = args
    d_out, d_res, d_st = _outputs(nb, BSZ)
    c0 = eng.counters()
    eng.dev_decode_records(d_body.data_ptr(), d_off.data_ptr(), nb, BSZ, False, d_out.data_ptr(), BSZ, BSZ, d_res.data_ptr(), d_st.data_ptr(),
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert eng.counters()["dx_blocks"] == c0["dx_blocks"]             # (the bulk kernel took them)
    _check(want, sizes, d_out, d_res, d_st)


def _encode_side(eng, nb):
    """as many 64 KiB text blocks for the encode side of a duplex call"""
    import torch
    dev = torch.device("cuda:0")
    src = np.ascontiguousarray(synth.make("T", nb * BSZ, BSZ)[:nb * BSZ])
    stride = eng.stage_stride(BSZ)
    return (src, torch.from_numpy(src).to(dev), stride, torch.zeros(nb * stride, dtype=torch.uint8, device=dev),
            torch.zeros(nb, dtype=torch.int32, device=dev))


@pytest.mark.gpu
def test_gpu_decode_steps_duplex(orc, eng, args):
    import torch
    nb, d_body, d_off, want, sizes = args
    d_out, d_res, d_st = _outputs(nb, BSZ)
    src, d_src, stride, d_stage, d_len = _encode_side(eng, nb)
    eng.dev_duplex_records(d_src.data_ptr(), src.size, BSZ, True, d_stage.data_ptr(), d_len.data_ptr(), d_body.data_ptr(), d_off.data_ptr(),
                           nb, BSZ, False, d_out.data_ptr(), BSZ, BSZ, d_res.data_ptr(), d_st.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _check(want, sizes, d_out, d_res, d_st)
    lens = d_len.cpu().numpy(); stage = d_stage.cpu().numpy()
    for i in (0, nb - 1):                                              # (the encode side's records are the oracle's)
        assert np.array_equal(stage[i * stride:i * stride + int(lens[i])], orc.block_record(src[i * BSZ:(i + 1) * BSZ], BSZ, True)), i


@pytest.mark.gpu
def test_gpu_decode_steps_dict(eng, args):
    """The same records under a dictionary none of them reaches into: k_decode_rec_dict runs the same LDS-staged batch."""
    import torch
    nb, d_body, d_off, want, sizes = args
    d_out, d_res, d_st = _outputs(nb, BSZ)
    d = eng.dict_create(np.random.default_rng(5).integers(0, 256, 4096, dtype=np.uint8))
    try:
        eng.dev_decode_records_ex(d_body.data_ptr(), d_off.data_ptr(), nb, BSZ, False, d_out.data_ptr(), BSZ, BSZ, d_res.data_ptr(), d_st.data_ptr(),
                                  linked=False, d=d, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        eng.dict_destroy(d)
    _check(want, sizes, d_out, d_res, d_st)


@pytest.mark.gpu
def test_gpu_decode_steps_text_4mib(orc, eng):
    """132 copies of the bench's 4 MiB T block's record (more than the few-block path takes) through k_decode_rec and through
    the decode side of a duplex call: 3.7 near steps per batch with members, every run length there is on text."""
    import torch
    dev = torch.device("cuda:0")
    src = np.ascontiguousarray(synth.make("T", BIG, BIG)[:BIG])
    rec = orc.block_record(src, BIG, True)
    d_src1 = torch.from_numpy(src).to(dev)
    d_body = torch.from_numpy(rec).to(dev).repeat(N_BIG)
    d_off = torch.arange(N_BIG + 1, dtype=torch.int64, device=dev) * rec.size
    stream = torch.cuda.current_stream().cuda_stream

    def check(d_out, d_res, d_st):
        assert int((d_st != OK).sum().item()) == 0 and int((d_res != BIG).sum().item()) == 0
        bad = (d_out.view(N_BIG, BIG) != d_src1).any(dim=1)
        assert int(bad.sum().item()) == 0, bad.nonzero()[:8].cpu().numpy()

    d_out, d_res, d_st = _outputs(N_BIG, BIG)
    c0 = eng.counters()
    eng.dev_decode_records(d_body.data_ptr(), d_off.data_ptr(), N_BIG, BIG, True, d_out.data_ptr(), BIG, BIG, d_res.data_ptr(), d_st.data_ptr(), stream)
    torch.cuda.synchronize()
    assert eng.counters()["dx_blocks"] == c0["dx_blocks"]
    check(d_out, d_res, d_st)

    d_out, d_res, d_st = _outputs(N_BIG, BIG)
    esrc, d_esrc, stride, d_stage, d_len = _encode_side(eng, N_BIG)
    eng.dev_duplex_records(d_esrc.data_ptr(), esrc.size, BSZ, True, d_stage.data_ptr(), d_len.data_ptr(), d_body.data_ptr(), d_off.data_ptr(),
                           N_BIG, BIG, True, d_out.data_ptr(), BIG, BIG, d_res.data_ptr(), d_st.data_ptr(), stream)
    torch.cuda.synchronize()
    check(d_out, d_res, d_st)
