"""The level-1 parser's candidate windows on the GPU (plz4_amd/csrc/lz4_seq_device.inl: candidate loads through a bounds-checked
buffer, only by the lanes that have a candidate; 16 bytes more for a hit that fills its 20-byte window): the crafted inputs of
tests/pwcases.py and 4 MiB text / mixed blocks through the one-wave parse (plz4hip_dev_encode_records, more blocks than the
few-block path takes), the duplex kernel (plz4hip_dev_duplex_records) and the few-block path (1 and 16 blocks, 64 KiB pieces):
every record is blk.CompressToBlk's, with LZ4_compress_fast's bytes in it."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import pwcases
from plz4_amd import synth

BSZ = 4 << 20


@pytest.fixture(scope="module")
def eng():
    from plz4_amd._native import Engine
    e = Engine(0)
    yield e
    e.close()


def _crafted_blocks(seeds):
    """One block per length and seed, all of one size."""
    blocks = [pwcases.block_for_length(L, seed)[0] for seed in seeds for L in pwcases.LENGTHS]
    assert len({b.size for b in blocks}) == 1
    return blocks


def _want(orc, blocks, bsz):
    with ThreadPoolExecutor(8) as ex:                                         # (the oracle releases the GIL inside ctypes calls)
        return list(ex.map(lambda b: orc.block_record(b, bsz, True), blocks))


def _dev_encode(eng, blocks, bsz):
    import torch
    dev = torch.device("cuda:0")
    nb = len(blocks)
    d_src = torch.from_numpy(np.concatenate(blocks)).to(dev)
    stride = eng.stage_stride(bsz)
    d_stage = torch.zeros(nb * stride, dtype=torch.uint8, device=dev)
    d_len = torch.zeros(nb, dtype=torch.int32, device=dev)
    eng.dev_encode_records(d_src.data_ptr(), d_src.numel(), bsz, True, d_stage.data_ptr(), d_len.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    lens = d_len.cpu().numpy(); stage = d_stage.cpu().numpy()
    return [stage[i * stride:i * stride + int(lens[i])] for i in range(nb)]


def _dev_duplex(eng, blocks, bsz, want):
    """Encodes `blocks` while it decodes their own records (the oracle's); returns the records, checks the decode."""
    import torch
    dev = torch.device("cuda:0")
    nb = len(blocks)
    src = np.concatenate(blocks)
    d_src = torch.from_numpy(src).to(dev)
    stride = eng.stage_stride(bsz)
    d_stage = torch.zeros(nb * stride, dtype=torch.uint8, device=dev)
    d_len = torch.zeros(nb, dtype=torch.int32, device=dev)
    off = np.zeros(nb + 1, dtype=np.int64); off[1:] = np.cumsum([w.size for w in want])
    d_body = torch.from_numpy(np.concatenate(want)).to(dev)
    d_off = torch.from_numpy(off).to(dev)
    d_out = torch.zeros(nb * bsz, dtype=torch.uint8, device=dev)
    d_res = torch.zeros(nb, dtype=torch.int32, device=dev)
    d_st = torch.full((nb,), -9, dtype=torch.int32, device=dev)
    eng.dev_duplex_records(d_src.data_ptr(), src.size, bsz, True, d_stage.data_ptr(), d_len.data_ptr(), d_body.data_ptr(), d_off.data_ptr(),
                           nb, bsz, True, d_out.data_ptr(), bsz, bsz, d_res.data_ptr(), d_st.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert int(d_st.abs().sum().item()) == 0 and int(d_res.to(torch.int64).sum().item()) == src.size
    assert np.array_equal(d_out[:src.size].cpu().numpy(), src)
    lens = d_len.cpu().numpy(); stage = d_stage.cpu().numpy()
    return [stage[i * stride:i * stride + int(lens[i])] for i in range(nb)]


def _same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.size == w.size and np.array_equal(g, w), i


@pytest.mark.gpu
def test_gpu_pw_crafted_one_wave_parse_and_duplex(orc, eng):
    blocks = _crafted_blocks(range(6))                   # 156 blocks: more than the few-block path takes
    bsz = blocks[0].size
    want = _want(orc, blocks, bsz)
    c0 = eng.counters()
    _same(_dev_encode(eng, blocks, bsz), want)
    assert eng.counters()["fx_blocks"] == c0["fx_blocks"]
    _same(_dev_duplex(eng, blocks, bsz, want), want)


@pytest.mark.gpu
@pytest.mark.parametrize("nb", [1, 16])
def test_gpu_pw_crafted_few_blocks(orc, ref, eng, nb):
    """Blocks of their own sizes through plz4hip_encode_records: the few-block path (pieces of 64 KiB), matches that end at
    matchLimit among them."""
    blocks = [pwcases.block_for_length(L, 7)[0] for L in pwcases.LENGTHS] + [pwcases.block_to_match_limit(L, 7)[0] for L in pwcases.LENGTHS]
    bsz = max(b.size for b in blocks)
    for i in range(0, len(blocks) - nb + 1, nb):
        grp = blocks[i:i + nb]
        c0 = eng.counters()
        recs = eng.encode_records(grp, bsz, True)
        assert eng.counters()["fx_blocks"] - c0["fx_blocks"] == nb
        _same(recs, [orc.block_record(b, bsz, True) for b in grp])
        for b, r in zip(grp, recs):
            n, comp = ref.compress_fast(b, bsz)
            assert n > 0 and np.array_equal(r[4:-4], comp[:n])


def _pool_4mib():
    m = synth.make("M", 3 * BSZ, BSZ)
    return [np.ascontiguousarray(synth.make("T", BSZ, BSZ)), np.ascontiguousarray(synth.text(BSZ, seed=77))] + \
           [np.ascontiguousarray(m[o:o + BSZ]) for o in range(0, m.size, BSZ)]


@pytest.mark.gpu
def test_gpu_pw_text_and_mixed_4mib(orc, ref, eng):
    pool = _pool_4mib()
    want = _want(orc, pool, BSZ)
    for b, w in zip(pool, want):
        n, comp = ref.compress_fast(b, BSZ)
        assert (n > 0 and np.array_equal(w[4:-4], comp[:n])) or (n == 0 and w.size == BSZ + 8)
    # the one-wave parse: 135 blocks in one call
    c0 = eng.counters()
    got = _dev_encode(eng, pool * 27, BSZ)
    assert eng.counters()["fx_blocks"] == c0["fx_blocks"]
    _same(got, want * 27)
    # the duplex kernel
    _same(_dev_duplex(eng, pool * 3, BSZ, want * 3), want * 3)
    # the few-block path: 1 and 16 blocks
    for grp, w in ((pool[:1], want[:1]), ((pool * 4)[:16], (want * 4)[:16])):
        c0 = eng.counters()
        recs = eng.encode_records(grp, BSZ, True)
        assert eng.counters()["fx_blocks"] - c0["fx_blocks"] == len(grp)
        _same(recs, w)


@pytest.mark.gpu
def test_gpu_pw_duplex_320_blocks(orc, eng):
    """k_l1_duplex at the size the bench runs it in kind: 320 x 4 MiB blocks each way, persistent waves taking several blocks each."""
    import torch
    bsz, nb = BSZ, 320
    pool = synth.make("T", 16 * bsz, bsz)
    pool[5 * bsz:6 * bsz] = synth.make("R", bsz, bsz)                       # one stored block per 16
    pool[9 * bsz:9 * bsz + (bsz >> 1)] = 0                                  # one with a 2 MiB run
    pool[12 * bsz:15 * bsz] = synth.make("M", 3 * bsz, bsz)
    d_pool = torch.from_numpy(pool).to(torch.device("cuda:0"))
    src = torch.cat([torch.roll(d_pool, -((r * 1000003) % pool.size)) if r else d_pool for r in range(nb // 16)]).cpu().numpy()
    blocks = [src[i * bsz:(i + 1) * bsz] for i in range(nb)]
    want = _want(orc, blocks, bsz)
    _same(_dev_duplex(eng, blocks, bsz, want), want)
