"""The grid batch's scalar hop on the GPU (plz4_amd/csrc/lz4_seq_device.inl: a finished walk stays on its last match, eight unconditional
hops, one question for more hops and the 36-byte window): the crafted blocks of tests/hopcases.py (128 KiB each: a batch that
executes nothing while its lane 0 has a successor, walks from lane 0, 8 / 9 / 13 matches in a batch, more than eight with a lane
that fills its 20-byte window) and one 4 MiB block of the bench's text, through the routes and block counts of
tests/test_gpu_parse_window.py -- the one-wave parse (more blocks than the few-block path takes), the duplex kernel, the few-block
path with 1 and 16 blocks: every record is blk.CompressToBlk's, byte for byte."""
import numpy as np
import pytest

import hopcases
from plz4_amd import synth
from test_gpu_parse_window import BSZ, _dev_duplex, _dev_encode, _same, _want


@pytest.fixture(scope="module")
def eng():
    from plz4_amd._native import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def crafted():
    """19 seeds of every case: 133 blocks of one size, more than the few-block path takes."""
    return [hopcases.block(name, seed)[0] for seed in range(19) for name in hopcases.NAMES]


@pytest.fixture(scope="module")
def crafted_want(orc, crafted):
    return _want(orc, crafted, hopcases.N_BLOCK)


@pytest.mark.gpu
def test_gpu_hops_crafted_one_wave_parse_and_duplex(eng, crafted, crafted_want):
    bsz = hopcases.N_BLOCK
    assert bsz > 65547 and len(crafted) > 128
    c0 = eng.counters()
    _same(_dev_encode(eng, crafted, bsz), crafted_want)
    assert eng.counters()["fx_blocks"] == c0["fx_blocks"]
    _same(_dev_duplex(eng, crafted, bsz, crafted_want), crafted_want)


@pytest.mark.gpu
@pytest.mark.parametrize("nb", [1, 16])
def test_gpu_hops_crafted_few_blocks(eng, crafted, crafted_want, nb):
    bsz = hopcases.N_BLOCK
    k = len(hopcases.NAMES)
    for i in range(0, max(k, nb), nb):                       # every case at least once
        c0 = eng.counters()
        recs = eng.encode_records(crafted[i:i + nb], bsz, True)
        assert eng.counters()["fx_blocks"] - c0["fx_blocks"] == nb
        _same(recs, crafted_want[i:i + nb])


@pytest.mark.gpu
def test_gpu_hops_text_4mib(orc, eng):
    blk = np.ascontiguousarray(synth.make("T", BSZ, BSZ))
    want = _want(orc, [blk], BSZ)
    c0 = eng.counters()
    _same(_dev_encode(eng, [blk] * 129, BSZ), want * 129)   # the one-wave parse
    assert eng.counters()["fx_blocks"] == c0["fx_blocks"]
    _same(_dev_duplex(eng, [blk] * 3, BSZ, want * 3), want * 3)
    for nb in (1, 16):                                       # the few-block path
        c0 = eng.counters()
        recs = eng.encode_records([blk] * nb, BSZ, True)
        assert eng.counters()["fx_blocks"] - c0["fx_blocks"] == nb
        _same(recs, want * nb)
