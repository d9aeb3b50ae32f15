"""The wave-wide HC parser for blocks of at most 4 KiB under a dictionary context (k_hcx of plz4hip.hip) through the C ABI and the
host layer: every block must be LZ4_compress_HC_continue's under the attached dictionary -- the real liblz4 streams -- byte for byte
and return value for return value, and hcx_blocks of plz4hip_ctx_counters must show that the parser encoded them.  The parser is
built for every HC level, 2..12 (hcx_cases.HCX_LEVELS); PLZ4HIP_HCX=0 keeps the one-thread parsers."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import hcdict
import hcx_cases as hc
from plz4_amd import synth

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def eng():
    from plz4_amd._native import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def cases(ref):
    return hc.all_cases(ref)


def _hcx(eng, c0):
    return eng.counters()["hcx_blocks"] - c0["hcx_blocks"]


@pytest.mark.parametrize("level", hc.HCX_LEVELS)
def test_gpu_hcx_case_list(ref, eng, cases, level):
    """The case list through plz4hip_compress_batch_dict: one call per dictionary with all of that dictionary's cases and
    capacities in the batch; the counter rises by exactly the number of blocks in the call."""
    groups = {}
    for case in cases:
        if level in hc.levels_of(case):
            groups.setdefault((case.dct.ctypes.data, case.dct.size), []).append(case)
    assert len(groups) >= len(hc.DICT_LENS)
    for grp in groups.values():
        dct = grp[0].dct
        keep, daddr = ref.new_dict_ctx_hc(hc.dict64(dct), level)
        comp = ref.stream_ctx_hc(level, daddr)
        srcs, caps, names = [], [], []
        for case in grp:
            for cap in hc.caps_of(case):
                srcs.append(case.block); caps.append(cap); names.append(case.name)
        d = eng.dict_create(np.ascontiguousarray(dct))
        c0 = eng.counters()
        res, outs = eng.compress_batch_dict(srcs, caps, d, level=level)
        assert _hcx(eng, c0) == len(srcs), (grp[0].name, level)
        eng.dict_destroy(d)
        for s, cap, name, r, o in zip(srcs, caps, names, res, outs):
            wr, wo = comp(s, cap)
            assert int(r) == wr and np.array_equal(o, wo), (name, level, cap, int(r), wr)


@pytest.mark.parametrize("ext_off", [False, True])
def test_gpu_hcx_mixed_sizes(ref, eng, monkeypatch, ext_off):
    """One level-9 call with blocks on both sides of the 4 KiB switch: the two small ones are the parser's -- behind the list path,
    and behind the one-thread kernels that PLZ4HIP_HC_EXT_OFF (read per call) keeps for the large ones."""
    if ext_off: monkeypatch.setenv("PLZ4HIP_HC_EXT_OFF", "1")
    else: monkeypatch.delenv("PLZ4HIP_HC_EXT_OFF", raising=False)
    data = hc.text_block(4096, 0)
    big = synth.text(70000, seed=78)
    srcs = [np.ascontiguousarray(data[:100]), data, np.ascontiguousarray(big[:4097]), big]
    caps = [hc.bound(s.size) for s in srcs]
    keep, daddr = ref.new_dict_ctx_hc(hc.dict64(hc.TEXT_DICT), 9)
    comp = ref.stream_ctx_hc(9, daddr)
    d = eng.dict_create(hc.TEXT_DICT)
    c0 = eng.counters()
    res, outs = eng.compress_batch_dict(srcs, caps, d, level=9)
    assert _hcx(eng, c0) == 2
    eng.dict_destroy(d)
    for s, cap, r, o in zip(srcs, caps, res, outs):
        wr, wo = comp(s, cap)
        assert int(r) == wr and np.array_equal(o, wo), s.size


@pytest.mark.parametrize("level", [2, 3, 12])
def test_gpu_hcx_many_small_blocks(ref, eng, level):
    """3000 blocks of 37..4096 bytes in one call: more blocks than resident waves, every one off the block queue."""
    rng = np.random.Generator(np.random.PCG64(4242))
    pool = synth.text(70000 + 400000, seed=77)[70000:]
    srcs = []
    for i in range(3000):
        n = int(rng.integers(37, 4097)); o = int(rng.integers(0, pool.size - n))
        srcs.append(np.ascontiguousarray(pool[o:o + n]))
    caps = [hc.bound(s.size) for s in srcs]
    keep, daddr = ref.new_dict_ctx_hc(hc.dict64(hc.TEXT_DICT), level)
    comp = ref.stream_ctx_hc(level, daddr)
    d = eng.dict_create(hc.TEXT_DICT)
    c0 = eng.counters()
    res, outs = eng.compress_batch_dict(srcs, caps, d, level=level)
    assert _hcx(eng, c0) == len(srcs)
    eng.dict_destroy(d)
    for i, (s, cap, r, o) in enumerate(zip(srcs, caps, res, outs)):
        wr, wo = comp(s, cap)
        assert int(r) == wr and np.array_equal(o, wo), (i, s.size)


def _blocks_4k():
    whole = np.concatenate([hc.text_block(4096, 0), hc.text_block(4096, 1), synth.random_bytes(4096, seed=3), hc.text_block(1234, 2)])
    return [np.ascontiguousarray(whole[o:o + 4096]) for o in range(0, whole.size, 4096)]


@pytest.mark.parametrize("cs", [True, False])
def test_gpu_hcx_records(ref, orc, eng, cs):
    """Record form with bsz = 4096: independent blocks under the dictionary (a stored record among them), and a linked frame whose
    only block is block 0."""
    blocks = _blocks_4k()
    d = eng.dict_create(hc.TEXT_DICT)
    for level in (2, 3, 9, 11):
        want, rets = hcdict.ref_records(ref, orc, blocks, 4096, level, False, hc.TEXT_DICT, checksum=cs)
        assert 0 in rets                                                 # (the noise block is stored)
        c0 = eng.counters()
        got = eng.encode_records_ex(blocks, 4096, cs, linked=False, d=d, level=level)
        assert _hcx(eng, c0) == len(blocks)
        assert [g.tobytes() for g in got] == want, level
        for blk in (blocks[0], blocks[3]):
            want, _ = hcdict.ref_records(ref, orc, [blk], 4096, level, True, hc.TEXT_DICT, checksum=cs)
            c0 = eng.counters()
            got = eng.encode_records_ex([blk], 4096, cs, linked=True, d=d, level=level)
            assert _hcx(eng, c0) == 1
            assert [g.tobytes() for g in got] == want, (level, blk.size)
    eng.dict_destroy(d)


def test_gpu_hcx_dev_records_gapped(ref, orc, eng):
    """plz4hip_dev_encode_records_ex on the gapped stride (64 KiB of scratch in front of every block) with bsz = 4096."""
    import torch
    dev = torch.device("cuda:0")
    blocks = _blocks_4k()
    plain = np.concatenate(blocks)
    d = eng.dict_create(hc.TEXT_DICT)
    nb, bsz, pad = len(blocks), 4096, 65536
    stride = bsz + 65536
    host = np.full(pad + nb * stride + 256, 0xA7, np.uint8)
    for i, b in enumerate(blocks):
        host[pad + i * stride:pad + i * stride + b.size] = b
    d_src = torch.from_numpy(host).to(dev)
    sstride = eng.stage_stride(bsz)
    for level in (2, 3, 9, 12):
        want, _ = hcdict.ref_records(ref, orc, blocks, bsz, level, False, hc.TEXT_DICT, checksum=True)
        d_stage = torch.zeros(nb * sstride + 64, dtype=torch.uint8, device=dev)
        d_len = torch.full((nb,), -7, dtype=torch.int32, device=dev)
        c0 = eng.counters()
        eng.dev_encode_records_ex(d_src.data_ptr() + pad, plain.size, stride, bsz, True, d_stage.data_ptr(), d_len.data_ptr(), linked=False, d=d,
                                  stream=torch.cuda.current_stream().cuda_stream, level=level)
        torch.cuda.synchronize()
        assert _hcx(eng, c0) == nb
        rl, st = d_len.cpu().numpy(), d_stage.cpu().numpy()
        recs = [st[i * sstride:i * sstride + int(rl[i])].tobytes() for i in range(nb)]
        assert recs == want and [int(x) for x in rl] == [len(w) for w in want], level
    assert np.array_equal(d_src.cpu().numpy()[pad:pad + plain.size - 0][:4096], host[pad:pad + 4096])     # (block 0 as it was)
    eng.dict_destroy(d)


def test_gpu_hcx_host_layer(ref, orc):
    """Writer(level=9, dictionary) over a payload of one short block and over 64 KiB + 2000 bytes (a short last block): the Reader
    gives the payload back and the frame holds the real liblz4's records."""
    from plz4_amd import host
    e = host.hip_engine(0)
    user = hc.TEXT_DICT.tobytes()
    pool = synth.text(70000 + 70000, seed=77)[70000:]
    for n in (3000, (64 << 10) + 2000):
        payload = np.ascontiguousarray(pool[:n])
        w = host.Writer(e, parallel=2, level=9, block_size=host.BlockIdx64KB, block_checksum=True, block_linked=False, dictionary=user)
        assert w.write(payload.tobytes())[1] == 0 and not w.close()
        frame = w.output()
        blocks = [np.ascontiguousarray(payload[o:o + (64 << 10)]) for o in range(0, n, 64 << 10)]
        want, _ = hcdict.ref_records(ref, orc, blocks, 64 << 10, 9, False, hc.TEXT_DICT, checksum=True)
        assert b"".join(want) in frame, n
        k, out, err = host.Reader(e, frame, dictionary=user).write_to()
        assert not err and out == payload.tobytes()
    e.close()


_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import hcx_cases as hc
from plz4_amd._native import Engine
e = Engine(0)
d = e.dict_create(hc.TEXT_DICT)
srcs = [hc.text_block(n, k) for k, n in enumerate((100, 4096, 1000))]
out = {}
for level in (2, 3, 9, 10):
    c0 = e.counters()
    res, outs = e.compress_batch_dict(srcs, [hc.bound(s.size) for s in srcs], d, level=level)
    out[str(level)] = {"res": [int(r) for r in res], "hex": [o.tobytes().hex() for o in outs], "hcx": e.counters()["hcx_blocks"] - c0["hcx_blocks"]}
e.dict_destroy(d); e.close()
print(json.dumps(out))
"""


def test_gpu_hcx_switch_off():
    """PLZ4HIP_HCX=0 (a fresh process): the one-thread parsers, the same bytes, the counter does not move."""
    got = {}
    for off in (False, True):
        env = dict(os.environ)
        env.pop("PLZ4HIP_HCX", None)
        if off: env["PLZ4HIP_HCX"] = "0"
        r = subprocess.run([sys.executable, "-c", _CHILD % (os.path.dirname(HERE), HERE)], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        got[off] = json.loads(r.stdout.strip().splitlines()[-1])
    for level in ("2", "3", "9", "10"):
        assert got[False][level]["hcx"] == 3 and got[True][level]["hcx"] == 0
        assert got[False][level]["res"] == got[True][level]["res"] and got[False][level]["hex"] == got[True][level]["hex"]
        assert all(r > 0 for r in got[False][level]["res"])


def test_gpu_hcx_one_ctx_mixed_calls(ref, orc):
    """Few-block decode, small-block HC + dictionary encode, trim, both again, close: on one ctx."""
    from plz4_amd._native import Engine
    e = Engine(0)
    bsz = 256 << 10
    data = synth.make("T", 2 * bsz, bsz, seed=3)
    big = [np.ascontiguousarray(data[o:o + bsz]) for o in range(0, data.size, bsz)]
    recs = [np.ascontiguousarray(r) for r in e.encode_records(big, bsz, True)]
    srcs = [hc.text_block(n, k) for k, n in enumerate((4096, 777, 13))]
    caps = [hc.bound(s.size) for s in srcs]
    keep, daddr = ref.new_dict_ctx_hc(hc.dict64(hc.TEXT_DICT), 6)
    comp = ref.stream_ctx_hc(6, daddr)
    d = e.dict_create(hc.TEXT_DICT)
    for rnd in range(2):
        c0 = e.counters()
        res, st, outs = e.decode_records(recs, bsz, True)
        assert not any(st) and all(np.array_equal(o, b) for o, b in zip(outs, big))
        res, outs = e.compress_batch_dict(srcs, caps, d, level=6)
        c1 = e.counters()
        assert c1["hcx_blocks"] - c0["hcx_blocks"] == len(srcs) and c1["dx_blocks"] - c0["dx_blocks"] == len(big)
        for s, cap, r, o in zip(srcs, caps, res, outs):
            wr, wo = comp(s, cap)
            assert int(r) == wr and np.array_equal(o, wo), (rnd, s.size)
        e.trim()
    e.dict_destroy(d)
    e.close()


def test_gpu_hcx_dictionary_footprint(eng):
    """50 create / destroy pairs: free device memory does not end lower than after the first pair by more than one dictionary's
    footprint (the drop the first create caused)."""
    import torch
    torch.cuda.synchronize()
    f0 = torch.cuda.mem_get_info()[0]
    d = eng.dict_create(hc.TEXT_DICT)
    footprint = f0 - torch.cuda.mem_get_info()[0]
    eng.dict_destroy(d)
    after_first = torch.cuda.mem_get_info()[0]
    for _ in range(49):
        eng.dict_destroy(eng.dict_create(hc.TEXT_DICT))
    assert footprint >= 0
    assert after_first - torch.cuda.mem_get_info()[0] <= max(footprint, 0)
