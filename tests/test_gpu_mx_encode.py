"""The few-block level-2 path on the GPU (plz4_amd/csrc/lz4_mx_device.inl behind launch_l1): calls of a handful of independent
blocks at level 2 have their LZ4MID walk cut across the chip, and every entry point that takes it must give LZ4_compress_HC(2)'s
bytes / blk.CompressToBlk's records of the real liblz4, exactly as the one-wave walk does.  Every case checks by the mx_blocks
delta of plz4hip_ctx_counters that the path took exactly the blocks it should: a silent fallback fails the test."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from plz4_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
N = 200 * 1024 + 13
K256 = 256 << 10
BSZ = 4 << 20


def _bound(n):
    return n + n // 255 + 16


def _small_env(mp, piece="8", warm="16"):
    mp.setenv("PLZ4HIP_MX_PIECE_KIB", piece)
    mp.setenv("PLZ4HIP_MX_WARMUP_KIB", warm)


@pytest.fixture(scope="module")
def eng():
    from plz4_amd._native import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def blocks():
    """Three blocks of 200 KiB + 13 (text, mixed, structured text with zeros) -- computed once, never written to."""
    out = [np.ascontiguousarray(synth.text(N, seed=31)), np.ascontiguousarray(synth.make("M", N, 1 << 14, seed=32)),
           np.ascontiguousarray(np.concatenate([synth.text(N // 2, seed=33), np.zeros(N - N // 2, dtype=np.uint8)]))]
    for b in out:
        b.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def body_data():
    """256 KiB blocks back to back: text, random (comes back stored), text of 200 KiB + 13."""
    d = np.ascontiguousarray(np.concatenate([synth.text(K256, seed=41), synth.random_bytes(K256, seed=42), synth.text(N, seed=43)]))
    d.setflags(write=False)
    return d


def _mx(eng, c0):
    c1 = eng.counters()
    return {"blocks": c1["mx_blocks"] - c0["mx_blocks"], "again": c1["mx_pieces_again"] - c0["mx_pieces_again"], "rounds": c1["mx_rounds_last"]}


def _record(ref, orc, src, bsz, cs):
    c, comp = ref.compress_hc(src, bsz, 2)
    payload, word = (src, 0x80000000 | src.size) if c == 0 else (comp[:c], c)
    rec = np.uint32(word).tobytes() + payload.tobytes()
    if cs:
        rec += np.uint32(orc.xxh32(np.ascontiguousarray(payload))).tobytes()
    return rec


def _cut(data, bsz):
    return [np.ascontiguousarray(data[o:o + bsz]) for o in range(0, data.size, bsz)]


@pytest.mark.parametrize("nb", [1, 3])
def test_gpu_mx_compress_batch(ref, eng, blocks, monkeypatch, nb):
    """26 pieces of 8 KiB per block, guessed starts 16 KiB early."""
    _small_env(monkeypatch)
    srcs = blocks[:nb]
    for caps in ([_bound(N)] * nb, [N] * nb):
        c0 = eng.counters()
        res, outs = eng.compress_batch(srcs, caps, level=2)
        d = _mx(eng, c0)
        assert d["blocks"] == nb and d["rounds"] >= 1, d
        for s, cap, r, o in zip(srcs, caps, res, outs):
            want, comp = ref.compress_hc(s, cap, 2)
            assert int(r) == want and np.array_equal(o, comp[:want]), (nb, cap)


def test_gpu_mx_one_4mib_block_at_the_defaults(ref, eng):
    src = np.ascontiguousarray(synth.text(BSZ, seed=7))
    c0 = eng.counters()
    res, outs = eng.compress_batch([src], [_bound(BSZ)], level=2)
    d = _mx(eng, c0)
    assert d["blocks"] == 1 and 1 <= d["rounds"] <= 32, d
    want, comp = ref.compress_hc(src, _bound(BSZ), 2)
    assert int(res[0]) == want and np.array_equal(outs[0], comp[:want])


@pytest.mark.parametrize("cs", [False, True])
def test_gpu_mx_encode_records(ref, orc, eng, body_data, monkeypatch, cs):
    _small_env(monkeypatch)
    srcs = _cut(body_data, K256)
    c0 = eng.counters()
    recs = eng.encode_records(srcs, K256, cs, level=2)
    assert _mx(eng, c0)["blocks"] == len(srcs)
    for i, (s, r) in enumerate(zip(srcs, recs)):
        assert r.tobytes() == _record(ref, orc, s, K256, cs), (i, cs)
    assert recs[1][3] & 0x80                                               # the random block is stored


def test_gpu_mx_device_resident_calls(ref, orc, eng, blocks, body_data, monkeypatch):
    """plz4hip_dev_compress (maxLen > 0), plz4hip_dev_encode_records and plz4hip_dev_encode_body (recOff, recLen, body bytes)."""
    import torch
    _small_env(monkeypatch)
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    nb, stride, bound = len(blocks), N + 64 + 3, _bound(N)
    d_src = torch.zeros(nb * stride, dtype=torch.uint8, device=dev)
    for i, x in enumerate(blocks):
        d_src[i * stride:i * stride + N] = torch.from_numpy(x.copy()).to(dev)
    d_len = torch.full((nb,), N, dtype=torch.int32, device=dev)
    d_cap = torch.full((nb,), bound, dtype=torch.int32, device=dev)
    d_dst = torch.zeros(nb * (bound + 64), dtype=torch.uint8, device=dev)
    d_res = torch.zeros(nb, dtype=torch.int32, device=dev)
    c0 = eng.counters()
    eng._chk(eng.L.plz4hip_dev_compress(eng.h, nb, d_src.data_ptr(), stride, d_len.data_ptr(), d_dst.data_ptr(), bound + 64,
                                        d_cap.data_ptr(), 2, N, d_res.data_ptr(), s))
    torch.cuda.synchronize()
    assert _mx(eng, c0)["blocks"] == nb
    res = d_res.cpu().numpy(); out = d_dst.cpu().numpy()
    for i, x in enumerate(blocks):
        want, comp = ref.compress_hc(x, bound, 2)
        assert int(res[i]) == want and np.array_equal(out[i * (bound + 64):i * (bound + 64) + want], comp[:want]), i

    srcs = _cut(body_data, K256)
    d_in = torch.from_numpy(body_data.copy()).to(dev)
    sstride = eng.stage_stride(K256)
    for cs in (False, True):
        want = [_record(ref, orc, x, K256, cs) for x in srcs]
        d_stage = torch.zeros(len(srcs) * sstride, dtype=torch.uint8, device=dev)
        d_rl = torch.zeros(len(srcs), dtype=torch.int32, device=dev)
        c0 = eng.counters()
        eng.dev_encode_records(d_in.data_ptr(), body_data.size, K256, cs, d_stage.data_ptr(), d_rl.data_ptr(), s, level=2)
        torch.cuda.synchronize()
        assert _mx(eng, c0)["blocks"] == len(srcs)
        stage = d_stage.cpu().numpy(); rl = d_rl.cpu().numpy()
        for i, w in enumerate(want):
            assert int(rl[i]) == len(w) and stage[i * sstride:i * sstride + len(w)].tobytes() == w, (cs, i)

        want_body = b"".join(want)
        d_body = torch.zeros(len(want_body) + 100, dtype=torch.uint8, device=dev)
        d_off = torch.full((len(srcs) + 1,), -1, dtype=torch.int64, device=dev)
        d_rl.zero_()
        c0 = eng.counters()
        eng.dev_encode_body(d_in.data_ptr(), body_data.size, K256, cs, d_body.data_ptr(), d_body.numel(), d_off.data_ptr(), d_rl.data_ptr(), s, level=2)
        torch.cuda.synchronize()
        assert _mx(eng, c0)["blocks"] == len(srcs)
        offs = np.concatenate([[0], np.cumsum([len(w) for w in want])])
        assert d_off.cpu().numpy().tolist() == offs.tolist()
        assert d_rl.cpu().numpy().tolist() == [len(w) for w in want]
        assert d_body[:len(want_body)].cpu().numpy().tobytes() == want_body, cs


def test_gpu_mx_many_rounds(ref, eng, monkeypatch):
    """8 KiB pieces started with no warm-up on 1 MiB of text: pieces walk again, more than one round -- and still the same bytes."""
    _small_env(monkeypatch, "8", "0")
    src = np.ascontiguousarray(synth.text(1 << 20, seed=9))
    c0 = eng.counters()
    res, outs = eng.compress_batch([src], [_bound(src.size)], level=2)
    d = _mx(eng, c0)
    assert d["blocks"] == 1 and d["rounds"] > 1 and d["again"] > 0, d
    want, comp = ref.compress_hc(src, _bound(src.size), 2)
    assert int(res[0]) == want and np.array_equal(outs[0], comp[:want])


def test_gpu_mx_mixed_lengths_in_one_call(ref, eng, monkeypatch):
    """An empty block, a 100-byte block, a block shorter than a piece and a 1 MiB block: the short ones are blocks of one piece."""
    _small_env(monkeypatch, "16", "32")
    t = synth.text(1 << 20, seed=12)
    srcs = [np.zeros(0, dtype=np.uint8), np.ascontiguousarray(t[:100]), np.ascontiguousarray(t[:9000]), np.ascontiguousarray(t)]
    caps = [_bound(x.size) for x in srcs]
    c0 = eng.counters()
    res, outs = eng.compress_batch(srcs, caps, level=2)
    assert _mx(eng, c0)["blocks"] == 4
    for x, cap, r, o in zip(srcs, caps, res, outs):
        want, comp = ref.compress_hc(x, cap, 2)
        assert int(r) == want and np.array_equal(o, comp[:want]), x.size


def test_gpu_mx_tight_capacity_writes_nothing_behind_dst(ref, eng, blocks, monkeypatch):
    """dstCap one byte below the compressed size: result 0 as the one-wave route, the bytes behind dst + dstCap untouched."""
    import torch
    _small_env(monkeypatch)
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    nb, stride = len(blocks), N + 64 + 3
    sizes = [ref.compress_hc(x, _bound(N), 2)[0] for x in blocks]
    caps = [sizes[0] - 1, sizes[1], sizes[2] - 1]
    dstride = max(sizes) + 256
    d_src = torch.zeros(nb * stride, dtype=torch.uint8, device=dev)
    for i, x in enumerate(blocks):
        d_src[i * stride:i * stride + N] = torch.from_numpy(x.copy()).to(dev)
    d_len = torch.full((nb,), N, dtype=torch.int32, device=dev)
    d_cap = torch.tensor(caps, dtype=torch.int32, device=dev)
    d_dst = torch.full((nb * dstride,), 0xA5, dtype=torch.uint8, device=dev)
    d_res = torch.full((nb,), -7, dtype=torch.int32, device=dev)
    c0 = eng.counters()
    eng._chk(eng.L.plz4hip_dev_compress(eng.h, nb, d_src.data_ptr(), stride, d_len.data_ptr(), d_dst.data_ptr(), dstride,
                                        d_cap.data_ptr(), 2, N, d_res.data_ptr(), s))
    torch.cuda.synchronize()
    assert _mx(eng, c0)["blocks"] == nb
    res = d_res.cpu().numpy(); out = d_dst.cpu().numpy()
    assert res.tolist() == [0, sizes[1], 0]
    for i, cap in enumerate(caps):
        assert np.all(out[i * dstride + cap:(i + 1) * dstride] == 0xA5), i
    assert np.array_equal(out[dstride:dstride + sizes[1]], ref.compress_hc(blocks[1], sizes[1], 2)[1])


def test_gpu_mx_limit_plus_one_blocks(ref, eng, blocks, monkeypatch):
    """The limit set to 2: a call of 3 blocks keeps the one-wave walk (counter unchanged), one of 2 takes the pieces; equal bytes."""
    _small_env(monkeypatch)
    monkeypatch.setenv("PLZ4HIP_MX_MAX_BLOCKS", "2")
    caps = [_bound(N)] * 3
    c0 = eng.counters()
    res3, outs3 = eng.compress_batch(blocks, caps, level=2)
    assert _mx(eng, c0)["blocks"] == 0
    c0 = eng.counters()
    res2, outs2 = eng.compress_batch(blocks[:2], caps[:2], level=2)
    assert _mx(eng, c0)["blocks"] == 2
    for i, x in enumerate(blocks):
        want, comp = ref.compress_hc(x, caps[i], 2)
        assert int(res3[i]) == want and np.array_equal(outs3[i], comp[:want]), i
        if i < 2:
            assert int(res2[i]) == want and np.array_equal(outs2[i], outs3[i]), i


_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from plz4_amd import synth
from plz4_amd._native import Engine
e = Engine(0)
n = 200 * 1024 + 13
srcs = [np.ascontiguousarray(synth.text(n, seed=51 + i)) for i in range(2)]
res, outs = e.compress_batch(srcs, [n + n // 255 + 16] * 2, level=2)
recs = e.encode_records(srcs, 256 << 10, True, level=2)
np.save(sys.argv[2], np.concatenate(outs + recs))
print(json.dumps({"res": [int(r) for r in res], "counters": e.counters()}))
e.close()
"""


def test_gpu_mx_off_gives_the_same_bytes(eng, tmp_path, monkeypatch):
    """PLZ4HIP_MX_MAX_BLOCKS=0 (in a fresh child process): the one-wave walk, counter 0, the same bytes as the pieces give here."""
    _small_env(monkeypatch)
    srcs = [np.ascontiguousarray(synth.text(N, seed=51 + i)) for i in range(2)]
    c0 = eng.counters()
    res, outs = eng.compress_batch(srcs, [_bound(N)] * 2, level=2)
    recs = eng.encode_records(srcs, K256, True, level=2)
    assert _mx(eng, c0)["blocks"] == 4
    mine = np.concatenate(outs + recs)
    env = dict(os.environ, PLZ4HIP_MX_MAX_BLOCKS="0")
    out = str(tmp_path / "off.npy")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, out], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got["counters"]["mx_blocks"] == 0
    assert got["res"] == [int(r) for r in res]
    assert np.array_equal(np.load(out), mine)


def test_gpu_mx_one_ctx_in_sequence_and_workspace_given_back(ref, orc, blocks, monkeypatch):
    """One ctx: mx call, level-1 few-block call, level-9 call, few-block decode, trim, mx call, close.  Every result right; after trim
    the device memory is back (the tolerance of test_gpu_fx_workspace_is_given_back)."""
    import torch
    from plz4_amd._native import Engine
    _small_env(monkeypatch)
    torch.cuda.init()
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    e = Engine(0)
    bound = _bound(N)
    want2 = [ref.compress_hc(x, bound, 2) for x in blocks]
    c0 = e.counters()
    res, outs = e.compress_batch(blocks, [bound] * 3, level=2)
    assert all(int(r) == w[0] and np.array_equal(o, w[1][:w[0]]) for r, o, w in zip(res, outs, want2))
    free1, _ = torch.cuda.mem_get_info()
    r1, o1 = e.compress_batch(blocks, [bound] * 3)                          # level 1, few blocks above 64 KiB: the Fx route
    assert all(int(r) == orc.compress_fast(x, bound)[0] for x, r in zip(blocks, r1))
    r9, o9 = e.compress_batch(blocks, [bound] * 3, level=9)
    for x, r, o in zip(blocks, r9, o9):
        w, comp = ref.compress_hc(x, bound, 9)
        assert int(r) == w and np.array_equal(o, comp[:w])
    rd, dec = e.decompress_batch([o.copy() for o in outs], [N] * 3)          # the few-block decoder
    assert all(int(r) == N and np.array_equal(d, x) for r, d, x in zip(rd, dec, blocks))
    c1 = e.counters()
    assert c1["mx_blocks"] - c0["mx_blocks"] == 3 and c1["fx_blocks"] - c0["fx_blocks"] == 3 and c1["dx_blocks"] - c0["dx_blocks"] == 3, c1
    e.trim()
    torch.cuda.synchronize()
    free2, _ = torch.cuda.mem_get_info()
    assert free1 < free0                                                    # (the calls held their workspaces)
    assert free2 >= free0 - (64 << 20), (free0 >> 20, free1 >> 20, free2 >> 20)
    res, outs = e.compress_batch(blocks, [bound] * 3, level=2)
    assert all(int(r) == w[0] and np.array_equal(o, w[1][:w[0]]) for r, o, w in zip(res, outs, want2))
    assert e.counters()["mx_blocks"] - c0["mx_blocks"] == 6
    e.close()
    torch.cuda.synchronize()
    free3, _ = torch.cuda.mem_get_info()
    assert free3 >= free0 - (64 << 20), (free0 >> 20, free3 >> 20)


def test_gpu_mx_two_streams_of_one_ctx(ref, eng, blocks, monkeypatch):
    """Two device calls enqueued on two streams before anything is waited for: the second waits for the pieces' workspace on the device."""
    import torch
    _small_env(monkeypatch)
    dev = torch.device("cuda:0")
    nb, stride, bound = len(blocks), N + 64 + 3, _bound(N)
    orders = (blocks, blocks[::-1])
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    bufs = []
    for srcs in orders:
        d_src = torch.zeros(nb * stride, dtype=torch.uint8, device=dev)
        for i, x in enumerate(srcs):
            d_src[i * stride:i * stride + N] = torch.from_numpy(x.copy()).to(dev)
        bufs.append((d_src, torch.full((nb,), N, dtype=torch.int32, device=dev), torch.full((nb,), bound, dtype=torch.int32, device=dev),
                     torch.zeros(nb * (bound + 64), dtype=torch.uint8, device=dev), torch.zeros(nb, dtype=torch.int32, device=dev)))
    torch.cuda.synchronize()
    c0 = eng.counters()
    for st, (d_src, d_len, d_cap, d_dst, d_res) in zip(streams, bufs):
        eng._chk(eng.L.plz4hip_dev_compress(eng.h, nb, d_src.data_ptr(), stride, d_len.data_ptr(), d_dst.data_ptr(), bound + 64,
                                            d_cap.data_ptr(), 2, N, d_res.data_ptr(), st.cuda_stream))
    torch.cuda.synchronize()
    assert _mx(eng, c0)["blocks"] == 2 * nb
    for srcs, (_, _, _, d_dst, d_res) in zip(orders, bufs):
        res = d_res.cpu().numpy(); out = d_dst.cpu().numpy()
        for i, x in enumerate(srcs):
            want, comp = ref.compress_hc(x, bound, 2)
            assert int(res[i]) == want and np.array_equal(out[i * (bound + 64):i * (bound + 64) + want], comp[:want]), i
