"""Chain and lists of a few blocks built in pieces across the chip (plz4_amd/csrc/lz4hc_lists_device.inl, k_hb_count .. k_hb_chain
behind hc_build): calls of a handful of blocks at levels 3..12 on the segmented route.  Everything behind the builder is untouched,
so every entry point must give the real liblz4's bytes, return values and capacity verdicts (LZ4_compress_HC; the record streams
of tests/hcdict.py) exactly as before.  Every case asserts the hb_blocks delta of plz4hip_ctx_counters: a silent fallback to one
wave per block fails the test."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import hcdict
from plz4_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
N = 200 * 1024 + 13
K256 = 256 << 10
BSZ = 4 << 20


def _bound(n):
    return n + n // 255 + 16


def _small_env(mp, piece="8"):
    mp.setenv("PLZ4HIP_HB_PIECE_KIB", piece)
    mp.setenv("PLZ4HIP_HB_MAX_BLOCKS", "64")


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
def want_hc(ref, blocks):
    """LZ4_compress_HC of the three blocks, per (level, capacity), computed on first use and kept."""
    memo = {}

    def get(i, level, cap):
        if (i, level, cap) not in memo:
            w, comp = ref.compress_hc(blocks[i], cap, level)
            memo[(i, level, cap)] = (w, comp[:w].copy())
        return memo[(i, level, cap)]
    return get


@pytest.fixture(scope="module")
def dict64():
    d = np.ascontiguousarray(synth.text(65536, seed=77))
    d.setflags(write=False)
    return d


def _hb(eng, c0):
    c1 = eng.counters()
    return {"blocks": c1["hb_blocks"] - c0["hb_blocks"], "pieces": c1["hb_pieces_last"], "hcx": c1["hcx_blocks"] - c0["hcx_blocks"]}


@pytest.mark.parametrize("level", [3, 6, 9, 10, 12])
@pytest.mark.parametrize("nb", [1, 3])
def test_gpu_hb_compress_batch(eng, blocks, want_hc, monkeypatch, nb, level):
    """26 pieces of 8 KiB per block; the capacities: the bound and n (the verdicts of a tight capacity unchanged)."""
    _small_env(monkeypatch)
    srcs = blocks[:nb]
    for cap in (_bound(N), N):
        c0 = eng.counters()
        res, outs = eng.compress_batch(srcs, [cap] * nb, level=level)
        d = _hb(eng, c0)
        assert d["blocks"] == nb and d["pieces"] == 26, d
        for i, (r, o) in enumerate(zip(res, outs)):
            want, comp = want_hc(i, level, cap)
            assert int(r) == want and np.array_equal(o, comp), (nb, level, cap, i)


def test_gpu_hb_one_4mib_block_at_the_defaults(ref, eng):
    src = np.ascontiguousarray(synth.text(BSZ, seed=7))
    c0 = eng.counters()
    res, outs = eng.compress_batch([src], [_bound(BSZ)], level=9)
    d = _hb(eng, c0)
    assert d["blocks"] == 1 and d["pieces"] >= 2, d
    want, comp = ref.compress_hc(src, _bound(BSZ), 9)
    assert int(res[0]) == want and np.array_equal(outs[0], comp[:want])


def test_gpu_hb_mixed_lengths_in_one_call(ref, eng, monkeypatch):
    """An empty block, a 100-byte block, a block of two pieces and a 1 MiB block: every one of them is built by the four stages."""
    _small_env(monkeypatch)
    t = synth.text(1 << 20, seed=12)
    srcs = [np.zeros(0, dtype=np.uint8), np.ascontiguousarray(t[:100]), np.ascontiguousarray(t[:9000]), np.ascontiguousarray(t)]
    caps = [_bound(x.size) for x in srcs]
    for level in (3, 9):
        c0 = eng.counters()
        res, outs = eng.compress_batch(srcs, caps, level=level)
        d = _hb(eng, c0)
        assert d["blocks"] == 4 and d["pieces"] == 128, d
        for x, cap, r, o in zip(srcs, caps, res, outs):
            want, comp = ref.compress_hc(x, cap, level)
            assert int(r) == want and np.array_equal(o, comp[:want]), (level, x.size)


@pytest.mark.parametrize("level", [3, 9])
def test_gpu_hb_encode_records_ex_linked_behind_a_dictionary(ref, orc, eng, dict64, monkeypatch, level):
    """Three linked 256 KiB blocks behind a 64 KiB dictionary: the lists run over segment + block, the segment's last three
    positions are never inserted."""
    _small_env(monkeypatch)
    t = synth.make("M", 3 * K256, 1 << 16, seed=64)
    srcs = [np.ascontiguousarray(t[i * K256:(i + 1) * K256]) for i in range(3)]
    d = eng.dict_create(dict64.copy())
    want, _ = hcdict.ref_records(ref, orc, srcs, K256, level, True, dict64.copy(), checksum=True)
    c0 = eng.counters()
    recs = eng.encode_records_ex(srcs, K256, True, linked=True, d=d, level=level)
    dl = _hb(eng, c0)
    assert dl["blocks"] == 3 and dl["pieces"] == 40 and dl["hcx"] == 0, dl
    for i, (r, w) in enumerate(zip(recs, want)):
        assert r.tobytes() == w, (level, i)
    eng.dict_destroy(d)


@pytest.mark.parametrize("level", [3, 9])
def test_gpu_hb_encode_records_ex_dictionary_independent(ref, orc, eng, blocks, dict64, monkeypatch, level):
    """Three independent blocks under the dictionary, one of them of at most 4 KiB: that one stays k_hcx's and is not counted."""
    _small_env(monkeypatch)
    srcs = [blocks[0].copy(), np.ascontiguousarray(synth.text(4000, seed=66)), blocks[1].copy()]
    d = eng.dict_create(dict64.copy())
    want, _ = hcdict.ref_records(ref, orc, srcs, K256, level, False, dict64.copy(), checksum=True)
    c0 = eng.counters()
    recs = eng.encode_records_ex(srcs, K256, True, linked=False, d=d, level=level)
    dl = _hb(eng, c0)
    assert dl["blocks"] == 2 and dl["hcx"] == 1, dl
    for i, (r, w) in enumerate(zip(recs, want)):
        assert r.tobytes() == w, (level, i)
    eng.dict_destroy(d)


def _to_dev(blocks_, stride):
    import torch
    dev = torch.device("cuda:0")
    d_src = torch.zeros(len(blocks_) * stride, dtype=torch.uint8, device=dev)
    for i, x in enumerate(blocks_):
        d_src[i * stride:i * stride + x.size] = torch.from_numpy(x.copy()).to(dev)
    return d_src


def test_gpu_hb_device_resident_calls(ref, orc, eng, blocks, want_hc, monkeypatch):
    """plz4hip_dev_compress on a padded stride and plz4hip_dev_encode_records, level 5."""
    import torch
    _small_env(monkeypatch)
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    nb, stride, bound = len(blocks), N + 64 + 3, _bound(N)
    d_src = _to_dev(blocks, stride)
    d_len = torch.full((nb,), N, dtype=torch.int32, device=dev)
    d_cap = torch.full((nb,), bound, dtype=torch.int32, device=dev)
    d_dst = torch.zeros(nb * (bound + 64), dtype=torch.uint8, device=dev)
    d_res = torch.zeros(nb, dtype=torch.int32, device=dev)
    c0 = eng.counters()
    eng._chk(eng.L.plz4hip_dev_compress(eng.h, nb, d_src.data_ptr(), stride, d_len.data_ptr(), d_dst.data_ptr(), bound + 64,
                                        d_cap.data_ptr(), 5, N, d_res.data_ptr(), s))
    torch.cuda.synchronize()
    assert _hb(eng, c0)["blocks"] == nb
    res = d_res.cpu().numpy(); out = d_dst.cpu().numpy()
    for i in range(nb):
        want, comp = want_hc(i, 5, bound)
        assert int(res[i]) == want and np.array_equal(out[i * (bound + 64):i * (bound + 64) + want], comp), i

    data = np.ascontiguousarray(np.concatenate([synth.text(K256, seed=41), synth.random_bytes(K256, seed=42), synth.text(N, seed=43)]))
    srcs = [np.ascontiguousarray(data[o:o + K256]) for o in range(0, data.size, K256)]
    want, _ = hcdict.ref_records(ref, orc, srcs, K256, 5, False, None, checksum=True)
    d_in = torch.from_numpy(data.copy()).to(dev)
    sstride = eng.stage_stride(K256)
    d_stage = torch.zeros(len(srcs) * sstride, dtype=torch.uint8, device=dev)
    d_rl = torch.zeros(len(srcs), dtype=torch.int32, device=dev)
    c0 = eng.counters()
    eng.dev_encode_records(d_in.data_ptr(), data.size, K256, True, d_stage.data_ptr(), d_rl.data_ptr(), s, level=5)
    torch.cuda.synchronize()
    assert _hb(eng, c0)["blocks"] == len(srcs)
    stage = d_stage.cpu().numpy(); rl = d_rl.cpu().numpy()
    for i, w in enumerate(want):
        assert int(rl[i]) == len(w) and stage[i * sstride:i * sstride + len(w)].tobytes() == w, i


def test_gpu_hb_limit_plus_one_blocks(eng, blocks, want_hc, monkeypatch):
    """The limit set to 2: a call of 3 blocks keeps one wave per block (counter unchanged), one of 2 takes the pieces; equal bytes."""
    _small_env(monkeypatch)
    monkeypatch.setenv("PLZ4HIP_HB_MAX_BLOCKS", "2")
    caps = [_bound(N)] * 3
    c0 = eng.counters()
    res3, outs3 = eng.compress_batch(blocks, caps, level=6)
    assert _hb(eng, c0)["blocks"] == 0
    c0 = eng.counters()
    res2, outs2 = eng.compress_batch(blocks[:2], caps[:2], level=6)
    assert _hb(eng, c0)["blocks"] == 2
    for i in range(3):
        want, comp = want_hc(i, 6, caps[i])
        assert int(res3[i]) == want and np.array_equal(outs3[i], comp), i
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
outs = []
res = []
for level in (3, 9, 12):
    r, o = e.compress_batch(srcs, [n + n // 255 + 16] * 2, level=level)
    res += [int(x) for x in r]; outs += o
np.save(sys.argv[2], np.concatenate(outs))
print(json.dumps({"res": res, "counters": e.counters()}))
e.close()
"""


def test_gpu_hb_off_gives_the_same_bytes(eng, tmp_path, monkeypatch):
    """PLZ4HIP_HB_MAX_BLOCKS=0 (in a fresh child process): one wave per block, counter 0, the same bytes as the pieces give here."""
    _small_env(monkeypatch)
    srcs = [np.ascontiguousarray(synth.text(N, seed=51 + i)) for i in range(2)]
    c0 = eng.counters()
    res, outs = [], []
    for level in (3, 9, 12):
        r, o = eng.compress_batch(srcs, [_bound(N)] * 2, level=level)
        res += [int(x) for x in r]; outs += o
    assert _hb(eng, c0)["blocks"] == 6
    mine = np.concatenate(outs)
    env = dict(os.environ, PLZ4HIP_HB_MAX_BLOCKS="0")
    out = str(tmp_path / "off.npy")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, out], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got["counters"]["hb_blocks"] == 0
    assert got["res"] == res
    assert np.array_equal(np.load(out), mine)


def test_gpu_hb_one_ctx_in_sequence_and_workspace_given_back(ref, orc, blocks, want_hc, monkeypatch):
    """One ctx: HB call, level-2 few-block call, few-block decode, trim, HB call, close.  Every result right; after trim the device
    memory is back (the tolerance of test_gpu_mx_one_ctx_in_sequence_and_workspace_given_back)."""
    import torch
    from plz4_amd._native import Engine
    _small_env(monkeypatch)
    torch.cuda.init()
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    e = Engine(0)
    bound = _bound(N)
    c0 = e.counters()
    res, outs = e.compress_batch(blocks, [bound] * 3, level=9)
    assert all(int(r) == want_hc(i, 9, bound)[0] and np.array_equal(o, want_hc(i, 9, bound)[1]) for i, (r, o) in enumerate(zip(res, outs)))
    free1, _ = torch.cuda.mem_get_info()
    r2, o2 = e.compress_batch(blocks, [bound] * 3, level=2)                 # level 2, few blocks: the Mx route
    for i, (r, o) in enumerate(zip(r2, o2)):
        w, comp = ref.compress_hc(blocks[i], bound, 2)
        assert int(r) == w and np.array_equal(o, comp[:w])
    rd, dec = e.decompress_batch([o.copy() for o in outs], [N] * 3)          # the few-block decoder
    assert all(int(r) == N and np.array_equal(d, x) for r, d, x in zip(rd, dec, blocks))
    c1 = e.counters()
    assert c1["hb_blocks"] - c0["hb_blocks"] == 3 and c1["mx_blocks"] - c0["mx_blocks"] == 3 and c1["dx_blocks"] - c0["dx_blocks"] == 3, c1
    e.trim()
    torch.cuda.synchronize()
    free2, _ = torch.cuda.mem_get_info()
    assert free1 < free0                                                    # (the calls held their workspaces)
    assert free2 >= free0 - (64 << 20), (free0 >> 20, free1 >> 20, free2 >> 20)
    res, outs = e.compress_batch(blocks, [bound] * 3, level=9)
    assert all(int(r) == want_hc(i, 9, bound)[0] and np.array_equal(o, want_hc(i, 9, bound)[1]) for i, (r, o) in enumerate(zip(res, outs)))
    assert e.counters()["hb_blocks"] - c0["hb_blocks"] == 6
    e.close()
    torch.cuda.synchronize()
    free3, _ = torch.cuda.mem_get_info()
    assert free3 >= free0 - (64 << 20), (free0 >> 20, free3 >> 20)


def test_gpu_hb_two_streams_of_one_ctx(eng, blocks, want_hc, monkeypatch):
    """Two device calls enqueued on two streams before anything is waited for: the second waits for the HC workspaces on the device."""
    import torch
    _small_env(monkeypatch)
    dev = torch.device("cuda:0")
    nb, stride, bound = len(blocks), N + 64 + 3, _bound(N)
    orders = ([0, 1, 2], [2, 1, 0])
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    bufs = []
    for order in orders:
        bufs.append((_to_dev([blocks[i] for i in order], stride), torch.full((nb,), N, dtype=torch.int32, device=dev),
                     torch.full((nb,), bound, dtype=torch.int32, device=dev),
                     torch.zeros(nb * (bound + 64), dtype=torch.uint8, device=dev), torch.zeros(nb, dtype=torch.int32, device=dev)))
    torch.cuda.synchronize()
    c0 = eng.counters()
    for st, (d_src, d_len, d_cap, d_dst, d_res) in zip(streams, bufs):
        eng._chk(eng.L.plz4hip_dev_compress(eng.h, nb, d_src.data_ptr(), stride, d_len.data_ptr(), d_dst.data_ptr(), bound + 64,
                                            d_cap.data_ptr(), 5, N, d_res.data_ptr(), st.cuda_stream))
    torch.cuda.synchronize()
    assert _hb(eng, c0)["blocks"] == 2 * nb
    for order, (_, _, _, d_dst, d_res) in zip(orders, bufs):
        res = d_res.cpu().numpy(); out = d_dst.cpu().numpy()
        for j, i in enumerate(order):
            want, comp = want_hc(i, 5, bound)
            assert int(res[j]) == want and np.array_equal(out[j * (bound + 64):j * (bound + 64) + want], comp), (order, j)
