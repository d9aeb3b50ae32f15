"""Linked frames of any length across the whole chip, through the C ABI: a linked decode call of more blocks than one pass of the
few-block path takes is cut into groups of consecutive blocks (launch_decode; PLZ4HIP_DXL_GROUP_BLOCKS) and must come back exactly
as the reference's reader walks it -- results, status, bytes, the window handed back -- with plz4hip_ctx_counters showing that the
groups answered it; plz4hip_dev_decode_records_ex does the same from a device-resident frame body.  The shapes are the smallest that
cross a group border; calls that set an environment switch run in a fresh child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import dxl_group_cases as gc
from orclib import ROOT
from plz4_amd import synth

pytestmark = pytest.mark.gpu

BSZ = gc.BSZ
OK, HASH, CORRUPT = gc.OK, gc.HASH, gc.CORRUPT
E_ARG = -1


@pytest.fixture(scope="module")
def eng():
    from plz4_amd._native import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def long_chain(orc):
    """One chain of 130 blocks of 64 KiB of T text under a 64 KiB dictionary, block checksums on; none of its records is stored.
    want[checksum]: the reference reader's blocks and window."""
    dct = np.ascontiguousarray(synth.text(65536, seed=77))
    text = synth.text(130 * BSZ, seed=31)
    blocks = [np.ascontiguousarray(text[i * BSZ:(i + 1) * BSZ]) for i in range(130)]
    recs = gc.frame(orc, blocks, BSZ, dct)
    assert [gc.is_stored(r) for r in recs] == [False] * 130
    w0, wl0 = gc.start_window(dct)
    bare = [np.ascontiguousarray(r[:-4]) for r in recs]
    want = {True: gc.walk(orc, recs, BSZ, True, w0, wl0), False: gc.walk(orc, bare, BSZ, False, w0, wl0)}
    assert all(s == OK for _, s, _ in want[True][0])
    return blocks, dct, {True: recs, False: bare}, want


@pytest.fixture(scope="module")
def cases(orc):
    return gc.build_cases(orc)


def _assert_chain(got, want, wwin, window, wl, tag):
    res, st, outs = got
    for i, (wr, ws, wo) in enumerate(want):
        assert (int(res[i]), int(st[i])) == (wr, ws), (tag, i, int(res[i]), int(st[i]), wr, ws)
        if wo is not None:
            assert np.array_equal(outs[i][:wr], wo), (tag, i)
    assert int(wl) == wwin.size and np.array_equal(window[:wwin.size], wwin), tag


# ---- a child process under an environment switch: the calls of an .npz through decode_records_ex (one chain) / decode_records_chains
_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from plz4_amd._native import Engine
z = np.load(sys.argv[2])
meta = json.loads(str(z["meta"]))
e = Engine(0)
info, arrs = [], {}
for k, m in enumerate(meta):
    recs = [np.ascontiguousarray(z["c%d_r%d" % (k, i)]) for i in range(sum(m["chains"]))]
    windows = z["c%d_w" % k].copy(); wl = z["c%d_wl" % k].copy()
    c0 = e.counters()
    if len(m["chains"]) == 1:
        res, st, outs, l = e.decode_records_ex(recs, m["bsz"], m["checksum"], linked=True, window=windows[0], window_len=int(wl[0]))
        wl = np.array([l], np.int32)
    else:
        chains, a = [], 0
        for n in m["chains"]:
            chains.append(recs[a:a + n]); a += n
        got, wl = e.decode_records_chains(chains, m["bsz"], m["checksum"], windows=windows, window_lens=wl)
        res = np.concatenate([g[0] for g in got]); st = np.concatenate([g[1] for g in got]); outs = [o for g in got for o in g[2]]
    c1 = e.counters()
    info.append({"dxl_blocks": c1["dxl_blocks"] - c0["dxl_blocks"], "groups": c1.get("dxl_groups_last", -1)})
    arrs["c%d_res" % k] = np.asarray(res, np.int32); arrs["c%d_st" % k] = np.asarray(st, np.int32)
    arrs["c%d_w" % k] = windows; arrs["c%d_wl" % k] = np.asarray(wl, np.int32)
    arrs["c%d_out" % k] = np.concatenate([o for o in outs] + [np.zeros(0, np.uint8)])
np.savez(sys.argv[3], **arrs)
print(json.dumps(info))
e.close()
"""


def _run_child(tmp_path, env, calls):
    """calls: [(chains of records, bsz, checksum, windows nCh x 65536, wlens)] -> per call (per chain (res, st, outs)), windows, wlens, info"""
    meta, arrs = [], {}
    for k, (chains, bsz, checksum, windows, wlens) in enumerate(calls):
        meta.append({"chains": [len(ch) for ch in chains], "bsz": bsz, "checksum": bool(checksum)})
        for i, r in enumerate(r for ch in chains for r in ch):
            arrs["c%d_r%d" % (k, i)] = r
        arrs["c%d_w" % k] = np.ascontiguousarray(windows); arrs["c%d_wl" % k] = np.asarray(wlens, np.int32)
    src, out = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, meta=json.dumps(meta), **arrs)
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, src, out], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    info = json.loads(p.stdout.strip().splitlines()[-1])
    z = np.load(out)
    result = []
    for k, (chains, *_rest) in enumerate(calls):
        res, st, flat = z["c%d_res" % k], z["c%d_st" % k], z["c%d_out" % k]
        got, a, o = [], 0, 0
        for ch in chains:
            outs = []
            for i in range(a, a + len(ch)):
                n = max(int(res[i]), 0); outs.append(flat[o:o + n]); o += n
            got.append((res[a:a + len(ch)], st[a:a + len(ch)], outs)); a += len(ch)
        result.append((got, z["c%d_w" % k], z["c%d_wl" % k], info[k]))
    return result


# ---- default settings ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("checksum", [True, False])
def test_gpu_dxl_groups_long_chain(orc, eng, long_chain, checksum):
    """130 blocks in one call: the oracle's outcome; as many blocks answered by the few-block path as when the chain is fed in calls
    of at most 128 blocks with the window carried; at least two groups."""
    blocks, dct, recs_by, want_by = long_chain
    recs = recs_by[checksum]; want, wwin = want_by[checksum]
    w0, wl0 = gc.start_window(dct)
    deltas = {}
    for parts in ([recs[:128], recs[128:]], [recs]):
        window, wl = w0.copy(), wl0
        c0 = eng.counters()
        res, st, outs = [], [], []
        for part in parts:
            r, s, o, wl = eng.decode_records_ex(part, BSZ, checksum, linked=True, window=window, window_len=wl)
            res += list(r); st += list(s); outs += o
        c1 = eng.counters()
        _assert_chain((res, st, outs), want, wwin, window, wl, (checksum, len(parts)))
        for b, o in zip(blocks, outs):
            assert np.array_equal(b, o)
        deltas[len(parts)] = c1["dxl_blocks"] - c0["dxl_blocks"]
    print("dxl_blocks: two calls %d, one call %d; groups %d" % (deltas[2], deltas[1], c1["dxl_groups_last"]))
    assert deltas[2] == 130
    assert deltas[1] == deltas[2]
    assert c1["dxl_groups_last"] >= 2


# ---- PLZ4HIP_DXL_GROUP_BLOCKS ----------------------------------------------------------------------------------------------------
def test_gpu_dxl_groups_of_four_cases(cases, tmp_path):
    """the lane-emulated suite's cases through the ABI at four blocks per group (all but the one that forces a group's jump rounds,
    which only the emulation can)"""
    calls = [(c.chains, c.bsz, c.checksum, c.windows, c.wlens) for c in cases]
    for case, (got, windows, wlens, info) in zip(cases, _run_child(tmp_path, {"PLZ4HIP_DXL_GROUP_BLOCKS": "4"}, calls)):
        case.check(got, windows, wlens)
        nb = sum(len(ch) for ch in case.chains)
        assert info == {"dxl_blocks": case.taken, "groups": -(-nb // 4)}, (case.name, info, case.taken)


def test_gpu_dxl_groups_of_sixteen_4mib(orc, tmp_path):
    """one chain of 40 blocks of 4 MiB (T / M / Z in turn) in groups of 16"""
    bsz = 4 << 20
    dct = np.ascontiguousarray(synth.text(65536, seed=78))
    blocks = [np.ascontiguousarray(synth.make("TMZ"[i % 3], bsz, 1 << 16, seed=40 + i % 6)) for i in range(40)]
    recs = gc.frame(orc, blocks, bsz, dct)
    assert not any(gc.is_stored(r) for r in recs)
    w0, wl0 = gc.start_window(dct)
    want, wwin = gc.walk(orc, recs, bsz, True, w0, wl0)
    (got, windows, wlens, info), = _run_child(tmp_path, {"PLZ4HIP_DXL_GROUP_BLOCKS": "16"}, [([recs], bsz, True, w0.reshape(1, 65536), [wl0])])
    _assert_chain(got[0], want, wwin, windows[0], wlens[0], "40x4MiB")
    for b, o in zip(blocks, got[0][2]):
        assert np.array_equal(b, o)
    assert info == {"dxl_blocks": 40, "groups": 3}, info


def test_gpu_dxl_groups_off_gives_the_same(orc, long_chain, tmp_path):
    """PLZ4HIP_DXL_GROUP_BLOCKS=0: one wave per chain beyond 128 blocks, as before -- the same bytes, status and window"""
    blocks, dct, recs_by, want_by = long_chain
    w0, wl0 = gc.start_window(dct)
    (got, windows, wlens, info), = _run_child(tmp_path, {"PLZ4HIP_DXL_GROUP_BLOCKS": "0"}, [([recs_by[True]], BSZ, True, w0.reshape(1, 65536), [wl0])])
    want, wwin = want_by[True]
    _assert_chain(got[0], want, wwin, windows[0], wlens[0], "off")
    assert info["dxl_blocks"] == 0, info


# ---- the group policy -------------------------------------------------------------------------------------------------------------
def test_gpu_dxl_groups_policy(orc, eng, long_chain):
    """few long chains take groups, many short ones stay on one wave per chain"""
    blocks, dct, recs_by, want_by = long_chain
    w0, wl0 = gc.start_window(dct)
    want, _ = want_by[True]
    # 2 chains x 70 blocks: the second chain is the first 70 blocks of the first one's frame again
    chains = [recs_by[True][:70], recs_by[True][:70]]
    wwin = gc.walk(orc, chains[0], BSZ, True, w0, wl0)[1]
    wall = np.stack([w0, w0]).copy()
    c0 = eng.counters()
    got, wl = eng.decode_records_chains(chains, BSZ, True, windows=wall, window_lens=np.array([wl0, wl0], np.int32))
    c1 = eng.counters()
    for k in range(2):
        _assert_chain(got[k], want[:70], wwin, wall[k], wl[k], ("2x70", k))
    assert c1["dxl_blocks"] - c0["dxl_blocks"] == 140 and c1["dxl_groups_last"] >= 2, (c0, c1)
    # 1024 chains x 1 block
    singles = [gc.frame(orc, [b], BSZ, None) for b in blocks[:16]]
    chains = [singles[k % 16] for k in range(1024)]
    c0 = eng.counters()
    got, wl = eng.decode_records_chains(chains, BSZ, True)
    c1 = eng.counters()
    for k in range(1024):
        res, st, outs = got[k]
        assert (int(res[0]), int(st[0])) == (BSZ, OK) and np.array_equal(outs[0], blocks[k % 16]), k
        assert int(wl[k]) == 65536
    assert c1["dxl_blocks"] - c0["dxl_blocks"] == 0, (c0, c1)


# ---- plz4hip_dev_decode_records_ex -------------------------------------------------------------------------------------------------
def _dev_call(eng, chains, bsz, checksum, windows=None, wlens=None, d=None):
    """the records packed back to back on the device, as dev_encode_body packs them -> per block res, st, outs; windows, wlens"""
    import torch
    dev = torch.device("cuda:0")
    recs = [r for ch in chains for r in ch]
    nb = len(recs)
    off = np.zeros(nb + 1, np.int64); off[1:] = np.cumsum([r.size for r in recs])
    d_body = torch.from_numpy(np.concatenate(recs + [np.zeros(64, np.uint8)])).to(dev)
    d_off = torch.from_numpy(off).to(dev)
    cap = bsz + 8; stride = (cap + 64 + 15) // 16 * 16
    d_out = torch.zeros(nb * stride + 64, dtype=torch.uint8, device=dev)
    d_res = torch.full((nb,), -7, dtype=torch.int32, device=dev); d_st = torch.full((nb,), -7, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    if d is None:
        nch = len(chains)
        w = np.zeros((nch, 131072), np.uint8); w[:, :65536] = windows
        d_w = torch.from_numpy(w).to(dev); d_wl = torch.from_numpy(np.asarray(wlens, np.int32)).to(dev)
        first = np.concatenate([[0], np.cumsum([len(ch) for ch in chains])]).astype(np.int32)
        eng.dev_decode_records_ex(d_body.data_ptr(), d_off.data_ptr(), nb, bsz, checksum, d_out.data_ptr(), stride, cap, d_res.data_ptr(), d_st.data_ptr(),
                                  linked=True, chain_first=first if nch > 1 else None, windows_ptr=d_w.data_ptr(), window_len_ptr=d_wl.data_ptr(), stream=s)
    else:
        eng.dev_decode_records_ex(d_body.data_ptr(), d_off.data_ptr(), nb, bsz, checksum, d_out.data_ptr(), stride, cap, d_res.data_ptr(), d_st.data_ptr(),
                                  linked=False, d=d, stream=s)
    torch.cuda.synchronize()
    res, st, out = d_res.cpu().numpy(), d_st.cpu().numpy(), d_out.cpu().numpy()
    outs = [out[i * stride:i * stride + max(int(res[i]), 0)] for i in range(nb)]
    if d is None:
        return res, st, outs, d_w.cpu().numpy()[:, :65536], d_wl.cpu().numpy()
    return res, st, outs, None, None


def test_gpu_dev_decode_records_ex_linked(orc, eng, long_chain, cases):
    """the 130-block chain and three chains of 5 / 1 / 6 blocks from a device-resident body equal the host call"""
    blocks, dct, recs_by, want_by = long_chain
    w0, wl0 = gc.start_window(dct)
    for checksum in (True, False):
        c0 = eng.counters()
        res, st, outs, windows, wlens = _dev_call(eng, [recs_by[checksum]], BSZ, checksum, w0.reshape(1, 65536), [wl0])
        c1 = eng.counters()
        want, wwin = want_by[checksum]
        _assert_chain((res, st, outs), want, wwin, windows[0], wlens[0], ("dev", checksum))
        hw = w0.copy()
        hres, hst, houts, hwl = eng.decode_records_ex(recs_by[checksum], BSZ, checksum, linked=True, window=hw, window_len=wl0)
        assert np.array_equal(res, hres) and np.array_equal(st, hst) and int(wlens[0]) == hwl and np.array_equal(windows[0][:hwl], hw[:hwl])
        assert all(np.array_equal(a, b) for a, b in zip(outs, houts))
        assert c1["dxl_blocks"] - c0["dxl_blocks"] == 130 and c1["dxl_groups_last"] >= 2
    case = next(c for c in cases if c.name == "chains-5-1-6")
    c0 = eng.counters()
    res, st, outs, windows, wlens = _dev_call(eng, case.chains, case.bsz, case.checksum, case.windows, case.wlens)
    assert eng.counters()["dxl_blocks"] - c0["dxl_blocks"] == 12
    got, a = [], 0
    for ch in case.chains:
        got.append((res[a:a + len(ch)], st[a:a + len(ch)], outs[a:a + len(ch)])); a += len(ch)
    case.check(got, windows, wlens)
    hwin = case.windows.copy()
    hgot, hwl = eng.decode_records_chains(case.chains, case.bsz, case.checksum, windows=hwin, window_lens=np.array(case.wlens, np.int32))
    for (r1, s1, o1), (r2, s2, o2) in zip(got, hgot):
        assert np.array_equal(r1, r2) and np.array_equal(s1, s2) and all(np.array_equal(a, b) for a, b in zip(o1, o2))
    assert np.array_equal(wlens, hwl)


@pytest.mark.parametrize("nb", [3, 200])
def test_gpu_dev_decode_records_ex_dictionary(orc, eng, nb):
    """independent blocks under a dictionary, few (the few-block path) and many (one wave per block)"""
    user = np.ascontiguousarray(synth.text(70000, seed=99))
    dctx = orc.dict_ctx(user); d = eng.dict_create(user)
    try:
        text = synth.text(8 * BSZ, seed=11)
        srcs = [np.ascontiguousarray(text[(i % 8) * BSZ:(i % 8 + 1) * BSZ]) for i in range(nb)]
        recs = [gc.record(orc, 1, np.ascontiguousarray(orc.compress_indie_dict(s, BSZ, dctx)[1]), s, True) for s in srcs[:8]]
        recs = [recs[i % 8] for i in range(nb)]
        c0 = eng.counters()
        res, st, outs, _, _ = _dev_call(eng, [recs], BSZ, True, d=d)
        taken = eng.counters()["dxl_blocks"] - c0["dxl_blocks"]
        hres, hst, houts, _ = eng.decode_records_ex(recs, BSZ, True, linked=False, d=d)
        assert np.array_equal(res, hres) and np.array_equal(st, hst) and not st.any()
        for s, o in zip(srcs, outs):
            assert np.array_equal(s, o)
        assert taken == (nb if nb <= 128 else 0), taken
    finally:
        eng.dict_destroy(d)


def test_gpu_dev_decode_records_ex_argument_errors(eng):
    import torch
    from plz4_amd._native import EngineError
    dev = torch.device("cuda:0")
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
    off = torch.zeros(8, dtype=torch.int64, device=dev)
    i32 = torch.zeros(8, dtype=torch.int32, device=dev)
    p = buf.data_ptr()

    def call(**kw):
        a = dict(linked=True, chain_first=None, n_chains=1, windows_ptr=p, window_len_ptr=i32.data_ptr(), d=None, nblocks=4)
        a.update(kw)
        nblocks = a.pop("nblocks")
        eng.dev_decode_records_ex(p, off.data_ptr(), nblocks, BSZ, True, p, BSZ + 16, BSZ + 8, i32.data_ptr(), i32.data_ptr(), **a)

    bad = [dict(chain_first=[1, 4]), dict(chain_first=[0, 3, 2, 4]), dict(chain_first=[0, 2, 3]), dict(chain_first=[0, 2, 5]),
           dict(windows_ptr=None), dict(window_len_ptr=None), dict(linked=False), dict(n_chains=0), dict(n_chains=2), dict(nblocks=-1)]
    for kw in bad:
        with pytest.raises(EngineError) as ei:
            call(**kw)
        assert ei.value.code == E_ARG, kw
    d = eng.dict_create(np.ascontiguousarray(synth.text(1000, seed=1)))
    try:
        with pytest.raises(EngineError) as ei:
            call(d=d)                                                       # linked = 1 takes its dictionary through the window
        assert ei.value.code == E_ARG
    finally:
        eng.dict_destroy(d)
    torch.cuda.synchronize()


# ---- content hash; mixed calls -----------------------------------------------------------------------------------------------------
def test_gpu_dxl_groups_content_hash(orc, eng, long_chain):
    blocks, dct, recs_by, want_by = long_chain
    h = eng.hash_create()
    eng.set_content_hash(h)
    try:
        w, wl = gc.start_window(dct)
        res, st, outs, wl = eng.decode_records_ex(recs_by[True], BSZ, True, linked=True, window=w, window_len=wl)
        assert not any(st) and eng.counters()["dxl_groups_last"] >= 2
        assert eng.hash_sum(h) == orc.xxh32(np.concatenate(blocks))
    finally:
        eng.set_content_hash(None)
        eng.hash_destroy(h)


def test_gpu_dxl_groups_one_ctx_mixed_calls(orc, long_chain):
    """a grouped decode, an HC encode with a dictionary and linked blocks, a few-block decode, trim, the grouped decode again"""
    from plz4_amd._native import Engine
    blocks, dct, recs_by, want_by = long_chain
    want, wwin = want_by[True]
    e = Engine(0)
    d = e.dict_create(dct)
    try:
        def grouped():
            w, wl = gc.start_window(dct)
            c0 = e.counters()
            res, st, outs, wl = e.decode_records_ex(recs_by[True], BSZ, True, linked=True, window=w, window_len=wl)
            c1 = e.counters()
            _assert_chain((res, st, outs), want, wwin, w, wl, "grouped")
            assert c1["dxl_blocks"] - c0["dxl_blocks"] == 130 and c1["dxl_groups_last"] >= 2
        grouped()
        srcs = blocks[:4]
        recs = [np.ascontiguousarray(r) for r in e.encode_records_ex(srcs, BSZ, True, linked=True, d=d, level=9)]
        w, wl = gc.start_window(dct)
        c0 = e.counters()
        res, st, outs, wl = e.decode_records_ex(recs, BSZ, True, linked=True, window=w, window_len=wl)
        assert not any(st) and all(np.array_equal(s, o) for s, o in zip(srcs, outs))
        assert e.counters()["dxl_blocks"] - c0["dxl_blocks"] == sum(not gc.is_stored(r) for r in recs)
        e.trim()
        grouped()
    finally:
        e.dict_destroy(d)
        e.close()
