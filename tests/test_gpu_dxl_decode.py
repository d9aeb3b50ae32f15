"""Linked and dictionary blocks decoded across the whole chip (dxl_* in lz4_dx_device.inl; k_dxl_link .. k_dxl_finish), through the C
ABI: few blocks with history outside the block must come back exactly as the one-wave kernels give them -- results, status, bytes
and the window handed back -- and plz4hip_ctx_counters must show that the few-block path answered them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from orclib import ROOT
from plz4_amd import synth

pytestmark = pytest.mark.gpu

BSZ = 4 << 20
OK, HASH, CORRUPT = 0, 1, 3


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
    return np.frombuffer(rec, dtype=np.uint8).copy()


def _frame(orc, blocks, bsz, dct):
    """A linked frame's records, block checksums on (without: the record less its last four bytes)."""
    dctx = orc.dict_ctx(dct) if dct is not None else None
    recs, prev = [], None
    for b in blocks:
        tail = None if prev is None else prev[-65536:].copy()
        r, c = orc.compress_linked(b, bsz, tail, dctx if prev is None else None)
        recs.append(_record(orc, r, c[:r], b, True)); prev = b
    return recs


def _start_window(dct):
    w = np.zeros(65536, dtype=np.uint8)
    wl = 0 if dct is None else min(dct.size, 65536)
    if wl:
        w[:wl] = dct[-wl:]
    return w, wl


def _walk(orc, recs, bsz, checksum, window, wl):
    """The reference's reader over a chain's records: per block (result, status, bytes); the window afterwards."""
    win = window[:wl].copy()
    out, dead = [], False
    for rec in recs:
        if dead:
            out.append((0, CORRUPT, None)); continue
        word = int(np.frombuffer(rec[:4].tobytes(), dtype=np.uint32)[0]); sz = word & 0x7FFFFFFF
        assert sz <= bsz and sz + 4 + (4 if checksum else 0) <= rec.size
        payload = np.ascontiguousarray(rec[4:4 + sz])
        if checksum and orc.xxh32(payload) != int(np.frombuffer(rec[4 + sz:8 + sz].tobytes(), dtype=np.uint32)[0]):
            out.append((0, HASH, None)); dead = True; continue
        if word >> 31:
            out.append((sz, OK, payload)); continue
        r, o = orc.decompress_safe_dict(payload, bsz + 8, win) if win.size else orc.decompress_safe(payload, bsz + 8)
        if r < 0:
            out.append((r, CORRUPT, None)); dead = True; continue
        out.append((r, OK, o[:r]))
        win = np.concatenate([win, o[:r]])[-65536:]
    return out, win


def _assert_chain(got, want, wwin, window, wl, tag):
    res, st, outs = got
    for i, (wr, ws, wo) in enumerate(want):
        assert (int(res[i]), int(st[i])) == (wr, ws), (tag, i, int(res[i]), int(st[i]), wr, ws)
        if wo is not None:
            assert np.array_equal(outs[i], wo), (tag, i)
    assert int(wl) == wwin.size and np.array_equal(window[:wwin.size], wwin), tag


@pytest.fixture(scope="module")
def frames(orc):
    """32 blocks of 4 MiB (T / M / Z in turn; M: 64 KiB pieces inside a block, so none is stored) as a linked frame, with a 64 KiB
    dictionary and without."""
    blocks = [np.ascontiguousarray(synth.make("TMZ"[i % 3], BSZ, 1 << 16, seed=700 + i)) for i in range(32)]
    dct = np.ascontiguousarray(synth.text(65536, seed=77))
    out = {}
    for with_dict in (False, True):
        recs = _frame(orc, blocks, BSZ, dct if with_dict else None)
        assert not any(r[3] & 0x80 for r in recs)
        out[with_dict] = recs
    return blocks, dct, out


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_dict", [False, True])
@pytest.mark.parametrize("checksum", [True, False])
@pytest.mark.parametrize("nb", [1, 3, 16, 32])
def test_gpu_dxl_linked_chains(orc, eng, frames, nb, checksum, with_dict):
    blocks, dct, recs_by = frames
    recs = [r if checksum else np.ascontiguousarray(r[:-4]) for r in recs_by[with_dict][:nb]]
    w0, wl0 = _start_window(dct if with_dict else None)
    want, wwin = _walk(orc, recs, BSZ, checksum, w0, wl0)
    assert all(s == OK for _, s, _ in want)
    for split in (None, (nb + 1) // 2) if nb > 1 else (None,):
        window = w0.copy(); wl = wl0
        c0 = eng.counters()
        parts = [recs] if split is None else [recs[:split], recs[split:]]
        res, st, outs = [], [], []
        for part in parts:
            r, s, o, wl = eng.decode_records_ex(part, BSZ, checksum, linked=True, window=window, window_len=wl)
            res += list(r); st += list(s); outs += o
        _assert_chain((res, st, outs), want, wwin, window, wl, (nb, checksum, with_dict, split))
        for b, o in zip(blocks, outs):
            assert np.array_equal(b, o)
        assert eng.counters()["dxl_blocks"] - c0["dxl_blocks"] == nb        # every block is a compressed one: all answered by the few-block path


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------
_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from plz4_amd._native import Engine
z = np.load(sys.argv[2])
n = int(z["n"]); recs = [np.ascontiguousarray(z["r%d" % i]) for i in range(n)]
e = Engine(0)
out = []; meta = []
for lo, hi in json.loads(sys.argv[4]):
    window = z["window"].copy(); wl = int(z["wl"])
    res, st, outs, wl = e.decode_records_ex(recs[lo:hi], 4 << 20, True, linked=True, window=window, window_len=wl)
    meta.append({"res": [int(r) for r in res], "st": [int(s) for s in st], "wl": int(wl)})
    out += outs + [window[:wl]]
np.save(sys.argv[3], np.concatenate(out))
print(json.dumps({"meta": meta, "counters": e.counters()}))
e.close()
"""


def test_gpu_dxl_off_gives_the_same(orc, eng, frames, tmp_path):
    """PLZ4HIP_DX_LINKED=0 (in a child process): the one-wave chain walk -- identical res, st, bytes and window, also for a chain with
    a block that does not decode."""
    blocks, dct, recs_by = frames
    recs = [r.copy() for r in recs_by[True][:16]]
    bad = recs[4].copy(); bad[4 + 2000:4 + 10000] = 0xFF                    # a literal length far beyond the input, behind a recomputed checksum
    sz = int(np.frombuffer(bad[:4].tobytes(), dtype=np.uint32)[0])
    bad[4 + sz:] = np.frombuffer(np.uint32(orc.xxh32(np.ascontiguousarray(bad[4:4 + sz]))).tobytes(), dtype=np.uint8)
    recs.append(bad)                                                        # index 16
    spans = [[0, 3], [0, 16], [3, 5], [14, 17]]
    assert _walk(orc, recs[14:17], BSZ, True, *_start_window(dct))[0][2][1] == CORRUPT
    w0, wl0 = _start_window(dct)
    mine, meta = [], []
    for lo, hi in spans:
        window = w0.copy()
        res, st, outs, wl = eng.decode_records_ex(recs[lo:hi], BSZ, True, linked=True, window=window, window_len=wl0)
        meta.append({"res": [int(r) for r in res], "st": [int(s) for s in st], "wl": int(wl)})
        mine += outs + [window[:wl]]
    np.savez(str(tmp_path / "in.npz"), n=len(recs), window=w0, wl=wl0, **{"r%d" % i: r for i, r in enumerate(recs)})
    env = dict(os.environ, PLZ4HIP_DX_LINKED="0")
    out = str(tmp_path / "off.npy")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(tmp_path / "in.npz"), out, json.dumps(spans)], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got["counters"]["dxl_blocks"] == 0
    assert got["meta"] == meta
    assert np.array_equal(np.load(out), np.concatenate(mine))


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------
def test_gpu_dxl_chains(orc, eng):
    bsz = 1 << 20
    dct = np.ascontiguousarray(synth.text(65536, seed=78))
    chains, windows, wlens = [], [], []
    for k in range(8):
        blocks = [np.ascontiguousarray(synth.make("TMZT"[(k + i) % 4], bsz, 1 << 16, seed=800 + 10 * k + i)) for i in range(4)]
        d = dct if k % 2 else None
        recs = _frame(orc, blocks, bsz, d)
        assert not any(r[3] & 0x80 for r in recs)
        w, wl = _start_window(d)
        chains.append(recs); windows.append(w); wlens.append(wl)
    chains[2][1] = chains[2][1].copy(); chains[2][1][40] ^= 0x55            # chain 2, block 1: checksum mismatch
    bad = chains[5][2].copy(); bad[4 + 2000:4 + 10000] = 0xFF               # chain 5, block 2: a literal length far beyond the input, behind a recomputed checksum
    sz = int(np.frombuffer(bad[:4].tobytes(), dtype=np.uint32)[0])
    bad[4 + sz:] = np.frombuffer(np.uint32(orc.xxh32(np.ascontiguousarray(bad[4:4 + sz]))).tobytes(), dtype=np.uint8)
    chains[5][2] = bad
    wall = np.stack(windows).copy()
    c0 = eng.counters()
    got, wl_out = eng.decode_records_chains(chains, bsz, True, windows=wall, window_lens=np.array(wlens, dtype=np.int32))
    taken = eng.counters()["dxl_blocks"] - c0["dxl_blocks"]
    for k, recs in enumerate(chains):
        want, wwin = _walk(orc, recs, bsz, True, windows[k], wlens[k])
        _assert_chain(got[k], want, wwin, wall[k], wl_out[k], ("chains", k))
        wcopy = windows[k].copy()
        res, st, outs, wl2 = eng.decode_records_ex(recs, bsz, True, linked=True, window=wcopy, window_len=wlens[k])
        _assert_chain((res, st, outs), want, wwin, wcopy, wl2, ("alone", k))
    assert [int(s) for s in got[2][1]] == [OK, HASH, CORRUPT, CORRUPT] and [int(s) for s in got[5][1]] == [OK, OK, CORRUPT, CORRUPT]
    assert taken == 6 * 4 + 1 + 2, taken                                    # six chains in full, the two others up to their bad block


# ---- 9 ---------------------------------------------------------------------------------------------------------------------------
def test_gpu_dxl_independent_blocks_with_dictionary(orc, eng):
    user = synth.text(70000, seed=99)
    big = [np.ascontiguousarray(synth.make("TMZT"[i], BSZ, 1 << 16, seed=900 + i)) for i in range(4)]
    small = [np.ascontiguousarray(synth.text(300000, seed=7)[:n]) for n in (4095, 4096, 4097, 65536, 200000)]
    for dct_user in (user, user[:30000], user[:5]):
        dct_user = np.ascontiguousarray(dct_user)
        dctx = orc.dict_ctx(dct_user); d = eng.dict_create(dct_user)
        dd = np.ascontiguousarray(dct_user[-65536:])
        for srcs in (big, small):
            comps = [np.ascontiguousarray(orc.compress_indie_dict(s, orc.bound(s.size), dctx)[1]) for s in srcs]
            for caps in ([s.size + 8 for s in srcs], [s.size for s in srcs], [s.size - 1 for s in srcs]):
                c0 = eng.counters()
                res, outs = eng.decompress_batch_dict(comps, caps, d)
                for cp, cap, r, o in zip(comps, caps, res, outs):
                    a, da = orc.decompress_safe_dict(cp, cap, dd)
                    assert int(r) == a, (dct_user.size, cp.size, cap, int(r), a)
                    if a >= 0:
                        assert np.array_equal(o[:a], da[:a])
                if srcs is big and caps[0] >= BSZ:
                    assert eng.counters()["dxl_blocks"] - c0["dxl_blocks"] == 4
        # the same blocks as records of a frame with independent blocks
        recs = [_record(orc, 1, np.ascontiguousarray(orc.compress_indie_dict(s, BSZ, dctx)[1]), s, True) for s in big]
        c0 = eng.counters()
        res, st, outs, _ = eng.decode_records_ex(recs, BSZ, True, linked=False, d=d)
        assert not any(st)
        for s, o in zip(big, outs):
            assert np.array_equal(s, o)
        assert eng.counters()["dxl_blocks"] - c0["dxl_blocks"] == 4
        eng.dict_destroy(d)


# ---- 10 --------------------------------------------------------------------------------------------------------------------------
def test_gpu_dxl_content_hash(orc, eng, frames):
    blocks, dct, recs_by = frames
    h = eng.hash_create()
    eng.set_content_hash(h)
    try:
        w, wl = _start_window(dct)
        c0 = eng.counters()
        res, st, outs, wl = eng.decode_records_ex(recs_by[True][:8], BSZ, True, linked=True, window=w, window_len=wl)
        assert not any(st) and eng.counters()["dxl_blocks"] - c0["dxl_blocks"] == 8
        assert eng.hash_sum(h) == orc.xxh32(np.concatenate(blocks[:8]))
    finally:
        eng.set_content_hash(None)
        eng.hash_destroy(h)


# ---- 11 --------------------------------------------------------------------------------------------------------------------------
def test_gpu_dxl_one_ctx_mixed_calls(orc):
    """The few-block decoder's workspace outlives an HC encode with a dictionary / linked blocks on the same ctx, and trim."""
    from plz4_amd._native import Engine
    e = Engine(0)
    bsz = 256 << 10
    dct = np.ascontiguousarray(synth.text(65536, seed=5))
    d = e.dict_create(dct)
    indep_src = [np.ascontiguousarray(synth.text(BSZ, seed=60 + i)) for i in range(3)]
    indep = [orc.block_record(s, BSZ, True) for s in indep_src]
    srcs = [np.ascontiguousarray(synth.make("TMTZ"[i], bsz, 1 << 16, seed=70 + i)) for i in range(4)]
    for _ in range(2):
        c0 = e.counters()
        res, st, outs = e.decode_records(indep, BSZ, True)
        assert not any(st) and all(np.array_equal(o[:int(r)], s) for o, r, s in zip(outs, res, indep_src))
        assert e.counters()["dx_blocks"] - c0["dx_blocks"] == 3
        recs = [np.ascontiguousarray(r) for r in e.encode_records_ex(srcs, bsz, True, linked=True, d=d, level=9)]
        w, wl = _start_window(dct)
        res, st, outs, wl = e.decode_records_ex(recs, bsz, True, linked=True, window=w, window_len=wl)
        assert not any(st)
        for s, o in zip(srcs, outs):
            assert np.array_equal(s, o)
        assert wl == 65536 and np.array_equal(w, np.concatenate(srcs)[-65536:])
        e.trim()
    e.dict_destroy(d)
    e.close()
