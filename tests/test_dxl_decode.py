"""The few-block decoder for blocks with history outside the block (dxl_* in plz4_amd/csrc/lz4_dx_device.inl: linked chains and
independent blocks under a dictionary, one pointer space per call) on the lane-emulated build of the same source
(tests/emu/emu_dxl.cpp): every block's result and bytes and the window a chain hands back must be those of a sequential walk with
the oracle's LZ4_decompress_safe_usingDict under the reference reader's window rule (compress/dict.go:28-41; stored blocks do not
enter the window, sync/reader.go:75-78), whichever of the two paths -- the few-block one or the one-wave walk behind it -- answers."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import corpus
from orclib import ROOT, _ptr, u8p
from plz4_amd import synth

SRC = os.path.join(ROOT, "tests", "emu", "emu_dxl.cpp")
SO = os.path.join(ROOT, "tests", "emu", "_build", "libemu_dxl.so")
DEPS = [SRC] + [os.path.join(ROOT, "plz4_amd", "csrc", f) for f in ("lz4_dx_device.inl", "lz4_device.inl", "wave.h")]
i32p = C.POINTER(C.c_int32)


class DxlEmu:
    def __init__(self):
        newest = max(os.path.getmtime(p) for p in DEPS)
        if not os.path.exists(SO) or os.path.getmtime(SO) < newest:
            os.makedirs(os.path.dirname(SO), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-parameter", "-o", SO, SRC])
        L = self.L = C.CDLL(SO)
        L.emu_dxl_decode.restype = C.c_int
        L.emu_dxl_decode.argtypes = [C.c_int, C.POINTER(C.c_void_p), i32p, i32p, i32p, i32p, i32p, C.c_int, u8p, i32p, C.c_int,
                                     u8p, C.c_int64, i32p, i32p, i32p, C.POINTER(C.c_int), C.c_int]

    def decode(self, chains, caps, windows, wlens, linked=True, rounds_forced=0):
        """chains: a list of chains, each a list of (payload, stored); caps: per block, in order; windows: nCh x 65536 (linked: updated in
        place; not linked: one row, the dictionary's last 64 KiB), wlens: int32 per row (updated).  Returns res, st, taken, outs, rounds."""
        blocks = [b for ch in chains for b in ch]
        nb = len(blocks)
        first, chain = [], []
        k = 0
        for c, ch in enumerate(chains):
            for _ in ch:
                first.append(k if linked else len(first)); chain.append(c if linked else 0)
            k += len(ch)
        keep = [np.ascontiguousarray(p) for p, _ in blocks]
        ptrs = (C.c_void_p * nb)(*[a.ctypes.data for a in keep])
        ln = np.array([a.size for a in keep], dtype=np.int32)
        stored = np.array([int(s) for _, s in blocks], dtype=np.int32)
        cap = np.array(caps, dtype=np.int32)
        stride = (int(cap.max()) + 64 + 15) // 16 * 16
        dst = np.zeros(nb * stride + 64, dtype=np.uint8)
        res = np.zeros(nb, np.int32); st = np.zeros(nb, np.int32); taken = np.zeros(nb, np.int32)
        rounds = C.c_int(0)
        ip = lambda a: a.ctypes.data_as(i32p)
        rc = self.L.emu_dxl_decode(nb, ptrs, ip(ln), ip(stored), ip(cap), ip(np.array(first, np.int32)), ip(np.array(chain, np.int32)),
                                   windows.shape[0], _ptr(windows), ip(wlens), int(linked), _ptr(dst), stride, ip(res), ip(st), ip(taken),
                                   C.byref(rounds), rounds_forced)
        assert rc == 0, rc                                                  # (-888888: the units of a block disagree about where they meet)
        outs = [dst[i * stride:i * stride + max(int(res[i]), 0)].copy() for i in range(nb)]
        return res, st, taken, outs, rounds.value


@pytest.fixture(scope="module")
def dxl():
    return DxlEmu()


# ---- the reference side -------------------------------------------------------------------------------------------------------
def _start_window(dct):
    """compress/dict.go:43-56: a frame's window starts as the dictionary's last 64 KiB."""
    w = np.zeros(65536, dtype=np.uint8)
    wl = 0 if dct is None else min(dct.size, 65536)
    if wl:
        w[:wl] = dct[-wl:]
    return w, wl


def _linked_frame(orc, data, bsz, dct=None, sizes=None):
    """StreamLinkedCtx block by block -> [(payload, stored)], the source blocks."""
    if sizes is None:
        sizes = [min(bsz, data.size - o) for o in range(0, data.size, bsz)]
    dctx = orc.dict_ctx(dct) if dct is not None else None
    blocks, srcs, prev, o = [], [], None, 0
    for n in sizes:
        b = np.ascontiguousarray(data[o:o + n]); o += n
        tail = None if prev is None else prev[-65536:].copy()
        r, c = orc.compress_linked(b, bsz, tail, dctx if prev is None else None)
        blocks.append((b.copy(), True) if r == 0 else (np.ascontiguousarray(c[:r]).copy(), False))
        srcs.append(b); prev = b
    return blocks, srcs


def _walk(orc, blocks, caps, window, wl):
    """The sequential reader: per block (result, status, bytes); the window afterwards."""
    win = window[:wl].copy()
    out, dead = [], False
    for (payload, stored), cap in zip(blocks, caps):
        if dead:
            out.append((0, 1, None)); continue
        if stored:
            out.append((payload.size, 0, payload)); continue
        r, o = orc.decompress_safe_dict(payload, cap, win) if win.size else orc.decompress_safe(payload, cap)
        if r < 0:
            out.append((r, 1, None)); dead = True; continue
        out.append((r, 0, o[:r]))
        win = np.concatenate([win, o[:r]])[-65536:]
    return out, win


def _check_chain(orc, dxl, blocks, bsz, dct, split=None, expect_plain=None):
    """One call, or two with the window carried.  Returns (compressed blocks the path took, compressed blocks)."""
    caps = [bsz + 8] * len(blocks)
    w0, wl0 = _start_window(dct)
    want, wwin = _walk(orc, blocks, caps, w0, wl0)
    windows = w0.reshape(1, 65536).copy(); wlens = np.array([wl0], dtype=np.int32)
    parts = [blocks] if not split else [blocks[:split], blocks[split:]]
    res, st, taken, outs = [], [], [], []
    for part in parts:
        r, s, t, o, _ = dxl.decode([part], [bsz + 8] * len(part), windows, wlens)
        res += list(r); st += list(s); taken += list(t); outs += o
    for i, (wr, ws, wo) in enumerate(want):
        assert (int(res[i]), int(st[i])) == (wr, ws), (i, int(res[i]), int(st[i]), wr, ws)
        if wo is not None:
            assert np.array_equal(outs[i], wo), i
            if expect_plain is not None and not ws:
                assert np.array_equal(outs[i], expect_plain[i]), i
    assert int(wlens[0]) == wwin.size and np.array_equal(windows[0][:wwin.size], wwin)
    comp = [i for i, (_, s) in enumerate(blocks) if not s]
    return sum(int(taken[i]) for i in comp), len(comp)


DICTS = {None: None, 70000: 70000, 30000: 30000, 5: 5}


def _data(kind, n, bsz, seed):
    return corpus.structured(n, seed) if kind == "S" else synth.make(kind, n, bsz, seed=seed)


# ---- 1. linked frames ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bsz", [64 << 10, 256 << 10])
def test_emu_dxl_linked_frames_small_blocks(orc, dxl, bsz):
    user = synth.text(70000, seed=42)
    taken = total = 0
    for k, kind in enumerate(("T", "M", "Z", "S")):
        for d, dlen in enumerate((None, 70000, 30000, 5)):
            dct = None if dlen is None else np.ascontiguousarray(user[:dlen])
            data = _data(kind, 5 * bsz + 777, bsz, seed=10 * k + d)
            blocks, srcs = _linked_frame(orc, data, bsz, dct)
            plain = srcs if not any(s for _, s in blocks) else None       # (a stored block garbles what refers to it: the walk is the yardstick)
            t, n = _check_chain(orc, dxl, blocks, bsz, dct, expect_plain=plain); taken += t; total += n
            t, n = _check_chain(orc, dxl, blocks, bsz, dct, split=2 + d % 3); taken += t; total += n
    assert taken > total // 2, (taken, total)


@pytest.mark.parametrize("kind", ["T", "M", "Z", "S"])
def test_emu_dxl_linked_frames_1mib(orc, dxl, kind):
    bsz = 1 << 20
    user = synth.text(70000, seed=43)
    for d, dlen in enumerate((None, 70000, 5)):
        dct = None if dlen is None else np.ascontiguousarray(user[:dlen])
        data = _data(kind, 3 * bsz + 4321, 1 << 16, seed=50 + d)          # (M: 64 KiB pieces inside the block, as in test_dx_decode)
        blocks, srcs = _linked_frame(orc, data, bsz, dct)
        assert not any(s for _, s in blocks)
        t, n = _check_chain(orc, dxl, blocks, bsz, dct, expect_plain=srcs)
        if kind != "S":
            assert t == n, (kind, dlen, t, n)                               # none left to the hand-over
        t, n = _check_chain(orc, dxl, blocks, bsz, dct, split=1, expect_plain=srcs)
        if kind != "S":
            assert t == n, (kind, dlen, t, n)


@pytest.mark.parametrize("kind", ["T", "M", "Z"])
def test_emu_dxl_linked_frame_3x4mib(orc, dxl, kind):
    bsz = 4 << 20
    dct = np.ascontiguousarray(synth.text(70000, seed=44))
    data = _data(kind, 3 * bsz, 1 << 16, seed=60)
    blocks, srcs = _linked_frame(orc, data, bsz, dct)
    assert not any(s for _, s in blocks)
    t, n = _check_chain(orc, dxl, blocks, bsz, dct, expect_plain=srcs)
    assert t == n == 3, (kind, t, n)
    t, n = _check_chain(orc, dxl, blocks, bsz, dct, split=2, expect_plain=srcs)
    assert t == n == 3, (kind, t, n)


# ---- 2. history over several predecessors; a stored block in the middle ---------------------------------------------------------
def test_emu_dxl_history_spans_several_blocks(orc, dxl):
    bsz = 64 << 10
    rng = np.random.default_rng(5)
    taken = total = 0
    for seed, dlen in ((1, None), (2, 30000), (3, 5), (4, 70000)):
        sizes = [int(rng.integers(20000, 50001)) for _ in range(9)]
        base = synth.text(60000, seed=seed)
        data = np.concatenate([base, base[::-1].copy(), base])[:sum(sizes)] if seed % 2 else corpus.structured(sum(sizes), seed)
        if data.size < sum(sizes):
            data = np.resize(data, sum(sizes))
        dct = None if dlen is None else np.ascontiguousarray(synth.text(70000, seed=9)[:dlen])
        blocks, srcs = _linked_frame(orc, data, bsz, dct, sizes=sizes)
        plain = srcs if not any(s for _, s in blocks) else None
        t, n = _check_chain(orc, dxl, blocks, bsz, dct, expect_plain=plain); taken += t; total += n
        t, n = _check_chain(orc, dxl, blocks, bsz, dct, split=4); taken += t; total += n
    assert taken > total // 2, (taken, total)


def test_emu_dxl_stored_block_stays_out_of_the_window(orc, dxl):
    """The successor of a stored block refers to the stored bytes; the reference's reader decodes it against the OLD window and
    garbles it (test_gpu_linked_decode_follows_reference_window_rule): that is the expected result."""
    bsz = 64 << 10
    a = synth.text(bsz, seed=1); r_ = synth.random_bytes(bsz, seed=2); b = np.concatenate([r_[-30000:], synth.text(bsz - 30000, seed=3)])
    blocks, srcs = _linked_frame(orc, np.concatenate([a, r_, b, synth.text(bsz, seed=4)]), bsz)
    assert blocks[1][1] and not blocks[2][1]
    t, n = _check_chain(orc, dxl, blocks, bsz, None)
    want, _ = _walk(orc, blocks, [bsz + 8] * 4, np.zeros(65536, np.uint8), 0)
    assert want[2][0] < 0 or not np.array_equal(want[2][2], b)             # the reference does not give the plaintext back here
    _check_chain(orc, dxl, blocks, bsz, None, split=2)


# ---- 3. independent blocks under a dictionary ------------------------------------------------------------------------------------
def test_emu_dxl_independent_blocks_with_dictionary(orc, dxl):
    user = synth.text(70000, seed=99)
    data = synth.text(1 << 20, seed=7)
    taken = total = 0
    for dct_user in (user, user[:30000], user[:5]):
        dct_user = np.ascontiguousarray(dct_user)
        dctx = orc.dict_ctx(dct_user)
        srcs = [np.ascontiguousarray(data[:n]) for n in (4095, 4096, 4097, 65536, 200000, 1 << 20)] + [corpus.structured(150000, 3)]
        comps = [np.ascontiguousarray(orc.compress_indie_dict(s, orc.bound(s.size), dctx)[1]) for s in srcs]
        dd, dl = _start_window(dct_user)
        for caps in ([s.size + 8 for s in srcs], [s.size for s in srcs], [s.size - 1 for s in srcs]):
            res, st, tk, outs, _ = dxl.decode([[(c, False)] for c in comps], caps, dd.reshape(1, 65536).copy(), np.array([dl], np.int32), linked=False)
            for i, (cp, cap) in enumerate(zip(comps, caps)):
                a, da = orc.decompress_safe_dict(cp, cap, dd[:dl])
                assert int(res[i]) == a, (dct_user.size, cp.size, cap, int(res[i]), a)
                if a >= 0:
                    assert np.array_equal(outs[i], da[:a])
                if srcs[i].size == 1 << 20 and cap >= srcs[i].size:
                    assert tk[i] == 1
            taken += int(tk.sum()); total += len(comps)
    assert taken > total // 2, (taken, total)


# ---- 4. corruption -----------------------------------------------------------------------------------------------------------------
def _damage(rng, payload, k, hist_len):
    bad = payload.copy()
    if k == 0:
        return bad[:int(rng.integers(1, bad.size))]
    if k == 1:
        i = int(rng.integers(0, bad.size)); bad[i] ^= 1 << int(rng.integers(0, 8))
    elif k == 2:
        i = int(rng.integers(0, bad.size)); bad[i] = 0xFF
    elif k == 3:
        i = int(rng.integers(0, bad.size - 1)); bad[i:i + 2] = 0
    else:
        # the first sequence's offset reaches the history's first byte (k == 4: accepted) or one byte past it (k == 5)
        ll = int(bad[0]) >> 4
        off = ll + hist_len + (k - 4)
        if ll == 15 or off > 65535 or off < 1:
            i = int(rng.integers(0, bad.size)); bad[i] ^= 0x10
        else:
            bad[1 + ll] = off & 255; bad[2 + ll] = off >> 8
    return bad


def test_emu_dxl_corrupt_chains(orc, dxl):
    bsz = 64 << 10
    rng = np.random.default_rng(17)
    cases = answered = 0
    for seed, dlen in enumerate((None, 5, 30000, 70000, 3000, None)):
        dct = None if dlen is None else np.ascontiguousarray(synth.text(70000, seed=77)[:dlen])
        sizes = [bsz] * 5 if seed % 2 else [int(rng.integers(9000, 40000)) for _ in range(5)]
        data = synth.text(sum(sizes), seed=seed + 1) if seed % 3 else corpus.structured(sum(sizes), seed + 700)
        blocks, _ = _linked_frame(orc, data, bsz, dct, sizes=sizes)
        w0, wl0 = _start_window(dct)
        caps = [bsz + 8] * 5
        for trial in range(36):
            at = trial % 5
            if blocks[at][1]:
                continue
            hist = min(65536, wl0 + sum(s for s, (_, st_) in zip(sizes[:at], blocks[:at]) if not st_))
            bad = list(blocks)
            bad[at] = (np.ascontiguousarray(_damage(rng, blocks[at][0], trial % 6, hist)), False)
            want, wwin = _walk(orc, bad, caps, w0, wl0)
            windows = w0.reshape(1, 65536).copy(); wlens = np.array([wl0], dtype=np.int32)
            res, st, taken, outs, _ = dxl.decode([bad], caps, windows, wlens)
            for i, (wr, ws, wo) in enumerate(want):
                assert (int(res[i]), int(st[i])) == (wr, ws), (seed, trial, i, int(res[i]), int(st[i]), wr, ws)
                if wo is not None:
                    assert np.array_equal(outs[i], wo), (seed, trial, i)
            assert int(wlens[0]) == wwin.size and np.array_equal(windows[0][:wwin.size], wwin), (seed, trial)
            cases += 1; answered += int(taken[at])
    assert cases >= 200, cases
    assert answered > 50, (answered, cases)


def test_emu_dxl_a_chain_that_has_not_converged_is_not_answered(orc, dxl):
    """Too few jump rounds for the copy chain: the blocks are left to the one-wave walk, whose bytes are right."""
    bsz = 256 << 10
    blocks, srcs = _linked_frame(orc, np.zeros(3 * bsz, np.uint8), bsz)
    windows = np.zeros((1, 65536), np.uint8); wlens = np.zeros(1, np.int32)
    res, st, taken, outs, _ = dxl.decode([blocks], [bsz + 8] * 3, windows, wlens, rounds_forced=6)
    assert not taken.any() and not st.any()
    for o, s in zip(outs, srcs):
        assert np.array_equal(o, s)
    assert int(wlens[0]) == 65536 and not windows[0].any()


# ---- 5. depth --------------------------------------------------------------------------------------------------------------------
def test_emu_dxl_deepest_copy_chain_of_a_frame(orc, dxl):
    """8 linked blocks of 4 MiB of one byte value: every byte points at the one before it, across the blocks' borders -- a copy chain
    as long as the call's output, which 24 rounds do not resolve."""
    bsz = 4 << 20
    data = np.full(8 * bsz, 0x5A, dtype=np.uint8)
    blocks, srcs = _linked_frame(orc, data, bsz)
    assert not any(s for _, s in blocks)
    windows = np.zeros((1, 65536), np.uint8); wlens = np.zeros(1, np.int32)
    res, st, taken, outs, rounds = dxl.decode([blocks], [bsz + 8] * 8, windows, wlens)
    assert taken.all() and not st.any()
    for r, o in zip(res, outs):
        assert int(r) == bsz and o.size == bsz and (o == 0x5A).all()
    assert int(wlens[0]) == 65536 and (windows[0] == 0x5A).all()
    assert 22 < rounds <= math.ceil(math.log2(8 * bsz)) + 1, rounds
