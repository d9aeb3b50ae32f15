"""Linked decode calls cut into groups of blocks: the cases tests/test_dxl_groups.py (lane-emulated, tests/emu/emu_dxl_groups.cpp) and
tests/test_gpu_dxl_groups.py (through the C ABI) share, the reference reader they are checked against, and the ctypes loader of the
emulation.  Test infrastructure only."""
import ctypes as C
import os
import subprocess

import numpy as np

from orclib import ROOT
from plz4_amd import synth

SRC = os.path.join(ROOT, "tests", "emu", "emu_dxl_groups.cpp")
SO = os.path.join(ROOT, "tests", "emu", "_build", "libemu_dxl_groups.so")
DEPS = [SRC] + [os.path.join(ROOT, "plz4_amd", "csrc", f) for f in ("lz4_dx_device.inl", "lz4_device.inl", "wave.h")]
i32p = C.POINTER(C.c_int32)
u8p = C.POINTER(C.c_uint8)

OK, HASH, SIZE, CORRUPT = 0, 1, 2, 3
BSZ = 64 << 10


class DxlGroupsEmu:
    def __init__(self):
        newest = max(os.path.getmtime(p) for p in DEPS)
        if not os.path.exists(SO) or os.path.getmtime(SO) < newest:
            os.makedirs(os.path.dirname(SO), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-parameter", "-o", SO, SRC])
        L = self.L = C.CDLL(SO)
        L.emu_dxlg_decode.restype = C.c_int
        L.emu_dxlg_decode.argtypes = [C.c_int, C.POINTER(C.c_void_p), i32p, C.c_int, C.c_int, C.c_int, i32p, u8p, i32p,
                                      C.c_int, i32p, u8p, C.c_int64, C.c_int, i32p, i32p, i32p, C.POINTER(C.c_int64)]

    def set_descending(self, d):
        self.L.emu_dxlg_set_descending(int(d))

    def decode(self, case):
        """-> (per chain (res, st, outs)), windows (nCh x 65536), window lengths, {"taken", "rounds", "groups"}, taken per block"""
        recs = [np.ascontiguousarray(r) for ch in case.chains for r in ch]
        nb, nch = len(recs), len(case.chains)
        first = np.zeros(nch + 1, np.int32)
        for k, ch in enumerate(case.chains):
            first[k + 1] = first[k] + len(ch)
        ptrs = (C.c_void_p * nb)(*[r.ctypes.data for r in recs])
        ln = np.array([r.size for r in recs], np.int32)
        win = np.zeros((nch, 131072), np.uint8); win[:, :65536] = case.windows
        wl = np.array(case.wlens, np.int32)
        cap = case.bsz + 8
        stride = (cap + 64 + 15) // 16 * 16
        dst = np.zeros(nb * stride + 64, np.uint8)
        res = np.zeros(nb, np.int32); st = np.zeros(nb, np.int32); taken = np.zeros(nb, np.int32)
        cnt = (C.c_int64 * 3)()
        ip = lambda a: a.ctypes.data_as(i32p)
        forced = None if case.forced is None else np.array(case.forced, np.int32)
        rc = self.L.emu_dxlg_decode(nb, ptrs, ip(ln), case.bsz, int(case.checksum), nch, ip(first), win.ctypes.data_as(u8p), ip(wl),
                                    case.group, ip(forced) if forced is not None else None, dst.ctypes.data_as(u8p), stride, cap,
                                    ip(res), ip(st), ip(taken), cnt)
        assert rc == 0, rc
        outs = [dst[i * stride:i * stride + max(int(res[i]), 0)].copy() for i in range(nb)]
        got = []
        for k in range(nch):
            a, b = int(first[k]), int(first[k + 1])
            got.append((res[a:b], st[a:b], outs[a:b]))
        return got, win[:, :65536].copy(), wl, {"taken": int(cnt[0]), "rounds": int(cnt[1]), "groups": int(cnt[2])}, taken


# ---- the reference side ---------------------------------------------------------------------------------------------------------
def start_window(dct):
    """compress/dict.go:43-56: a frame's window starts as the dictionary's last 64 KiB."""
    w = np.zeros(65536, dtype=np.uint8)
    wl = 0 if dct is None else min(dct.size, 65536)
    if wl:
        w[:wl] = dct[-wl:]
    return w, wl


def record(orc, comp_ret, comp, src, checksum):
    """blk.CompressToBlk framing of one encoder result (blk.go:78-109)."""
    if comp_ret == 0:
        payload, word = src, 0x80000000 | src.size
    else:
        payload, word = comp, comp.size
    rec = np.uint32(word).tobytes() + payload.tobytes()
    if checksum:
        rec += np.uint32(orc.xxh32(np.ascontiguousarray(payload))).tobytes()
    return np.frombuffer(rec, dtype=np.uint8).copy()


def frame(orc, blocks, bsz, dct, checksum=True):
    """A linked frame's records (StreamLinkedCtx block by block)."""
    dctx = orc.dict_ctx(dct) if dct is not None else None
    recs, prev = [], None
    for b in blocks:
        tail = None if prev is None else prev[-65536:].copy()
        r, c = orc.compress_linked(b, bsz, tail, dctx if prev is None else None)
        recs.append(record(orc, r, c[:r], b, checksum)); prev = b
    return recs


def is_stored(rec):
    return bool(rec[3] & 0x80)


def rehash(orc, rec):
    """the record with its block checksum made to match its payload again"""
    rec = rec.copy()
    sz = int(np.frombuffer(rec[:4].tobytes(), dtype=np.uint32)[0]) & 0x7FFFFFFF
    rec[4 + sz:8 + sz] = np.frombuffer(np.uint32(orc.xxh32(np.ascontiguousarray(rec[4:4 + sz]))).tobytes(), dtype=np.uint8)
    return rec


def walk(orc, recs, bsz, checksum, window, wl):
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


class Case:
    """One call: chains of records, the windows it comes in with, the group size.  want: per chain the reference reader's blocks and
    window.  taken: the compressed blocks the few-block path must answer (the case's counter) -- every compressed block in front of
    its chain's first block that is not OK, less those of the groups in `walked` (forced: jump rounds per group, emulation only)."""

    def __init__(self, orc, name, chains, dicts, group, bsz=BSZ, checksum=True, forced=None, walked=()):
        self.name, self.chains, self.group, self.bsz, self.checksum, self.forced = name, chains, group, bsz, checksum, forced
        ws = [start_window(d) for d in dicts]
        self.windows = np.stack([w for w, _ in ws]); self.wlens = [wl for _, wl in ws]
        self.want = [walk(orc, ch, bsz, checksum, w, wl) for ch, (w, wl) in zip(chains, ws)]
        self.taken, k = 0, 0
        for ch, (blocks, _) in zip(chains, self.want):
            for rec, (_, st, _) in zip(ch, blocks):
                if st == OK and not is_stored(rec) and (k // group) not in walked:
                    self.taken += 1
                k += 1

    def check(self, got, windows, wlens):
        for k, ((res, st, outs), (blocks, wwin)) in enumerate(zip(got, self.want)):
            for i, (wr, ws, wo) in enumerate(blocks):
                assert (int(res[i]), int(st[i])) == (wr, ws), (self.name, k, i, int(res[i]), int(st[i]), wr, ws)
                if wo is not None:
                    assert np.array_equal(outs[i][:wr], wo), (self.name, k, i)
            assert int(wlens[k]) == wwin.size and np.array_equal(windows[k][:wwin.size], wwin), (self.name, k, "window")


def _blocks(kind, n, size, seed):
    return [np.ascontiguousarray(synth.make(kind, size, 1 << 14, seed=seed + i)) for i in range(n)]


def _past_history(orc, rec, hist_len):
    """the first sequence's offset one byte past the history (hist_len bytes in front of the block), behind a matching checksum"""
    bad = rec.copy()
    ll = int(bad[4]) >> 4
    off = ll + hist_len + 1
    assert ll != 15 and 1 <= off <= 65535, (ll, hist_len)
    bad[5 + ll] = off & 255; bad[6 + ll] = off >> 8
    return rehash(orc, bad)


def build_cases(orc):
    user = np.ascontiguousarray(synth.text(70000, seed=42))
    cases = []
    # chains of 9 blocks of 64 KiB, a dictionary of 70 000 / 5 bytes and none, at group sizes 1, 2, 4 and 9
    for d, dlen in enumerate((70000, 5, None)):
        dct = None if dlen is None else np.ascontiguousarray(user[:dlen])
        recs = frame(orc, _blocks("TMZ"[d], 9, BSZ, 100 + 10 * d), BSZ, dct)
        assert not any(is_stored(r) for r in recs)
        for g in (1, 2, 4, 9):
            cases.append(Case(orc, "nine-d%s-g%d" % (dlen, g), [recs], [dct], g))
    # blocks of 20 000 .. 50 000 bytes: the 64 KiB in front of a block span several predecessors, across a group border
    rng = np.random.default_rng(5)
    sizes = [int(rng.integers(20000, 50001)) for _ in range(9)]
    text = synth.text(sum(sizes), seed=7)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    small = [np.ascontiguousarray(text[offs[i]:offs[i + 1]]) for i in range(9)]
    for dlen in (30000, None):
        dct = None if dlen is None else np.ascontiguousarray(user[:dlen])
        recs = frame(orc, small, BSZ, dct)
        assert not any(is_stored(r) for r in recs)
        cases.append(Case(orc, "span-d%s-g2" % dlen, [recs], [dct], 2))
        cases.append(Case(orc, "span-d%s-g4-nochecksum" % dlen, [[np.ascontiguousarray(r[:-4]) for r in recs]], [dct], 4, checksum=False))
    # a stored block as the last block of a group (3 of [0, 4)) and as the first of the next (4)
    for at in (3, 4):
        blocks = _blocks("T", 9, BSZ, 300)
        blocks[at] = np.ascontiguousarray(synth.random_bytes(BSZ, seed=9))
        recs = frame(orc, blocks, BSZ, user)
        assert [is_stored(r) for r in recs] == [i == at for i in range(9)]
        cases.append(Case(orc, "stored-at%d" % at, [recs], [user], 4))
    # three chains of 5 / 1 / 6 blocks at group size 4
    dicts = [user, None, np.ascontiguousarray(user[:5])]
    chains = [frame(orc, _blocks("TZM"[k], n, BSZ, 400 + 10 * k), BSZ, dicts[k]) for k, n in enumerate((5, 1, 6))]
    assert not any(is_stored(r) for ch in chains for r in ch)
    cases.append(Case(orc, "chains-5-1-6", chains, dicts, 4))
    # damage in the last block of a group (1 of [0, 2)) and in the first of the next (2): chain 0 of two; 7 blocks of 20 000 bytes,
    # so the history in front of the damaged block is 20 000 / 40 000 bytes and an offset can reach past it
    plain = [np.ascontiguousarray(text[i * 20000:(i + 1) * 20000]) for i in range(7)]
    good = frame(orc, plain, BSZ, None)
    other = frame(orc, _blocks("T", 5, BSZ, 500), BSZ, user)
    assert not any(is_stored(r) for r in good + other)
    for at in (1, 2):
        a = good[at].copy(); a[-1] ^= 0x40                                   # a wrong block checksum
        b = good[at].copy(); sz = b.size - 8; b[4 + sz // 4:4 + sz // 2] = 0xFF; b = rehash(orc, b)   # a damaged payload behind a matching checksum
        c = _past_history(orc, good[at], at * 20000)
        for tag, bad in (("hash", a), ("payload", b), ("offset", c)):
            ch = list(good); ch[at] = bad
            case = Case(orc, "bad-%s-at%d" % (tag, at), [ch, other], [None, user], 2)
            sts = [s for _, s, _ in case.want[0][0]]
            assert sts[:at] == [OK] * at and sts[at] == (HASH if tag == "hash" else CORRUPT) and sts[at + 1:] == [CORRUPT] * (6 - at), (tag, at, sts)
            assert all(s == OK for _, s, _ in case.want[1][0])
            assert case.taken == at + 5
            cases.append(case)
    return cases


def flagged_case(orc):
    """Emulation only: group 1 of three is given one jump round -- its blocks are valid but have not come to rest, so the path does
    not answer for them: that group goes through the walk, the next is back on the path."""
    user = np.ascontiguousarray(synth.text(70000, seed=42))
    recs = frame(orc, _blocks("T", 9, BSZ, 600), BSZ, user)
    assert not any(is_stored(r) for r in recs)
    return Case(orc, "flagged-group1", [recs], [user], 3, forced=[0, 1, 0], walked=(1,))
