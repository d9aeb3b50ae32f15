"""One call of more than 65 535 blocks: the shared case builder of tests/test_many_blocks_cases.py (CPU) and
tests/test_gpu_many_blocks.py (GPU).  N = 257 * 257 tiny blocks cross 2^16 and leave a remainder of 1 against every blocks-per-
workgroup grouping of the launch code (4, 16, 64, 256).  Two forms of the same idea: `ragged` (host-pointer calls: sizes 0..1024)
and `contiguous` (device calls: one buffer cut at BSZ, the last block short).  Every expected value is computed once per process,
by the real liblz4 (oracle/_ref) or the oracle restatement, never by the engine, and cached here.  Test infrastructure.

Layout conventions: ragged plaintext is one buffer + offsets; everything per block that has a bounded size (compressed blocks,
records, decoded blocks) is a 2-D uint8 array, one row ("slot") per block, pre-filled with FILL, so that the engine can be handed
row addresses and the comparison is a few whole-array operations."""
import ctypes as C
import functools

import numpy as np

import corpus
import orclib
from plz4_amd import synth

N = 257 * 257                      # 66 049
BSZ = 1024
SEED = 0x6D62
FILL = 0xA5
RAW_STRIDE = 1056                  # >= LZ4_compressBound(1024) = 1044, and a guard behind it
REC_STRIDE = 1040                  # BSZ + 8 and a guard of 8 (== plz4hip_dev_stage_stride(1024))
KINDS = ("text", "noise", "structured", "zeros")
vp = C.c_void_p


class Rows:
    """Blocks of bounded size, one per row of .a (uint8[N, stride]); .n: the bytes of every row that count (int32[N])."""

    def __init__(self, a, n):
        self.a, self.n = a, np.ascontiguousarray(n, dtype=np.int32)

    def addr(self, col=0):
        return self.a.ctypes.data + col + np.arange(self.a.shape[0], dtype=np.int64) * self.a.shape[1]


class Ragged:
    """Blocks of any size back to back in .buf; block i = buf[off[i]:off[i + 1]]."""

    def __init__(self, buf, sizes):
        self.buf = buf
        self.n = np.ascontiguousarray(sizes, dtype=np.int32)
        self.off = np.zeros(self.n.size + 1, dtype=np.int64); self.off[1:] = np.cumsum(self.n)

    def addr(self):
        return self.buf.ctypes.data + self.off[:-1]

    def block(self, i):
        return self.buf[int(self.off[i]):int(self.off[i + 1])]


def rows(count, stride):
    return np.full((count, stride), FILL, dtype=np.uint8)


def mask(lens, stride):
    """True where column < lens[row]."""
    return np.arange(stride, dtype=np.int32)[None, :] < np.asarray(lens, dtype=np.int32)[:, None]


def first_bad_row(got, want, lens):
    """None when got == want in the first lens[i] bytes of every row i; else the first row that differs (the per-block search
    runs only after the whole-array comparison has failed)."""
    m = mask(np.maximum(lens, 0), got.shape[1])
    if np.array_equal(got[m], want[m]):
        return None
    bad = np.flatnonzero(((got != want) & m).any(axis=1))
    return int(bad[0])


# ---- the inputs

@functools.lru_cache(maxsize=None)
def _pools():
    size = 4 << 20
    return {"text": synth.text(size, seed=SEED), "noise": synth.random_bytes(size, seed=SEED),
            "structured": corpus.structured(size, SEED), "zeros": np.zeros(size, dtype=np.uint8)}


@functools.lru_cache(maxsize=None)
def ragged():
    """Sizes 0..1024: the first 64 are 0..63, the last 64 are 1024..961, every eighth block in between is exactly 1024 bytes (of
    noise: those are the stored records of the host record calls); content rotates over KINDS by block index."""
    rng = np.random.Generator(np.random.PCG64(SEED))
    sizes = rng.integers(0, BSZ + 1, size=N).astype(np.int32)
    idx = np.arange(N)
    sizes[idx % 8 == 5] = BSZ                                           # 5 % 4 == 1: noise
    sizes[:64] = np.arange(64)
    sizes[-64:] = BSZ - np.arange(64)
    case = Ragged(np.empty(int(sizes.sum(dtype=np.int64)) + 64, dtype=np.uint8), sizes)
    case.buf[-64:] = 0
    pools = _pools()
    start = (idx.astype(np.int64) * 1031) % ((4 << 20) - BSZ)
    for k, kind in enumerate(KINDS):
        pool = pools[kind]
        for i in np.flatnonzero((idx % 4 == k) & (sizes > 0)).tolist():
            o = int(case.off[i]); n = int(sizes[i]); s = int(start[i])
            case.buf[o:o + n] = pool[s:s + n]
    return case


STRETCH = 37                        # blocks per stretch of one kind (odd: stretches do not line up with any group of blocks)
LAST = 777                          # the short last block


@functools.lru_cache(maxsize=None)
def contiguous():
    """(N - 1) * BSZ + LAST bytes, the four kinds in stretches of STRETCH blocks: full-size noise blocks become stored records."""
    total = (N - 1) * BSZ + LAST
    buf = np.empty(total, dtype=np.uint8)
    pools = _pools()
    step = STRETCH * BSZ
    for s, o in enumerate(range(0, total, step)):
        n = min(step, total - o)
        p = (s * 100003) % ((4 << 20) - step)
        buf[o:o + n] = pools[KINDS[s % 4]][p:p + n]
    return buf


def contiguous_sizes():
    sizes = np.full(N, BSZ, dtype=np.int32); sizes[-1] = LAST
    return sizes


@functools.lru_cache(maxsize=None)
def contiguous_as_ragged():
    return Ragged(contiguous(), contiguous_sizes())


# ---- the checkers, bound a second time with plain addresses for arguments (66 049 calls per leg: no array wrappers)

@functools.lru_cache(maxsize=None)
def _orc():
    orclib.build_oracle()
    L = C.CDLL(orclib.ORC_SO)
    L.orc_xxh32.restype = C.c_uint32; L.orc_xxh32.argtypes = [vp, C.c_size_t]
    L.orc_compress_bound.restype = C.c_int; L.orc_compress_bound.argtypes = [C.c_int]
    L.orc_decompress_safe.restype = C.c_int; L.orc_decompress_safe.argtypes = [vp, C.c_int, vp, C.c_int]
    L.orc_decompress_safe_dict.restype = C.c_int; L.orc_decompress_safe_dict.argtypes = [vp, C.c_int, vp, C.c_int, vp, C.c_int]
    L.orc_block_record.restype = C.c_int; L.orc_block_record.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp]
    L.orc_stream_init.argtypes = [vp]; L.orc_stream_reset_fast.argtypes = [vp]
    L.orc_stream_load_dict.restype = C.c_int; L.orc_stream_load_dict.argtypes = [vp, vp, C.c_int, C.c_int]
    L.orc_stream_attach.argtypes = [vp, vp]
    L.orc_stream_compress.restype = C.c_int; L.orc_stream_compress.argtypes = [vp, vp, C.c_int, vp, C.c_int]
    return L


@functools.lru_cache(maxsize=None)
def _ref():
    L = C.CDLL(orclib.REF_SO)
    L.LZ4_compress_fast.restype = C.c_int; L.LZ4_compress_fast.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int]
    L.LZ4_compress_HC.restype = C.c_int; L.LZ4_compress_HC.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int]
    L.LZ4_decompress_safe.restype = C.c_int; L.LZ4_decompress_safe.argtypes = [vp, vp, C.c_int, C.c_int]
    L.LZ4_sizeofStateHC.restype = C.c_int
    L.LZ4_resetStreamHC_fast.argtypes = [vp, C.c_int]
    L.LZ4_loadDictHC.restype = C.c_int; L.LZ4_loadDictHC.argtypes = [vp, vp, C.c_int]
    L.LZ4_compress_HC_continue.restype = C.c_int; L.LZ4_compress_HC_continue.argtypes = [vp, vp, vp, C.c_int, C.c_int]
    return L


def bound(n):
    return int(_orc().orc_compress_bound(int(n)))


def _case(form):
    return ragged() if form == "ragged" else contiguous_as_ragged()


# ---- raw blocks: (result int32[N], Rows of what the reference wrote)

@functools.lru_cache(maxsize=None)
def want_raw(level, cap_kind, form="ragged"):
    """LZ4_compress_fast (level 1) / LZ4_compress_HC (levels 2..12) of every block at cap = bound ("bound") or cap = n ("n")."""
    case = _case(form)
    caps = raw_caps(cap_kind, form)
    out = rows(N, RAW_STRIDE)
    res = np.zeros(N, dtype=np.int32)
    L = _ref()
    src, dst, n, cap = case.addr().tolist(), (out.ctypes.data + np.arange(N, dtype=np.int64) * RAW_STRIDE).tolist(), case.n.tolist(), caps.tolist()
    if level == 1:
        f = L.LZ4_compress_fast
        r = [f(src[i], dst[i], n[i], cap[i], 1) for i in range(N)]
    else:
        f = L.LZ4_compress_HC
        r = [f(src[i], dst[i], n[i], cap[i], level) for i in range(N)]
    res[:] = r
    return res, Rows(out, res)


def raw_caps(cap_kind, form="ragged"):
    case = _case(form)
    if cap_kind == "n":
        return case.n.copy()
    table = np.array([bound(n) for n in range(BSZ + 1)], dtype=np.int32)
    return table[case.n]


@functools.lru_cache(maxsize=None)
def damaged_blocks():
    """The reference's level-1 blocks (cap = bound) with every 101st damaged: one flipped byte and one byte cut off the end take
    turns (a block of one byte keeps its length and gets the flip)."""
    res, good = want_raw(1, "bound")
    bad = Rows(good.a.copy(), res.copy())
    for k, i in enumerate(range(0, N, 101)):
        ln = int(bad.n[i])
        if k % 2 == 1 and ln >= 2:
            bad.n[i] = ln - 1
        else:
            bad.a[i, (7 * k) % ln] ^= 1 << (k % 8)
    return bad


def decode_caps(extra):
    """Capacity n + extra of every block; every 97th block n - 1."""
    caps = ragged().n + np.int32(extra)
    caps[::97] = np.maximum(ragged().n[::97] - 1, 0)
    return caps


@functools.lru_cache(maxsize=None)
def want_decode(extra):
    """LZ4_decompress_safe of damaged_blocks() at decode_caps(extra): (codes, Rows of the output where the code is >= 0)."""
    comp = damaged_blocks()
    caps = decode_caps(extra)
    out = rows(N, REC_STRIDE)
    f = _ref().LZ4_decompress_safe
    src, dst, n, cap = comp.addr().tolist(), (out.ctypes.data + np.arange(N, dtype=np.int64) * REC_STRIDE).tolist(), comp.n.tolist(), caps.tolist()
    res = np.array([f(src[i], dst[i], n[i], cap[i]) for i in range(N)], dtype=np.int32)
    return res, Rows(out, np.maximum(res, 0))


@functools.lru_cache(maxsize=None)
def want_xxh32(form="ragged"):
    case = _case(form)
    f = _orc().orc_xxh32
    src, n = case.addr().tolist(), case.n.tolist()
    return np.array([f(src[i], n[i]) for i in range(N)], dtype=np.uint32)


# ---- records (blk.CompressToBlk, blk/blk.go:69-109): Rows of [LE32 size | stored bit][payload][LE32 xxh32(payload)?]

def _frame(out, res, case, checksum):
    """The framing of tests/test_gpu_dict.py::_record around encoder results res whose bytes already lie at column 4 of out."""
    f = _orc().orc_xxh32
    n = case.n
    stored = res == 0
    plen = np.where(stored, n, res).astype(np.int32)
    word = np.where(stored, 0x80000000 | n.astype(np.int64), res.astype(np.int64)).astype(np.uint32)
    src = case.addr().tolist(); dst = (out.ctypes.data + 4 + np.arange(N, dtype=np.int64) * out.shape[1]).tolist()
    for i in np.flatnonzero(stored & (n > 0)).tolist():
        C.memmove(dst[i], src[i], int(n[i]))
    out[:, 0:4] = word.view(np.uint8).reshape(N, 4)
    if checksum:
        pl = plen.tolist()
        x = np.array([f(dst[i], pl[i]) for i in range(N)], dtype=np.uint32)
        out[np.arange(N)[:, None], (4 + plen)[:, None] + np.arange(4)[None, :]] = x.view(np.uint8).reshape(N, 4)
    return Rows(out, plen + 4 + (4 if checksum else 0))


@functools.lru_cache(maxsize=None)
def want_records(level, form="ragged", checksum=True):
    """Records at BSZ: level 1 orc_block_record, levels 2..12 LZ4_compress_HC at cap = BSZ in the framing above."""
    case = _case(form)
    out = rows(N, REC_STRIDE)
    src, n = case.addr().tolist(), case.n.tolist()
    if level == 1:
        f = _orc().orc_block_record
        dst = (out.ctypes.data + np.arange(N, dtype=np.int64) * REC_STRIDE).tolist()
        ln = np.array([f(src[i], n[i], BSZ, int(checksum), dst[i]) for i in range(N)], dtype=np.int32)
        return Rows(out, ln)
    f = _ref().LZ4_compress_HC
    dst = (out.ctypes.data + 4 + np.arange(N, dtype=np.int64) * REC_STRIDE).tolist()
    res = np.array([f(src[i], dst[i], n[i], BSZ, level) for i in range(N)], dtype=np.int32)
    return _frame(out, res, case, checksum)


def body_of(recs):
    """The records back to back (the frame's block section) and their offsets (int64[N + 1])."""
    off = np.zeros(recs.n.size + 1, dtype=np.int64); off[1:] = np.cumsum(recs.n)
    return recs.a[mask(recs.n, recs.a.shape[1])], off


def stored_share(recs):
    return float((recs.a[:, 3] & 0x80).astype(bool).mean())


def plaintext_rows(form="ragged"):
    """The plaintext, one block per row of REC_STRIDE bytes."""
    case = _case(form)
    out = rows(N, REC_STRIDE)
    out[mask(case.n, REC_STRIDE)] = case.buf[:int(case.off[-1])]
    return Rows(out, case.n)


@functools.lru_cache(maxsize=None)
def damaged_records(checksum):
    """The level-1 records of the ragged blocks with every 89th damaged, three ways in turn: 0 a payload byte under block
    checksums (hash mismatch), 1 the size word raised to BSZ + 9 (size overflow), 2 a payload byte without block checksums
    (whatever liblz4 makes of it).  Way 0 is applied in the records with checksums only, way 2 in those without, way 1 in both.
    Returns (records, result, status, Rows of the plaintext each record decodes to) -- derived as tests/test_gpu_parity.py does:
    status 1 and result 0, status 2 and result 0, and LZ4_decompress_safe's code into BSZ + 8 bytes (status 3 when negative)."""
    good = want_records(1, "ragged", True)
    recs = Rows(good.a.copy(), good.n.copy())
    if not checksum:
        recs.n -= 4                                                       # (the checksum's four bytes are not part of the record)
    plain = plaintext_rows("ragged")
    out = Rows(plain.a.copy(), plain.n.copy())
    res = ragged().n.copy(); st = np.zeros(N, dtype=np.int32)
    f = _ref().LZ4_decompress_safe
    for k, i in enumerate(range(0, N, 89)):
        way = k % 3
        plen = int(recs.n[i]) - 4 - (4 if checksum else 0)
        word = int(recs.a[i, 0:4].view("<u4")[0])
        if way == 1:
            recs.a[i, 0:4] = np.frombuffer(np.uint32(BSZ + 9).tobytes(), dtype=np.uint8)
            res[i], st[i] = 0, 2
        elif way == 0 and checksum:
            recs.a[i, 4 + (5 * k) % plen] ^= 1 << (k % 8)
            res[i], st[i] = 0, 1
        elif way == 2 and not checksum:
            recs.a[i, 4 + (5 * k) % plen] ^= 1 << (k % 8)
            if word & 0x80000000:
                out.a[i, :plen] = recs.a[i, 4:4 + plen]                   # a stored block is copied as it is
            else:
                r = int(f(recs.a[i, 4:].ctypes.data, out.a[i].ctypes.data, plen, BSZ + 8))
                res[i] = r; st[i] = 0 if r >= 0 else 3
    out.n = np.maximum(res, 0).astype(np.int32)
    return recs, res, st, out


def content_hash(out, res):
    """xxh32 of the blocks with result > 0 in block order (what a content-hash stream attached to the call must hold)."""
    keep = np.where(res > 0, out.n, 0)
    data = np.ascontiguousarray(out.a[mask(keep, out.a.shape[1])])
    return int(_orc().orc_xxh32(data.ctypes.data, data.size))


# ---- history outside the block, contiguous form

def _stream_buf(size):
    buf = C.create_string_buffer(size + 64)
    return buf, (C.addressof(buf) + 63) & ~63


@functools.lru_cache(maxsize=None)
def want_linked_records(level):
    """WithBlockLinked over the contiguous form, no dictionary: block i > 0 primed with block i - 1 (its last <= 64 KiB, here all of
    it), held in memory of its own as the reference's writer holds it.  Level 1: the oracle's stream emulation (orc.compress_linked);
    levels 2..12: liblz4's HC stream driven as tests/hcdict.py::ref_records drives it."""
    case = contiguous_as_ragged()
    out = rows(N, REC_STRIDE)
    src, n = case.addr().tolist(), case.n.tolist()
    dst = (out.ctypes.data + 4 + np.arange(N, dtype=np.int64) * REC_STRIDE).tolist()
    tail = np.zeros(BSZ + 64, dtype=np.uint8); ta = tail.ctypes.data
    r = [0] * N
    if level == 1:
        L = _orc()
        keep, s = _stream_buf(C.sizeof(orclib.OrcStream))
        init, reset, load, comp = L.orc_stream_init, L.orc_stream_reset_fast, L.orc_stream_load_dict, L.orc_stream_compress
        for i in range(N):
            init(s); reset(s)
            if i:
                C.memmove(ta, src[i - 1], n[i - 1]); load(s, ta, n[i - 1], 0)
            r[i] = comp(s, src[i], n[i], dst[i], BSZ)
    else:
        L = _ref()
        keep, s = _stream_buf(L.LZ4_sizeofStateHC())
        L.LZ4_resetStreamHC_fast(s, level)
        load, comp = L.LZ4_loadDictHC, L.LZ4_compress_HC_continue
        for i in range(N):
            if i:
                C.memmove(ta, src[i - 1], n[i - 1]); load(s, ta, n[i - 1])
            r[i] = comp(s, src[i], dst[i], n[i], BSZ)
    del keep
    return _frame(out, np.array(r, dtype=np.int32), case, True)


@functools.lru_cache(maxsize=None)
def dictionary():
    return np.ascontiguousarray(synth.text(70000, seed=SEED + 1))


@functools.lru_cache(maxsize=None)
def want_dict_records():
    """Every block of the contiguous form on its own under dictionary(), level 1 (orc.compress_indie_dict), as records with block
    checksums; and what orc.decompress_safe_dict makes of every payload against the dictionary's last 64 KiB: (records, result,
    Rows of plaintext)."""
    case = contiguous_as_ragged()
    L = _orc()
    dct = dictionary()
    dctx = orclib.Oracle().dict_ctx(dct)
    keep, s = _stream_buf(C.sizeof(orclib.OrcStream))
    out = rows(N, REC_STRIDE)
    src, n = case.addr().tolist(), case.n.tolist()
    dst = (out.ctypes.data + 4 + np.arange(N, dtype=np.int64) * REC_STRIDE).tolist()
    init, reset, attach, comp = L.orc_stream_init, L.orc_stream_reset_fast, L.orc_stream_attach, L.orc_stream_compress
    da = C.addressof(dctx)
    r = [0] * N
    for i in range(N):
        init(s); reset(s); attach(s, da)
        r[i] = comp(s, src[i], n[i], dst[i], BSZ)
    res = np.array(r, dtype=np.int32)
    recs = _frame(out, res, case, True)
    d64 = np.ascontiguousarray(dct[-65536:])
    plain = rows(N, REC_STRIDE)
    pa = (plain.ctypes.data + np.arange(N, dtype=np.int64) * REC_STRIDE).tolist()
    f = L.orc_decompress_safe_dict
    dec = np.zeros(N, dtype=np.int32)
    for i in range(N):
        if r[i] == 0:
            C.memmove(pa[i], src[i], n[i]); dec[i] = n[i]
        else:
            dec[i] = f(dst[i], r[i], pa[i], BSZ + 8, d64.ctypes.data, d64.size)
    del keep
    return recs, dec, Rows(plain, np.maximum(dec, 0))
