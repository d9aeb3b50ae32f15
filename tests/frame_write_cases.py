"""The frame writer (plz4hip_dev_write_frames) for the CPU and the GPU tests: a model written from the table of rules in
include/plz4hip.h and from nothing else -- the oracle supplies the reference's header bytes, xxh32 and block records -- and the list of
cases.  Test infrastructure only."""
from __future__ import annotations

import functools

import numpy as np

import body_index_cases as bic
import stream_index_cases as sic

OK, NO_ROOM, RECORD = range(3)
CANARY = 0xC7
K64 = 64 << 10
GAP = K64 + 65536

INFO_FIELDS = ("end", "nFrames", "nRecs", "status", "firstBadRec")
INFO_DTYPE = np.dtype([("end", "<i8"), ("nFrames", "<i4"), ("nRecs", "<i4"), ("status", "<i4"), ("firstBadRec", "<i4"), ("reserved", "<i4", (2,))])
OPTS_FIELDS = ("bsz", "blockChecksum", "linked", "contentChecksum", "contentSize", "hasDictId", "dictId", "reserved")
assert INFO_DTYPE.itemsize == 32


def info_of(raw):
    assert not raw["reserved"].any(), "info.reserved is not 0"
    return {k: int(raw[k]) for k in INFO_FIELDS}


def wrap64(v: int) -> int:
    """two's complement: what 64-bit arithmetic makes of a table that holds anything"""
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def opts(bck=False, cck=False, csize=False, dict_id=None, linked=False, bsz=K64):
    return dict(bsz=bsz, blockChecksum=int(bck), linked=int(linked), contentChecksum=int(cck), contentSize=int(csize),
                hasDictId=int(dict_id is not None), dictId=int(dict_id or 0), reserved=0)


def opts_words(o) -> np.ndarray:
    return np.array([o[k] for k in OPTS_FIELDS], dtype=np.uint32).view(np.int32)


class Case:
    """One call.  src: the array `src` points into (block i at i * stride); body / rec_off: what the encoder left; out_cap: None for
    exactly the stream's length.  body_bytes may say more than body holds where the rules keep the call from reading it."""

    def __init__(self, name, o, src, src_bytes, stride, body, rec_off, k, out_cap=None, body_bytes=None, waves=1 << 20, slices=1):
        self.name, self.opts, self.src, self.src_bytes, self.stride = name, o, np.ascontiguousarray(src, dtype=np.uint8), int(src_bytes), int(stride)
        self.body = np.ascontiguousarray(body, dtype=np.uint8)
        self.body_bytes = self.body.size if body_bytes is None else int(body_bytes)
        self.rec_off = np.ascontiguousarray(rec_off, dtype=np.int64)
        self.k, self.waves, self.slices = int(k), waves, slices
        g = geometry(self)
        assert self.rec_off.size == g["n"] + 1
        self.out_cap = g["nf"] * (g["H"] + g["T"]) + (int(self.rec_off[g["n"]]) if g["n"] else 0) if out_cap is None else int(out_cap)

    def block(self, i):
        bsz = self.opts["bsz"]
        return self.src[i * self.stride:i * self.stride + min(bsz, self.src_bytes - i * bsz)]

    def plaintext(self, first=0, last=None):
        n = geometry(self)["n"]
        parts = [self.block(i) for i in range(first, n if last is None else last)]
        return np.concatenate(parts) if parts else np.zeros(0, np.uint8)


def geometry(c):
    o = c.opts
    bsz = o["bsz"]
    n = (c.src_bytes + bsz - 1) // bsz
    k = c.k or max(n, 1)
    return dict(n=n, k=k, nf=max(1, (n + k - 1) // k), H=7 + 8 * o["contentSize"] + 4 * o["hasDictId"], T=4 + 4 * o["contentChecksum"],
                flg=0x40 | (0 if o["linked"] else 0x20) | o["blockChecksum"] << 4 | o["contentSize"] << 3 | o["contentChecksum"] << 2 | o["hasDictId"],
                bd={K64: 4, 256 << 10: 5, 1 << 20: 6, 4 << 20: 7}[bsz] << 4)


def model(orc, c):
    """-> dict(info, frames, out_rec_off, stream, start): frames and out_rec_off None where the call writes neither (NO_ROOM); stream:
    the bytes out[start .. E) must hold, None unless the status is OK"""
    o, g = c.opts, geometry(c)
    n, k, nf, H, T = g["n"], g["k"], g["nf"], g["H"], g["T"]
    bsz, bck = o["bsz"], o["blockChecksum"]
    off = [int(v) for v in c.rec_off]
    tail = off[n] if n else 0
    if not 0 <= tail <= c.body_bytes:
        end, room = -1, RECORD
    else:
        end = nf * (H + T) + tail
        room = NO_ROOM if end > c.out_cap else OK
    if room == NO_ROOM:
        return dict(info=dict(end=end, nFrames=nf, nRecs=n, status=NO_ROOM, firstBadRec=-1), frames=None, out_rec_off=None, stream=None, start=0)

    def is_bad(i):
        a, b = off[i], off[i + 1]
        if a < 0 or b < a or b > c.body_bytes:
            return True
        if b - a < 4 + 4 * bck:
            return True
        size = int.from_bytes(bytes(c.body[a:a + 4]), "little") & 0x7FFFFFFF
        return size > bsz or 4 + size + 4 * bck != b - a

    frames, first_bad, parts = [], -1, []
    for f in range(nf):
        first, last = f * k, min((f + 1) * k, n)
        bad = next((i for i in range(first, last) if is_bad(i)), -1)
        if bad >= 0 and first_bad < 0:
            first_bad = bad
        plain = min(c.src_bytes, last * bsz) - first * bsz
        frm, to = (off[first], off[last]) if n else (0, 0)
        hdr_off = wrap64(f * (H + T) + frm)
        total = orc.xxh32(c.plaintext(first, last)) if o["contentChecksum"] and bad < 0 else 0
        frames.append(dict(hdrOff=hdr_off, bodyOff=wrap64(hdr_off + H), end=wrap64((f + 1) * (H + T) + to), contentSz=plain if o["contentSize"] else 0,
                           dictId=o["dictId"] if o["hasDictId"] else 0, contentSum=total, firstRec=first, nRecs=last - first, bsz=bsz,
                           flags=g["flg"], blockDesc=g["bd"], kind=0, nibble=0, status=bic.END_MARK if bad < 0 else -1 - bad, reserved=0))
        if first_bad < 0:
            parts += [sic.u8(orc.frame_header(g["bd"] >> 4, linked=bool(o["linked"]), block_checksum=bool(bck), content_checksum=bool(o["contentChecksum"]),
                                              content_size=plain if o["contentSize"] else None, dict_id=o["dictId"] if o["hasDictId"] else None)),
                      c.body[frm:to], bic.le32(0)] + ([bic.le32(total)] if o["contentChecksum"] else [])
    out_rec_off = np.array([wrap64(off[i] + (i // k + 1) * H + (i // k) * T) for i in range(n)] +
                           [wrap64(off[n] + nf * H + (nf - 1) * T) if n else 0], dtype=np.int64)
    status = RECORD if first_bad >= 0 or room == RECORD else OK
    stream = np.concatenate(parts) if status == OK else None
    start = off[0] if n else 0                                  # (recOff[0] need not be 0: the stream then starts at out + recOff[0])
    assert stream is None or start + stream.size == end
    return dict(info=dict(end=end, nFrames=nf, nRecs=n, status=status, firstBadRec=first_bad), frames=frames, out_rec_off=out_rec_off, stream=stream,
                start=start)


# ------------------------------------------------------------------------------------------------------------ pieces
N_SHARED = 49


@functools.lru_cache(maxsize=None)
def shared_plaintext() -> np.ndarray:
    """49 blocks of text, the second one incompressible: its record is a stored one"""
    from plz4_amd import synth
    data = synth.text(N_SHARED * K64, seed=77)
    data[K64:2 * K64] = synth.random_bytes(K64, seed=78)
    data.setflags(write=False)
    return data


class Records:
    """the oracle's record of every block of a prefix of the shared plaintext, computed once per (block, length, block checksum)"""

    def __init__(self, orc):
        self.orc, self.memo = orc, {}

    def record(self, i, length, bck):
        key = (i, length, bool(bck))
        if key not in self.memo:
            self.memo[key] = self.orc.block_record(np.array(shared_plaintext()[i * K64:i * K64 + length]), K64, bool(bck)).copy()
        return self.memo[key]

    def body(self, src_bytes, bck, base=0):
        """-> (body with `base` bytes of noise in front, recOff)"""
        n = (src_bytes + K64 - 1) // K64
        recs = [self.record(i, min(K64, src_bytes - i * K64), bck) for i in range(n)]
        off = np.cumsum([base] + [r.size for r in recs]).astype(np.int64)
        return np.concatenate([np.full(base, 0xB7, np.uint8)] + recs), off


def laid_out(src_bytes, stride):
    """the first src_bytes of the shared plaintext, block i at i * stride, 0xEE in the gaps"""
    data = shared_plaintext()
    if stride == K64:
        return np.array(data[:src_bytes])
    n = (src_bytes + K64 - 1) // K64
    buf = np.full((n - 1) * stride + (src_bytes - (n - 1) * K64) if n else 0, 0xEE, np.uint8)
    for i in range(n):
        blk = data[i * K64:min((i + 1) * K64, src_bytes)]
        buf[i * stride:i * stride + blk.size] = blk
    return buf


def good_case(recs, name, o, src_bytes, k, stride=K64, base=0, **kw):
    body, off = recs.body(src_bytes, o["blockChecksum"], base)
    return Case(name, o, laid_out(src_bytes, stride), src_bytes, stride, body, off, k, **kw)


def cases(orc):
    """-> (the cases every status of which is OK, the failure cases)"""
    recs = Records(orc)
    good, bad = [], []
    # 1. option bits: every combination; H in {7, 11, 15, 19}, T in {4, 8}; linked goes with one frame only
    for linked in (False, True):
        for j in range(16):
            bck, cck, cs, did = bool(j & 1), bool(j & 2), bool(j & 4), bool(j & 8)
            o = opts(bck, cck, cs, 0xA1B2C3D4 + j if did else None, linked)
            good.append(good_case(recs, "options %d%s" % (j, ", linked" if linked else ""), o, 3 * K64 - 100 - j, 0 if linked else 2))
    # 2. frame sizes, both strides
    full = opts(True, True, True)
    for k in (0, 1, 2, 3):
        for n in sorted({0, 1, max(k - 1, 0), k, k + 1, 2 * k + 1}):
            for stride in (K64, GAP, GAP + 24):
                if n or stride == K64:
                    good.append(good_case(recs, "k %d, %d blocks, stride %d" % (k, n, stride), full, max(n * K64 - 333, 0), k, stride,
                                          base=5 if n == k else 0, slices=1 + n % 3))
    # 3. frame counts on grids of 1 - 3 waves; H + T = 15: every misalignment of a move among the first sixteen frames
    sums = opts(False, True)
    for nf, waves in ((15, 1), (16, 1), (17, 1), (17, 2), (33, 2), (33, 3), (49, 3), (49, 1)):
        good.append(good_case(recs, "%d frames, %d waves" % (nf, waves), sums, nf * K64 - 4099, 1, waves=waves))
    good.append(good_case(recs, "17 frames of 2, 2 waves", full, 33 * K64 + 1, 2, waves=2))
    # 4. last blocks, and frames whose whole plaintext is below a stripe
    for t in (1, 15, 16, 17):
        good.append(good_case(recs, "%d bytes" % t, sums, t, 0))
        good.append(good_case(recs, "two blocks and %d bytes, k 1" % t, full, 2 * K64 + t, 1))
        good.append(good_case(recs, "two blocks and %d bytes, k 2" % t, sums, 2 * K64 + t, 2, stride=GAP))
        good.append(good_case(recs, "two blocks and %d bytes, k 0" % t, full, 2 * K64 + t, 0))
    # 5. room: exactly enough is enough
    c = good_case(recs, "room to spare", full, 5 * K64 - 9, 2)
    c.out_cap += 100
    good.append(c)

    # ---- failures
    src_bytes = 5 * K64 - 9
    def base_case(name, o=full, k=2, **kw):
        return good_case(recs, name, o, src_bytes, k, **kw)
    def mutated(name, fn, **kw):
        c = base_case(name, **kw)
        c.body, c.rec_off = c.body.copy(), c.rec_off.copy()
        fn(c)
        bad.append(c)
    def drop(c, *which):                                        # a block the engine failed on: its record takes no room
        lens = np.diff(c.rec_off)
        keep = [c.body[c.rec_off[i]:c.rec_off[i + 1]] for i in range(lens.size) if i not in which]
        for i in which:
            lens[i] = 0
        c.rec_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        c.body = np.concatenate(keep)
        c.body_bytes = c.body.size
        c.out_cap += 100
    def word(c, i, w):
        c.body[c.rec_off[i]:c.rec_off[i] + 4] = bic.le32(w)
    mutated("record 2 takes no room", lambda c: drop(c, 2))
    mutated("records 1 and 3 take no room", lambda c: drop(c, 3, 1))
    mutated("record 0 takes no room, one frame", lambda c: drop(c, 0), k=0)
    mutated("record 4 takes no room, k 1", lambda c: drop(c, 4), k=1)
    mutated("size word above bsz", lambda c: word(c, 1, K64 + 1))
    mutated("stored size word above bsz", lambda c: word(c, 1, 0x80000000 | (K64 + 1)))
    mutated("size word of 0xFFFFFFFF in record 3, of 0 in record 4", lambda c: (word(c, 4, 0), word(c, 3, 0xFFFFFFFF)))
    mutated("size word one short", lambda c: word(c, 2, int.from_bytes(bytes(c.body[c.rec_off[2]:c.rec_off[2] + 4]), "little") - 1))
    c = base_case("block checksums assumed but absent", o=opts(False, True, True))
    c.opts = full
    bad.append(c)
    c = base_case("block checksums present, not assumed")
    c.opts = opts(False, True, True)
    bad.append(c)
    def cut(c, by):
        c.body_bytes = int(c.rec_off[-1]) - by
        c.body = c.body[:c.body_bytes]
    mutated("the body overflowed its cap by one byte", lambda c: cut(c, 1))
    mutated("the body overflowed its cap by two records", lambda c: cut(c, int(c.rec_off[5] - c.rec_off[3]) + 1), k=1)
    def put(c, i, v):
        c.rec_off[i] = v
    mutated("a negative offset", lambda c: put(c, 2, -5))
    mutated("a first offset of -1", lambda c: put(c, 0, -1))
    mutated("an offset that steps back", lambda c: put(c, 3, int(c.rec_off[2]) - 1), k=1)
    mutated("an offset of 2^62", lambda c: put(c, 1, 1 << 62), k=1)
    mutated("a last offset of -2^63", lambda c: put(c, 5, -(1 << 63)))
    mutated("a last offset of 2^63 - 1", lambda c: put(c, 5, (1 << 63) - 1), k=0)
    mutated("offsets that step back beyond the last", lambda c: (put(c, 2, int(c.rec_off[5]) + 7), put(c, 3, int(c.rec_off[5]) + 9)), k=1)
    # no room
    for cap in (lambda e: e - 1, lambda e: 0, lambda e: e // 2):
        c = base_case("no room")
        c.out_cap = cap(c.out_cap)
        c.name = "no room: %d" % c.out_cap
        bad.append(c)
    c = good_case(recs, "no room for the empty frame", full, 0, 0)
    c.out_cap -= 1
    bad.append(c)
    # offsets above 2^32 and a tiny outCap: the exact end, and no byte of the body (there is none) is read
    c = base_case("a base above 2^32", o=opts(True, False, True), k=1)
    c.rec_off = c.rec_off + ((1 << 32) + 12345)
    c.body_bytes = int(c.rec_off[-1])
    c.body = np.zeros(1, np.uint8)
    c.out_cap = 1000
    bad.append(c)
    return good, bad
