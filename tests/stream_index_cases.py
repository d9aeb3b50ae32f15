"""The stream index (plz4hip_dev_index_stream) for the CPU and the GPU tests: a model of the reader's header-mode / body-mode walk,
written from the table of steps in include/plz4hip.h and from nothing else, the pieces streams are built from, and the list of cases.
Test infrastructure only."""
from __future__ import annotations

import numpy as np

import body_index_cases as bic

(END, FRAMES_FULL, RECORDS_FULL, HEADER_READ, MAGIC, VERSION, RESERVED_BIT, BLOCK_DESCRIPTOR, HEADER_HASH, SKIP, BODY,
 CONTENT_HASH_READ) = range(12)

FRAME_FIELDS = ("hdrOff", "bodyOff", "end", "contentSz", "dictId", "contentSum", "firstRec", "nRecs", "bsz", "flags", "blockDesc", "kind",
                "nibble", "status", "reserved")
INFO_FIELDS = ("end", "nFrames", "nRecs", "status", "nSkippable", "maxBsz", "flagsAnd", "flagsOr")
FRAME_DTYPE = np.dtype([("hdrOff", "<i8"), ("bodyOff", "<i8"), ("end", "<i8"), ("contentSz", "<u8"), ("dictId", "<u4"), ("contentSum", "<u4"),
                        ("firstRec", "<i4"), ("nRecs", "<i4"), ("bsz", "<i4"), ("flags", "u1"), ("blockDesc", "u1"), ("kind", "u1"),
                        ("nibble", "u1"), ("status", "<i4"), ("reserved", "<i4")])
INFO_DTYPE = np.dtype([("end", "<i8"), ("nFrames", "<i4"), ("nRecs", "<i4"), ("status", "<i4"), ("nSkippable", "<i4"), ("maxBsz", "<i4"),
                       ("flagsAnd", "u1"), ("flagsOr", "u1"), ("pad", "u1", (2,))])
assert FRAME_DTYPE.itemsize == 64 and INFO_DTYPE.itemsize == 32

M32 = 0xFFFFFFFF


def xxh32_short(b: bytes) -> int:
    """xxh32, seed 0, of fewer than 16 bytes"""
    assert len(b) < 16
    rotl = lambda x, r: ((x << r) | (x >> (32 - r))) & M32
    h = (374761393 + len(b)) & M32
    k = 0
    while k + 4 <= len(b):
        h = (rotl((h + int.from_bytes(b[k:k + 4], "little") * 3266489917) & M32, 17) * 668265263) & M32
        k += 4
    for c in b[k:]:
        h = (rotl((h + c * 374761393) & M32, 11) * 2654435761) & M32
    h ^= h >> 15; h = (h * 2246822519) & M32
    h ^= h >> 13; h = (h * 3266489917) & M32
    return h ^ (h >> 16)


def reader_of(buf: np.ndarray):
    """read(off, n) -> the n bytes at off of a uint8 array"""
    return lambda off, n: bytes(buf[off:off + n])


def model(read, n_bytes: int, max_frames: int, max_recs: int):
    """-> (frames: list of dicts with FRAME_FIELDS, recOff[0 .. max_recs] as int64, info: dict with INFO_FIELDS).
    read(off, n) is asked only for bytes inside [0, n_bytes)."""
    def get(off, n):
        assert 0 <= off and off + n <= n_bytes, "the model itself reads outside the stream"
        return read(off, n)

    off, frames, listed, rec_end = 0, [], [], 0
    n_skip, max_bsz, f_and, f_or = 0, 0, 0xFF, 0
    while True:
        end = off
        if off == n_bytes:
            status = END; break
        if len(frames) == max_frames:
            status = FRAMES_FULL; break
        left = n_bytes - off
        if left < 7:
            status = HEADER_READ; break
        magic = int.from_bytes(get(off, 4), "little")
        if 0x184D2A50 <= magic <= 0x184D2A5F:
            if left < 8:
                status = HEADER_READ; break
            size = int.from_bytes(get(off + 4, 4), "little")
            if size > left - 8:
                status = SKIP; break
            frames.append(dict(hdrOff=off, bodyOff=off + 8, end=off + 8 + size, contentSz=size, dictId=0, contentSum=0, firstRec=len(listed),
                               nRecs=0, bsz=0, flags=0, blockDesc=0, kind=1, nibble=magic & 15, status=bic.END_MARK, reserved=0))
            n_skip += 1
            off += 8 + size
            continue
        if magic != 0x184D2204:
            status = MAGIC; break
        flg, bd = get(off + 4, 2)
        if flg >> 6 != 1:
            status = VERSION; break
        if flg & 2:
            status = RESERVED_BIT; break
        if ((bd >> 4) & 7) < 4 or bd & 0x80 or bd & 0x0F:
            status = BLOCK_DESCRIPTOR; break
        hlen = 7 + (8 if flg & 8 else 0) + (4 if flg & 1 else 0)
        if hlen > left:
            status = HEADER_READ; break
        hdr = get(off, hlen)
        if hdr[hlen - 1] != (xxh32_short(hdr[4:hlen - 1]) >> 8) & 0xFF:
            status = HEADER_HASH; break
        bsz = (64 << 10) << 2 * (((bd >> 4) & 7) - 4)
        f = dict(hdrOff=off, bodyOff=off + hlen, end=0, contentSz=int.from_bytes(hdr[6:14], "little") if flg & 8 else 0,
                 dictId=int.from_bytes(hdr[hlen - 5:hlen - 1], "little") if flg & 1 else 0, contentSum=0, firstRec=len(listed), nRecs=0,
                 bsz=bsz, flags=flg, blockDesc=bd, kind=0, nibble=0, status=0, reserved=0)
        frames.append(f)
        f_and &= flg; f_or |= flg; max_bsz = max(max_bsz, bsz)
        # the body walk: the table of plz4hip_dev_index_body, off == nBytes being a truncated word
        off += hlen
        while True:
            end = off
            if n_bytes - off < 4:
                body = bic.TRUNCATED_WORD; break
            word = int.from_bytes(get(off, 4), "little")
            if word == 0:
                body = bic.END_MARK; end = off + 4; break
            if len(listed) == max_recs:
                body = bic.FULL; break
            size = word & 0x7FFFFFFF
            if size > bsz:
                body = bic.SIZE_OVERFLOW; break
            need = 4 + size + (4 if flg & 16 else 0)
            if need > n_bytes - off:
                body = bic.TRUNCATED_BLOCK; break
            listed.append(off)
            off += need; rec_end = off
        f["nRecs"] = len(listed) - f["firstRec"]; f["status"] = body; f["end"] = end
        if body == bic.FULL:
            status = RECORDS_FULL; break
        if body != bic.END_MARK:
            status = BODY; break
        if flg & 4:
            if n_bytes - end < 4:
                status = CONTENT_HASH_READ; break
            f["contentSum"] = int.from_bytes(get(end, 4), "little")
            end += 4; f["end"] = end
        off = end
    lz4 = len(frames) - n_skip
    info = dict(end=end, nFrames=len(frames), nRecs=len(listed), status=status, nSkippable=n_skip, maxBsz=max_bsz,
                flagsAnd=f_and if lz4 else 0, flagsOr=f_or)
    rec_off = np.array(listed + [rec_end] * (max_recs + 1 - len(listed)), dtype=np.int64)
    return frames, rec_off, info


def frames_of(raw: np.ndarray, n: int):
    """the first n entries of a table of FRAME_DTYPE as the model's dicts"""
    return [{k: int(raw[j][k]) for k in FRAME_FIELDS} for j in range(n)]


def info_of(raw: np.ndarray):
    assert not raw["pad"].any(), "info.pad is not 0"
    return {k: int(raw[k]) for k in INFO_FIELDS}


# ------------------------------------------------------------------------------------------------------------ pieces
def u8(b) -> np.ndarray:
    return np.frombuffer(bytes(b), dtype=np.uint8)


def skippable(nibble: int, payload: int, declared: int | None = None, seed: int = 3) -> np.ndarray:
    """a skippable frame: magic 0x184D2A50 | nibble, LE32 size (`declared` if it is to lie), `payload` bytes of 0x01..0xFF noise"""
    rng = np.random.default_rng(seed + payload)
    return np.concatenate([bic.le32(0x184D2A50 | nibble), bic.le32(payload if declared is None else declared),
                           rng.integers(1, 256, size=payload, dtype=np.uint8)])


def made_frame(orc, n_recs: int, bs_idx: int = 4, linked: bool = False, bck: bool = False, cck: bool = False, content_size=None,
               dict_id=None, seed: int = 1, end_mark: bool = True) -> np.ndarray:
    """the oracle's header, then n_recs records of hand-made size words over noise (body_index_cases.build_body), the end mark, and
    four bytes of noise as the content checksum if the header asks for one"""
    hdr = u8(orc.frame_header(bs_idx, linked=linked, block_checksum=bck, content_checksum=cck, content_size=content_size, dict_id=dict_id))
    sizes, stored = bic.record_sizes(n_recs, 1024, seed)
    body, _ = bic.build_body(sizes, stored, bck, end_mark, 4 if (cck and end_mark) else 0, seed=seed)
    return np.concatenate([hdr, body])


FLG_COMBOS = [(linked, bck, cck, cs, did) for linked in (False, True) for bck in (False, True) for cck in (False, True)
              for cs in (False, True) for did in (False, True)]


def header_len(cs, did):
    return 7 + (8 if cs else 0) + (4 if did else 0)


def combo_frame(orc, k: int, combo, bs_idx: int, n_recs: int = 2) -> np.ndarray:
    linked, bck, cck, cs, did = combo
    return made_frame(orc, n_recs, bs_idx, linked, bck, cck, 0x0102030405060708 + k if cs else None, 0xA1B2C3D4 + k if did else None, seed=40 + k)


def rehash(frame: np.ndarray, hlen: int) -> np.ndarray:
    """the header's hash byte set to what its descriptor bytes now hash to"""
    frame[hlen - 1] = (xxh32_short(bytes(frame[4:hlen - 1])) >> 8) & 0xFF
    return frame


def oracle_frames(orc):
    """real frames from the oracle's writer over a few KiB: every pair of checksum options at 64 KiB blocks, and one each with a
    content size and a dictionary id in the header (orc.frame_header in front of the same block section).
    -> [(frame, plaintext bytes, reader options)]"""
    from plz4_amd import synth
    out = []
    for k, (bck, cck) in enumerate(((False, False), (True, False), (False, True), (True, True))):
        data = synth.make("M", 3000 + 700 * k, 64 << 10)
        out.append((orc.frame_encode(data, 4, bck, cck).copy(), data, {}))
    data = synth.make("T", 5000, 64 << 10)
    plain = orc.frame_encode(data, 4, True, True)
    for cs, did in ((data.size, None), (None, 77), (data.size, 0xFFFFFFFF)):
        hdr = u8(orc.frame_header(4, block_checksum=True, content_checksum=True, content_size=cs, dict_id=did))
        out.append((np.concatenate([hdr, plain[7:]]), data, {}))
    return out


# ------------------------------------------------------------------------------------------------------------ the cases
class Case:
    """name, the stream, the table sizes to run it with (None: room for everything), decodable: every LZ4 frame in it is a real
    one from the oracle's writer, so the host layer's Reader can be driven over the same bytes"""

    def __init__(self, name, stream, sizes=None, decodable=False):
        self.name, self.stream, self.sizes, self.decodable = name, np.ascontiguousarray(stream, dtype=np.uint8), sizes, decodable


def cat(*parts):
    parts = [p for p in parts if p.size]
    return np.concatenate(parts) if parts else np.zeros(0, np.uint8)


def cases(orc):
    out = []
    add = lambda *a, **kw: out.append(Case(*a, **kw))
    real = oracle_frames(orc)
    R = [f for f, _, _ in real]
    lead = R[3]                                                 # a real frame in front: the header under test is not at offset 0

    # 1. headers: all four BD ids x every FLG combination in one stream; each alone; every truncation of each header
    every = [combo_frame(orc, k, c, 4 + (k + j) % 4) for j in range(4) for k, c in enumerate(FLG_COMBOS)]
    add("all 128 headers", cat(*every))
    for k, c in enumerate(FLG_COMBOS):
        f = combo_frame(orc, k, c, 4 + k % 4)
        hlen = header_len(c[3], c[4])
        for cut in range(1, hlen + 1):                          # (cut == hlen: the whole header and no size word)
            add("header %d cut to %d" % (k, cut), cat(lead, f[:cut]))
        add("header %d alone, cut to %d" % (k, hlen - 1), f[:hlen - 1])

    # 2. bad headers, on the shortest and the longest header
    for k in (0, 31):
        c = FLG_COMBOS[k]
        hlen = header_len(c[3], c[4])
        good = combo_frame(orc, k, c, 5)
        def bad(name, at, value, fix=True):
            f = good.copy(); f[at] = value
            if fix:
                rehash(f, hlen)
            add("%s (header %d)" % (name, hlen), cat(lead, f, R[0]))
        for j, m in enumerate((0x184D2203, 0x184D2205, 0x184D2A60, 0x184D2A4F, 0x04224D19, 0)):
            f = good.copy(); f[:4] = bic.le32(m)
            add("magic %08x (header %d)" % (m, hlen), cat(lead, f))
        flg, bd = int(good[4]), int(good[5])
        for v in (0, 2, 3):
            bad("version %d" % v, 4, (flg & 0x3F) | v << 6)
            bad("version %d, stale hash" % v, 4, (flg & 0x3F) | v << 6, fix=False)
        bad("reserved bit", 4, flg | 2)
        for i in range(4):
            bad("BD id %d" % i, 5, i << 4)
        bad("BD bit 7", 5, bd | 0x80)
        for bit in range(4):
            bad("BD low nibble bit %d" % bit, 5, bd | 1 << bit)
        # the order of the checks: the first one in the table wins
        f = good.copy(); f[4] = (flg & 0x3F) | 2; f[5] = 0x8F
        add("version, reserved bit and BD at once (header %d)" % hlen, cat(lead, f))
        f = good.copy(); f[4] = flg | 2; f[5] = 0x00
        add("reserved bit and BD at once (header %d)" % hlen, cat(lead, f))
        f = good.copy(); f[5] = 0x30
        add("bad BD in a cut header (header %d)" % hlen, cat(lead, f[:7]))
        for v in range(256):
            if v != int(good[hlen - 1]):
                f = good.copy(); f[hlen - 1] = v
                add("hash byte %02x (header %d)" % (v, hlen), cat(lead, f))
        for at in [4] + list(range(6, hlen - 1)):               # a flipped descriptor bit that passes the sanity checks
            f = good.copy(); f[at] ^= 0x10
            add("descriptor byte %d flipped (header %d)" % (at, hlen), cat(lead, f))

    # 3. skippable frames
    add("16 nibbles, then a frame", cat(*[skippable(n, n * 3) for n in range(16)], R[1]), decodable=True)
    for n in range(16):
        add("nibble %x alone" % n, skippable(n, 5), decodable=True)
    add("skippable of size 0, last", cat(R[0], skippable(3, 0)), decodable=True)
    add("skippable that ends at nBytes", cat(R[0], skippable(4, 9)), decodable=True)
    add("skippable one byte long of its size", cat(R[0], skippable(4, 9, declared=10)), decodable=True)
    add("skippable of 0xFFFFFFFF", cat(R[0], skippable(5, 9, declared=0xFFFFFFFF)), decodable=True)
    add("skippable of 0x80000000", cat(skippable(5, 0, declared=0x80000000)), decodable=True)
    add("skippable, eighth byte missing", cat(R[2], skippable(6, 0)[:7]), decodable=True)
    add("skippable, eighth byte missing, alone", skippable(6, 0)[:7], decodable=True)
    add("skippable in front, between and last", cat(skippable(1, 7), R[0], skippable(2, 0), skippable(15, 300), R[3], skippable(0, 1)), decodable=True)
    add("a frame's magic inside a skippable payload", cat(R[1], skippable(9, 0, declared=R[0].size), R[0], R[2]), decodable=True)

    # 4. real frames back to back, and cut
    add("seven real frames", cat(*R), decodable=True)
    full = cat(R[2], R[3])                                      # the last one: block and content checksums
    for cut in range(1, 13):                                    # 1-4: the trailer; 5-8: the end mark; then the last record
        add("two real frames cut by %d" % cut, full[:full.size - cut], decodable=True)
    nock = cat(R[3], R[1])                                      # no content checksum: 1-4 cut the end mark
    for cut in range(1, 6):
        add("real frame without a trailer cut by %d" % cut, nock[:nock.size - cut], decodable=True)

    # 5. record counts on the edges of the 64-entry store groups, inside a frame and exactly at a frame boundary
    counts = (63, 1, 64, 0, 65, 129, 0, 62)
    mk = lambda order, **kw: [made_frame(orc, n, 4 + j % 4, bck=bool(j & 1), cck=bool(j & 2), seed=70 + j, **kw) for j, n in enumerate(order)]
    groups = cat(*mk(counts))
    n_recs = sum(counts)
    add("frames of 63, 1, 64, 0, 65, 129, 0, 62 records", groups,
        sizes=[(len(counts) + 2, n_recs + 70)] + [(mf, mr) for mf in (len(counts) - 1, len(counts), len(counts) + 1, 0)
                                                  for mr in (n_recs - 1, n_recs, n_recs + 1, 0)])
    add("frames of 64, 64, 1 records", cat(*mk((64, 64, 1))), sizes=[(4, 200), (3, 129), (3, 128), (3, 64), (3, 63), (2, 128), (1, 64)])
    add("frames of 129, 0 records, a skippable one between", cat(mk((129,))[0], skippable(2, 11), mk((0,))[0]),
        sizes=[(5, 140), (3, 129), (3, 128), (2, 129), (1, 129), (0, 0)])
    for n in (0, 1, 63, 64, 65, 129):
        f = made_frame(orc, n, 4, bck=True, cck=True, seed=90 + n)
        add("one frame of %d records" % n, f, sizes=[(1, n), (2, n + 1), (1, max(n - 1, 0)), (1, n + 70), (0, n), (1, 0)])
        add("one frame of %d records, trailer cut" % n, f[:f.size - 2], sizes=[(1, n + 1)])
    # an unterminated last frame: its records end where the bytes end / its last record is cut / its next word lies
    un = made_frame(orc, 5, 4, bck=True, cck=True, seed=17, end_mark=False)
    add("unterminated last frame", cat(R[0], un))
    add("unterminated last frame, last record cut", cat(R[0], un[:un.size - 3]))
    add("unterminated last frame, two bytes of a word", cat(R[0], un, u8(b"\x05\x00")))
    add("a size word above bsz", cat(R[0], un, bic.le32((64 << 10) + 1), np.full(9, 7, np.uint8)))
    add("a size word of 0xFFFFFFFF", cat(R[0], un, bic.le32(0xFFFFFFFF), np.full(9, 7, np.uint8)))
    add("a stored record of exactly bsz", cat(un, bic.le32(0x80000000 | (64 << 10)), np.full((64 << 10) + 4, 9, np.uint8), bic.le32(0), u8(b"abcd")))

    # 6. next to nothing
    add("empty", np.zeros(0, np.uint8), sizes=[(0, 0), (1, 1), (3, 70)], decodable=True)
    for n in range(1, 7):
        add("%d bytes of a frame" % n, R[0][:n], sizes=[(2, 2), (0, 0)], decodable=True)
        add("%d bytes of a skippable frame" % n, skippable(7, 0)[:n], decodable=True)
        add("%d zeros" % n, np.zeros(n, np.uint8), decodable=True)
    add("7 zeros", np.zeros(7, np.uint8), decodable=True)
    return out


def sizes_of(case, frames, info):
    """the (maxFrames, maxRecs) pairs a case runs with; frames, info: the model's answer with room for everything"""
    if case.sizes is not None:
        return case.sizes
    nf, nr = info["nFrames"], info["nRecs"]
    return [(nf + 3, nr + 70), (nf, nr), (max(nf - 1, 0), nr + 1), (nf + 1, max(nr - 1, 0))]


ROOMY = (400, 2000)                                             # more table than any case of cases() needs
