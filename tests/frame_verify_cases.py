"""The frame verdicts (plz4hip_dev_verify_frames) for the CPU and the GPU tests: a model of the table of rules in include/plz4hip.h,
written from that table and from nothing else, the builders of hand-made dst / result / status arrays and frame tables -- the call
does not care which decoder left them -- and the list of cases.  Expected checksums are the oracle's xxh32.  Test infrastructure
only."""
from __future__ import annotations

import numpy as np

import body_index_cases as bic
import stream_index_cases as sic

OK, SKIPPABLE, RANGE, BLOCK, INCOMPLETE, CONTENT_HASH, CONTENT_SIZE = range(7)
BLK_OK, BLK_HASH_MISMATCH, BLK_SIZE_OVERFLOW, BLK_CORRUPT = 0, 1, 2, 3

VERDICT_FIELDS = ("contentSz", "contentSum", "status", "firstBad", "blockStatus")
SV_FIELDS = ("contentBytes", "firstBadFrame", "status", "nFrames", "nOk", "nSkippable")
VERDICT_DTYPE = np.dtype([("contentSz", "<u8"), ("contentSum", "<u4"), ("status", "<i4"), ("firstBad", "<i4"), ("blockStatus", "<i4"),
                          ("reserved", "<i4", (2,))])
SV_DTYPE = np.dtype([("contentBytes", "<i8"), ("firstBadFrame", "<i4"), ("status", "<i4"), ("nFrames", "<i4"), ("nOk", "<i4"),
                     ("nSkippable", "<i4"), ("reserved", "<i4")])
assert VERDICT_DTYPE.itemsize == 32 and SV_DTYPE.itemsize == 32

CANARY = 0xC7
FLG = 0x60                                                      # version 01, independent blocks
CCK, CSZ = 4, 8                                                 # FLG bits: content checksum, content size


# ------------------------------------------------------------------------------------------------------------ the model
def model(orc, c):
    """-> (verdicts: list of dicts with VERDICT_FIELDS for frames [0, nFrames), sv: dict with SV_FIELDS)"""
    nf = max(0, min(int(c.info["nFrames"][0]), c.max_frames))
    out = []
    for f in range(nf):
        e = c.frames[f]
        v = dict(contentSz=0, contentSum=0, status=None, firstBad=-1, blockStatus=0)
        out.append(v)
        if int(e["kind"]) == 1:
            v["status"] = SKIPPABLE
            continue
        first, n, flg = int(e["firstRec"]), int(e["nRecs"]), int(e["flags"])
        complete = int(e["status"]) == bic.END_MARK
        hashed = complete and bool(flg & CCK)
        data = []
        if first < 0 or n < 0 or first + n > c.max_recs:
            v["status"] = RANGE
        else:
            for i in range(first, first + n):
                if int(c.status[i]) != BLK_OK:
                    v.update(status=BLOCK, firstBad=i, blockStatus=int(c.status[i])); break
                r = int(c.result[i])
                if r < 0 or r > c.cap:
                    v.update(status=RANGE, firstBad=i); break
                v["contentSz"] += r
                if hashed:
                    assert i * c.stride + r <= c.dst.size, "the model itself reads outside dst"
                    data.append(bytes(c.dst[i * c.stride:i * c.stride + r]))
        if hashed:
            v["contentSum"] = orc.xxh32(b"".join(data))
        if v["status"] is not None:
            continue
        if not complete:
            v["status"] = INCOMPLETE
        elif flg & CCK and v["contentSum"] != int(e["contentSum"]):
            v["status"] = CONTENT_HASH
        elif flg & CSZ and v["contentSz"] != int(e["contentSz"]):
            v["status"] = CONTENT_SIZE
        else:
            v["status"] = OK
    sv = dict(contentBytes=0, firstBadFrame=-1, status=0, nFrames=nf, nOk=sum(v["status"] == OK for v in out),
              nSkippable=sum(v["status"] == SKIPPABLE for v in out))
    for f, v in enumerate(out):
        sv["contentBytes"] += v["contentSz"]
        if v["status"] not in (OK, SKIPPABLE):
            sv.update(firstBadFrame=f, status=v["status"]); break
    return out, sv


def verdicts_of(raw: np.ndarray, n: int):
    assert not raw["reserved"][:n].any(), "verdict.reserved is not 0"
    return [{k: int(raw[j][k]) for k in VERDICT_FIELDS} for j in range(n)]


def sv_of(raw):
    assert int(raw["reserved"]) == 0, "sv.reserved is not 0"
    return {k: int(raw[k]) for k in SV_FIELDS}


# ------------------------------------------------------------------------------------------------------------ the builders
class Case:
    """what one call takes: frames (FRAME_DTYPE, at least max_frames entries), info (INFO_DTYPE x 1), max_frames, dst (uint8,
    max_recs * stride bytes), stride, cap, result / status (int32 x max_recs), max_recs; waves: the cap on the grid, or None"""

    def __init__(self, name, frames, n_frames_info, max_frames, dst, stride, cap, result, status, max_recs, waves=None):
        self.name, self.frames, self.max_frames, self.dst, self.stride, self.cap = name, frames, max_frames, dst, stride, cap
        self.result, self.status, self.max_recs, self.waves = result, status, max_recs, waves
        self.info = np.zeros(1, dtype=sic.INFO_DTYPE)
        self.info["nFrames"] = n_frames_info
        self.info["status"] = sic.END


class Builder:
    """frames of hand-made pieces: record i is `result` bytes of noise at dst + i * stride"""

    def __init__(self, orc, cap, stride=None, seed=1):
        self.orc, self.cap, self.stride = orc, cap, cap if stride is None else stride
        self.rng = np.random.default_rng(seed)
        self.recs, self.frames = [], []                         # (bytes, result, status); dicts of FRAME_FIELDS

    def frame(self, pieces, flg=FLG | CCK, entry_status=bic.END_MARK, sum_xor=0, size_delta=0, statuses=None, results=None,
              first_rec=None, n_recs=None, kind=0):
        """pieces: the records' lengths; statuses / results: {index in the frame: value} that lie about a record; sum_xor /
        size_delta: what the entry's stored checksum / content size is off by; first_rec / n_recs: a lying table entry"""
        first = len(self.recs)
        datas = [self.rng.integers(0, 256, size=int(n), dtype=np.uint8) for n in pieces]
        for k, d in enumerate(datas):
            self.recs.append((d, (results or {}).get(k, d.size), (statuses or {}).get(k, BLK_OK)))
        whole = np.concatenate(datas) if datas else np.zeros(0, np.uint8)
        self.frames.append(dict(hdrOff=0, bodyOff=7, end=11, contentSz=whole.size + size_delta if flg & CSZ else 0, dictId=0,
                                contentSum=(self.orc.xxh32(whole) ^ sum_xor) if flg & CCK else 0,
                                firstRec=first if first_rec is None else first_rec, nRecs=len(pieces) if n_recs is None else n_recs,
                                bsz=64 << 10, flags=flg, blockDesc=0x40, kind=kind, nibble=0, status=entry_status, reserved=0))
        return self

    def skippable(self, payload=11, first_rec=None):
        self.frames.append(dict(hdrOff=0, bodyOff=8, end=8 + payload, contentSz=payload, dictId=0, contentSum=0,
                                firstRec=len(self.recs) if first_rec is None else first_rec, nRecs=0, bsz=0, flags=0, blockDesc=0, kind=1,
                                nibble=3, status=bic.END_MARK, reserved=0))
        return self

    def build(self, name, max_frames=None, n_frames_info=None, extra_recs=0, drop_recs=0, waves=None):
        """max_frames: the table the call is told of (default: the frames built); n_frames_info: what info->nFrames says (default:
        min(frames built, max_frames)); extra_recs: padding records behind the listed ones, as the index pads recOff; drop_recs:
        maxRecs that many short of the records the table lists"""
        n = len(self.frames)
        mf = n if max_frames is None else max_frames
        tab = np.frombuffer(bytes([CANARY]) * (64 * max(n, mf)), dtype=sic.FRAME_DTYPE).copy()
        for j, f in enumerate(self.frames):
            for k, v in f.items():
                tab[j][k] = v
        mr = len(self.recs) + extra_recs - drop_recs
        dst = np.full(max(mr, 0) * self.stride, 0xEE, dtype=np.uint8)
        result = np.zeros(mr, dtype=np.int32); status = np.full(mr, BLK_SIZE_OVERFLOW, dtype=np.int32)
        for i, (d, r, st) in enumerate(self.recs[:mr]):
            dst[i * self.stride:i * self.stride + d.size] = d
            result[i] = r; status[i] = st
        return Case(name, tab, min(n, mf) if n_frames_info is None else n_frames_info, mf, dst, self.stride, self.cap, result, status, mr,
                    waves)


# ------------------------------------------------------------------------------------------------------------ the cases
# the smallest shapes at which each path of the piece update can go wrong: the byte-wise completion, the eight-in-flight loop, the
# ring entered at 64 stripes and refilled at 128
PIECE_LENGTHS = (0, 1, 3, 4, 15, 16, 17, 31, 32, 127, 128, 1023, 1024, 1025, 2047, 2048, 2049, 2048 + 16 * 3 + 5, 2048 + 16 * 64 + 7,
                 2048 + 16 * 129 + 1)
PIECE_CAP = max(PIECE_LENGTHS)


def piece_cases(orc):
    out = []
    # 1. every length behind every pending fill, 7 more bytes behind it (what the piece left pending must go on correctly)
    b = Builder(orc, PIECE_CAP, PIECE_CAP + 3, seed=2)
    for n in PIECE_LENGTHS:
        for fill in range(16):
            b.frame(([fill] if fill else []) + [n, 7])
    out.append(b.build("every length behind every fill", extra_recs=3))
    # 2. a piece that is the last one, and one that starts behind whole stripes
    b = Builder(orc, PIECE_CAP, seed=3)
    for n in PIECE_LENGTHS:
        b.frame([n]); b.frame([32, n]); b.frame([n, n])
    out.append(b.build("every length alone, behind 32 bytes, twice"))
    # 3. runs of 1-byte and 0-byte pieces inside one stripe and across stripes; frames of 0 records; totals of 0, 15 and 16 bytes
    b = Builder(orc, 40, 48, seed=4)
    b.frame([1] * 16).frame([1] * 17).frame([1] * 40).frame([0] * 20).frame([0] * 17 + [1] * 3 + [0] * 16 + [1] * 14)
    b.frame([5] + [0, 1] * 24).frame([1, 0] * 8).frame([3] + [1] * 13 + [33] + [1] * 15 + [0] * 3 + [2])
    b.frame([]).frame([15]).frame([16]).frame([7, 8]).frame([8, 8]).frame([0]).frame([0, 0, 15]).frame([0, 16, 0]).frame([4, 4, 4, 3]).frame([4, 4, 4, 4])
    b.frame([], flg=FLG | CCK | CSZ).frame([], flg=FLG)
    out.append(b.build("runs of tiny pieces, empty frames, totals below a stripe"))
    # 4. 15, 16, 17 and 33 frames; 16 W + 1 frames beyond a grid of W waves
    for n, waves in ((15, None), (16, None), (17, None), (33, None), (33, 2), (33, 1), (17, 1), (49, 3)):
        b = Builder(orc, 600, seed=5 + n)
        for k in range(n):
            b.frame([(k * 37) % 300, (k * 101) % 600, k % 19])
        out.append(b.build("%d frames%s" % (n, "" if waves is None else ", %d waves" % waves), waves=waves))
    # 5. frames of very different lengths in one wave
    b = Builder(orc, 3000, seed=9)
    for k, n in enumerate((0, 9000, 1, 64, 3000, 16, 2048, 15, 5, 1024, 0, 6001, 17, 128, 2049, 33)):
        b.frame([3000] * (n // 3000) + [n % 3000])
    out.append(b.build("sixteen frames of 0 .. 9000 bytes in one wave"))
    return out


def verdict_stream(orc, seed=11):
    """one table with every verdict in it, the first rule of the header's table winning wherever two apply"""
    b = Builder(orc, 300, 304, seed=seed)
    b.skippable()                                                                               # 0  a skippable frame first
    b.frame([100, 200, 50])                                                                     # 1  OK
    b.frame([10, 20, 30], statuses={0: BLK_HASH_MISMATCH})                                      # 2  a bad block first
    b.skippable(0)                                                                              # 3  ... between
    b.frame([10, 20, 30], statuses={1: BLK_CORRUPT}, results={1: -7})                           # 4  in the middle (BLOCK before RANGE)
    b.frame([10, 20, 30], statuses={2: BLK_SIZE_OVERFLOW})                                      # 5  last
    b.frame([10, 20, 30], results={1: -1})                                                      # 6  a result of -1 with status OK
    b.frame([10, 20, 30], results={2: 301})                                                     # 7  dstCap + 1
    b.frame([300, 0, 300], results={})                                                          # 8  results of exactly dstCap: OK
    b.frame([40, 50], sum_xor=1, size_delta=1, flg=FLG | CCK | CSZ)                             # 9  wrong hash and wrong size: HASH
    b.frame([40, 50], size_delta=-1, flg=FLG | CCK | CSZ)                                       # 10 right hash, wrong size: SIZE
    b.frame([40, 50], flg=FLG | CCK | CSZ)                                                      # 11 both right
    b.frame([40, 50], flg=FLG | CSZ)                                                            # 12 a right size without a checksum
    b.frame([40, 50], size_delta=1 << 32, flg=FLG | CSZ)                                        # 13 a wrong one (above 32 bits)
    b.frame([40, 50], flg=FLG, sum_xor=5)                                                       # 14 nothing to check
    b.frame([40, 50], first_rec=-1)                                                             # 15 RANGE
    b.frame([40, 50], n_recs=-2)                                                                # 16
    b.frame([40, 50], first_rec=0x7FFFFFFF, n_recs=0x7FFFFFFF)                                  # 17 the sum overflows 32 bits
    b.frame([], first_rec=0x7FFFFFFE, n_recs=0)                                                 # 18 RANGE although nothing is listed
    b.frame([40, 50], kind=1, first_rec=-5, n_recs=-5)                                          # 19 SKIPPABLE wins over RANGE
    b.frame([40, 50], entry_status=bic.TRUNCATED_BLOCK, statuses={1: BLK_CORRUPT})              # 20 BLOCK wins over INCOMPLETE
    b.frame([40, 50], entry_status=bic.FULL, first_rec=-1)                                      # 21 RANGE wins over INCOMPLETE
    b.frame([40, 50], sum_xor=0x80000000, statuses={1: BLK_HASH_MISMATCH})                      # 22 BLOCK wins over CONTENT_HASH
    b.frame([40, 50], flg=FLG | CSZ, size_delta=3, results={0: 400})                            # 23 RANGE wins over CONTENT_SIZE
    b.frame([40, 50], sum_xor=0xFFFFFFFF)                                                       # 24 CONTENT_HASH alone
    b.skippable(5)                                                                              # 25
    b.frame([40, 50], entry_status=bic.TRUNCATED_WORD, sum_xor=3, flg=FLG | CCK | CSZ, size_delta=9)   # 26 INCOMPLETE: nothing compared
    b.skippable(1)                                                                              # 27 a skippable frame last
    return b


def verdict_cases(orc):
    out = []
    n = len(verdict_stream(orc).frames)
    out.append(verdict_stream(orc).build("every verdict", extra_recs=5))
    for mf in (n - 1, n, n + 1, 0):
        out.append(verdict_stream(orc).build("every verdict, maxFrames %d" % mf, max_frames=mf, n_frames_info=n))
    out.append(verdict_stream(orc).build("every verdict, info->nFrames above maxFrames", max_frames=n - 3, n_frames_info=0x7FFFFFFF))
    out.append(verdict_stream(orc).build("every verdict, info->nFrames negative", n_frames_info=-1))
    out.append(verdict_stream(orc).build("every verdict, info->nFrames 0", n_frames_info=0))
    out.append(verdict_stream(orc).build("every verdict, one wave", waves=1))
    # firstRec + nRecs one beyond maxRecs: the last frame's last record is not the decode's
    b = Builder(orc, 64, seed=12).frame([10, 20]).frame([30, 40, 50])
    out.append(b.build("one record beyond maxRecs", drop_recs=1))
    b = Builder(orc, 64, seed=12).frame([10, 20]).frame([30, 40, 50])
    out.append(b.build("exactly maxRecs"))
    b = Builder(orc, 64, seed=12).frame([10, 20]).frame([30, 40, 50])
    out.append(b.build("maxRecs 0", drop_recs=5))
    # an incomplete last frame behind good ones; a bad frame first; all good: contentBytes is the sum over all
    b = Builder(orc, 64, seed=13).frame([10, 20]).skippable().frame([30, 40, 50], entry_status=bic.TRUNCATED_WORD)
    out.append(b.build("an incomplete last frame"))
    b = Builder(orc, 64, seed=14).frame([10, 20], sum_xor=2).frame([30, 40, 50])
    out.append(b.build("a bad frame first"))
    b = Builder(orc, 64, seed=15)
    for k in range(70):                                         # the summary's second step of 64 entries
        b.frame([k % 64, 1]) if k % 5 else b.skippable()
    out.append(b.build("seventy good frames"))
    b = Builder(orc, 64, seed=15)
    for k in range(70):
        b.frame([k % 64, 1], sum_xor=int(k in (66, 68))) if k % 5 else b.skippable()
    out.append(b.build("seventy frames, the 67th bad"))
    for at in (63, 64):
        b = Builder(orc, 64, seed=16)
        for k in range(130):
            b.frame([k % 64, 1], statuses={1: BLK_CORRUPT} if k == at else None)
        out.append(b.build("130 frames, entry %d bad" % at))
    out.append(Builder(orc, 64).build("no frames"))
    return out


def cases(orc):
    return piece_cases(orc) + verdict_cases(orc)


# ------------------------------------------------------------------------------------------------------------ real frames
def decoded_case(orc, stream: np.ndarray, name: str, cap: int = 64 << 10, extra_frames: int = 2, extra_recs: int = 3):
    """the model of the stream index over `stream`, and every listed record decoded by the oracle: what index and one record decode
    leave for the call.  -> (Case, the index's info)"""
    frames, rec_off, info = sic.model(sic.reader_of(stream), stream.size, 64, 256)
    n, mr = info["nRecs"], info["nRecs"] + extra_recs
    stride = cap
    dst = np.full(mr * stride, 0xEE, dtype=np.uint8)
    result = np.zeros(mr, dtype=np.int32); status = np.full(mr, BLK_SIZE_OVERFLOW, dtype=np.int32)
    for i in range(n):
        at = int(rec_off[i])
        word = int.from_bytes(bytes(stream[at:at + 4]), "little")
        size = word & 0x7FFFFFFF
        payload = stream[at + 4:at + 4 + size]
        if word >> 31:
            out = payload
        else:
            r, out = orc.decompress_safe(np.ascontiguousarray(payload), cap)
            assert r >= 0
        dst[i * stride:i * stride + out.size] = out
        result[i] = out.size; status[i] = BLK_OK
    mf = len(frames) + extra_frames
    tab = np.frombuffer(bytes([CANARY]) * (64 * mf), dtype=sic.FRAME_DTYPE).copy()
    for j, f in enumerate(frames):
        for k, v in f.items():
            tab[j][k] = v
    return Case(name, tab, len(frames), mf, dst, stride, cap, result, status, mr), info
