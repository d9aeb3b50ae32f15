// lz4_stream_index_device.inl -- the index of a whole LZ4 stream that lies in device memory: the reader's header-mode / body-mode
// walk (rdr/rdr.go:242-296, header/read.go:26-119, header/skip.go:38-76, blk/frame.go:54-139) as device code, for
// plz4hip_dev_index_stream.
//
// A stream is frames back to back, skippable ones among them; where frame k + 1 starts is known only behind frame k's end mark, so
// a host that walks it pays a device-to-host round trip per header, per body and per trailer.  Here the whole chain stays in ONE
// wavefront, like the body walk it contains (lz4_body_index_device.inl), without LDS and without a workspace:
//
//   * the walk state (off, the frame and record counts) is wave-uniform;
//   * a header is ONE round trip: lanes 0 .. 18 each load the byte of the longest possible header that is in range, and the fields
//     come out with readlane; the descriptor's xxh32 (at most 14 bytes) is uniform arithmetic;
//   * the record walk is wave_walk_records with the stream-wide record index: lane (i & 63) holds record i's offset and a group of
//     64 goes out with one coalesced 512-byte store, across frame boundaries; the padding of recOff runs once, behind the stream;
//   * a frame's 64-byte table entry is one store, lanes 0 .. 15 a dword each;
//   * every test is `need > nBytes - off` in 64 bits; the walk reads header bytes, size words and content-checksum words, each only
//     where the remaining length holds it: never a payload byte, nothing outside [bytes, bytes + nBytes).
#pragma once
#include "lz4_body_index_device.inl"

namespace plz4 {

// why the stream walk stopped (== PLZ4HIP_STREAM_* of include/plz4hip.h; plz4hip.hip asserts it)
enum : int {
    kStreamEnd             = 0,
    kStreamFramesFull      = 1,
    kStreamRecordsFull     = 2,
    kStreamHeaderRead      = 3,
    kStreamMagic           = 4,
    kStreamVersion         = 5,
    kStreamReservedBit     = 6,
    kStreamBlockDescriptor = 7,
    kStreamHeaderHash      = 8,
    kStreamSkip            = 9,
    kStreamBody            = 10,
    kStreamContentHashRead = 11
};

struct FrameIndex {                                          // == plz4hip_frame_index
    int64_t  hdrOff, bodyOff, end;
    uint64_t contentSz;
    uint32_t dictId, contentSum;
    int32_t  firstRec, nRecs, bsz;
    uint8_t  flags, blockDesc, kind, nibble;
    int32_t  status, reserved;
};
struct StreamIndex {                                         // == plz4hip_stream_index
    int64_t end;
    int32_t nFrames, nRecs, status, nSkippable, maxBsz;
    uint8_t flagsAnd, flagsOr, pad[2];
};

// one step of xxh32 over a 4-byte lane / a single byte, for inputs below 16 bytes (xxh32.ChecksumZero of a frame descriptor)
DEV uint32_t sx_word(uint32_t h, uint32_t w) { return rotl32(h + w * 3266489917u, 17) * 668265263u; }
DEV uint32_t sx_byte(uint32_t h, uint32_t b) { return rotl32(h + b * 374761393u, 11) * 2654435761u; }

// the 16 dwords of a table entry, lane k's one: a select chain over uniform values (no indexed array: the compiler may put one into scratch)
DEV void wave_store_frame(FrameIndex* e, const int64_t hdrOff, const int64_t bodyOff, const int64_t end, const uint64_t contentSz,
                          const uint32_t dictId, const uint32_t contentSum, const int firstRec, const int nRecs, const int bsz,
                          const uint32_t bytes4, const int status)
{
    uint32_t* const p = (uint32_t*)e;
    LANES({
        const int k = LANE;
        uint32_t v = 0;                                      // (lane 15: reserved)
        v = k == 0 ? (uint32_t)hdrOff : v;     v = k == 1 ? (uint32_t)((uint64_t)hdrOff >> 32) : v;
        v = k == 2 ? (uint32_t)bodyOff : v;    v = k == 3 ? (uint32_t)((uint64_t)bodyOff >> 32) : v;
        v = k == 4 ? (uint32_t)end : v;        v = k == 5 ? (uint32_t)((uint64_t)end >> 32) : v;
        v = k == 6 ? (uint32_t)contentSz : v;  v = k == 7 ? (uint32_t)(contentSz >> 32) : v;
        v = k == 8 ? dictId : v;               v = k == 9 ? contentSum : v;
        v = k == 10 ? (uint32_t)firstRec : v;  v = k == 11 ? (uint32_t)nRecs : v;
        v = k == 12 ? (uint32_t)bsz : v;       v = k == 13 ? bytes4 : v;
        v = k == 14 ? (uint32_t)status : v;
        if (k < 16) p[k] = v;
    })
}

// frames: maxFrames entries; recOff: maxRecs + 1.  0 <= maxRecs <= 0x7FFFFFFE, maxFrames >= 0.  The steps and their order: the table
// at plz4hip_dev_index_stream in include/plz4hip.h.
DEV void wave_index_stream(const uint8_t* bytes, const int64_t nBytes, const int maxFrames, const int maxRecs, FrameIndex* frames,
                           int64_t* recOff, StreamIndex* info)
{
    int64_t off = 0, end = 0, recEnd = 0;                    // recEnd: the end of the last listed record
    int     nFrames = 0, nSkip = 0, i = 0, status, maxBsz = 0;
    uint32_t flagsAnd = 0xFFu, flagsOr = 0;
    LV(int64_t, held);
    LV(uint32_t, hb);
    LANES({ held[I_] = 0; })
    for (;;) {
        end = off;
        if (off == nBytes)        { status = kStreamEnd;        break; }
        if (nFrames == maxFrames) { status = kStreamFramesFull; break; }
        const int64_t left = nBytes - off;
        if (left < 7)             { status = kStreamHeaderRead; break; }
        const int avail = (int)min_<int64_t>(left, 19);
        LANES({ hb[I_] = LANE < avail ? (uint32_t)bytes[off + LANE] : 0u; })
        const uint32_t magic = RL(hb, 0) | RL(hb, 1) << 8 | RL(hb, 2) << 16 | RL(hb, 3) << 24;
        const uint32_t b4 = RL(hb, 4), b5 = RL(hb, 5), b6 = RL(hb, 6);
        if ((magic >> 4) == (0x184D2A50u >> 4)) {                                          // a skippable frame (skip.go:38-76)
            if (left < 8)                     { status = kStreamHeaderRead; break; }
            const uint32_t size = b4 | b5 << 8 | b6 << 16 | RL(hb, 7) << 24;
            if ((int64_t)size > left - 8)     { status = kStreamSkip;       break; }
            const int64_t behind = off + 8 + (int64_t)size;
            wave_store_frame(frames + nFrames, off, off + 8, behind, size, 0, 0, i, 0, 0, 1u << 16 | (magic & 15u) << 24, kBodyEndMark);
            ++nFrames; ++nSkip;
            off = behind;
            continue;
        }
        if (magic != 0x184D2204u)             { status = kStreamMagic;           break; }
        const uint32_t flg = b4, bd = b5;
        if ((flg >> 6) != 1u)                 { status = kStreamVersion;         break; }  // read.go:107-119, in its order
        if (flg & 2u)                         { status = kStreamReservedBit;     break; }
        if (((bd >> 4) & 7u) < 4u || (bd & 0x8Fu)) { status = kStreamBlockDescriptor; break; }
        const int hlen = 7 + ((flg & 8u) ? 8 : 0) + ((flg & 1u) ? 4 : 0);
        if (hlen > avail)                     { status = kStreamHeaderRead;      break; }
        // xxh32 (seed 0) of bytes 4 .. hlen - 2: 2, 6, 10 or 14 of them -- whole words, then always two single bytes
        const int dlen = hlen - 5;
        uint32_t h = 374761393u + (uint32_t)dlen;
        uint64_t contentSz = 0;
        uint32_t dictId = 0;
        int at = 4;
        if (flg & 8u) {
            const uint32_t w0 = b4 | b5 << 8 | b6 << 16 | RL(hb, 7) << 24;
            const uint32_t w1 = RL(hb, 8) | RL(hb, 9) << 8 | RL(hb, 10) << 16 | RL(hb, 11) << 24;
            h = sx_word(sx_word(h, w0), w1);
            contentSz = (uint64_t)(w0 >> 16) | (uint64_t)w1 << 16 | (uint64_t)RL(hb, 12) << 48 | (uint64_t)RL(hb, 13) << 56;
            at = 12;
        }
        if (flg & 1u) {
            const uint32_t w = RL(hb, at) | RL(hb, at + 1) << 8 | RL(hb, at + 2) << 16 | RL(hb, at + 3) << 24;
            h = sx_word(h, w);
            dictId = w >> 16 | RL(hb, at + 4) << 16 | RL(hb, at + 5) << 24;
            at += 4;
        }
        h = sx_byte(sx_byte(h, RL(hb, at)), RL(hb, at + 1));
        h ^= h >> 15; h *= 2246822519u; h ^= h >> 13; h *= 3266489917u; h ^= h >> 16;
        if (((h >> 8) & 0xFFu) != RL(hb, hlen - 1)) { status = kStreamHeaderHash; break; }
        // the frame is listed; its records (frame.go:54-98) go into the one recOff
        const int     bsz = 65536 << 2 * (int)(((bd >> 4) & 7u) - 4u);
        const int     firstRec = i;
        const int64_t hdrOff = off;
        off += hlen;
        const int64_t bodyOff = off;
        const int body = wave_walk_records(bytes, nBytes, bsz, (flg & 16u) != 0, maxRecs, kBodyTruncatedWord, recOff, held, off, i, end);
        if (i > firstRec) recEnd = off;
        uint32_t contentSum = 0;
        status = body == kBodyEndMark ? -1 : body == kBodyFull ? kStreamRecordsFull : kStreamBody;
        if (body == kBodyEndMark && (flg & 4u)) {
            if (nBytes - end < 4) status = kStreamContentHashRead;
            else { contentSum = UNI(ld32u(bytes + end)); end += 4; }
        }
        wave_store_frame(frames + nFrames, hdrOff, bodyOff, end, contentSz, dictId, contentSum, firstRec, i - firstRec, bsz,
                         flg | bd << 8, body);
        ++nFrames;
        flagsAnd &= flg; flagsOr |= flg; maxBsz = max_(maxBsz, bsz);
        if (status >= 0) break;
        off = end;
    }
    wave_pad_rec_off(i, recEnd, maxRecs, recOff, held);
    if (nFrames == nSkip) flagsAnd = 0;
    LANES({
        if (LANE == 0) {
            info->end = end; info->nFrames = nFrames; info->nRecs = i; info->status = status; info->nSkippable = nSkip;
            info->maxBsz = maxBsz; info->flagsAnd = (uint8_t)flagsAnd; info->flagsOr = (uint8_t)flagsOr; info->pad[0] = 0; info->pad[1] = 0;
        }
    })
}

}  // namespace plz4
