// lz4_body_index_device.inl -- the index of a frame body that lies in device memory: the size-word walk of FrameReader._read
// (internal/pkg/blk/frame.go:54-98) as device code, for plz4hip_dev_index_body.
//
// A frame's block section is self-describing: every record starts with an LE32 size word and the next record begins
// 4 + size (+ 4 with block checksums) bytes later.  The record decoders want the offset of every record (recOff), and until now the
// only thing that produced it was this engine's own encoder.  The walk is one serial chain -- hop i + 1 cannot start before hop i's
// word has arrived -- so it is ONE wavefront, without LDS and without a workspace; like the streaming checksum it is there to run
// beside other launches and to keep the host out of the chain, not to be fast.
//
//   * the walk state (off, i) is wave-uniform: the size word is loaded byte-safe (ld32u: records lie at any alignment) and taken from
//     the first lane, as rec_head<true> takes a record's head;
//   * lane (i & 63) keeps hop i's offset in a register; every 64 hops the wave writes them with one coalesced 512-byte store, the
//     partial last group likewise, and behind the walk all lanes fill recOff[nBlocks .. maxBlocks] with the final offset, 64 entries
//     a store: the padded tail reads as zero-length records, which rec_head turns into PLZ4HIP_BLK_SIZE_OVERFLOW, result 0, no byte
//     written -- so a decode of maxBlocks records may be enqueued behind the walk without the host looking at nBlocks first;
//   * offsets are 64 bits wide and every test is `need > bodyBytes - off`, never `off + need > bodyBytes`: no size word overflows it;
//   * the walk reads the four bytes of a size word, only where bodyBytes - off >= 4, and nothing else: no payload byte, no byte
//     outside [body, body + bodyBytes);
//   * it ends after at most maxBlocks + 1 loads (the last one tells an end mark from a full index);
//   * the walk and the padding are two functions: the stream index (lz4_stream_index_device.inl) runs the walk once per frame over
//     one recOff, with the stream-wide record index, and the padding once behind the last frame.
#pragma once
#include "wave.h"

namespace plz4 {

// why the walk stopped (== PLZ4HIP_BODY_* of include/plz4hip.h; plz4hip.hip asserts it)
enum : int {
    kBodyEndMark        = 0,   // a size word of 0 (descriptor.DataBlockSize.EOF, frame.go:71): end = behind the word
    kBodyEndOfBytes     = 1,   // off == bodyBytes: a bare block section, as plz4hip_dev_encode_body writes it
    kBodyFull           = 2,   // a record behind the maxBlocks the caller has room for
    kBodySizeOverflow   = 3,   // zerr.ErrBlockSizeOverflow (frame.go:79-81)
    kBodyTruncatedWord  = 4,   // zerr.ErrBlockSizeRead (frame.go:57-61): fewer than four bytes where a size word starts
    kBodyTruncatedBlock = 5    // zerr.ErrBlockRead (frame.go:91-98): the record's bytes end behind the body
};

struct BodyIndex { int64_t end; int32_t nBlocks; int32_t status; };      // == plz4hip_body_index

// The walk: FrameReader._read's steps from `off` on, over [base, base + nBytes), listing records from index i on (lane (k & 63) of
// `held` keeps record k's offset until its group of 64 is stored, so i and held may come from an earlier walk over the same recOff:
// plz4hip_dev_index_stream runs one walk per frame).  atEnd: what off == nBytes means to the caller.  -> why the walk stopped; off is
// left at the end of the last listed record, i behind it, end as the table in plz4hip.h says.  Stores whole groups of 64 only.
DEV int wave_walk_records(const uint8_t* base, const int64_t nBytes, const int bsz, const bool checksum, const int maxBlocks, const int atEnd,
                          int64_t* recOff, LVREF(int64_t, held), int64_t& off, int& i, int64_t& end)
{
    const int64_t tail = checksum ? 8 : 4;                  // size word + block checksum
    int status;
    for (;;) {
        end = off;
        if (off == nBytes)    { status = atEnd;              break; }
        if (nBytes - off < 4) { status = kBodyTruncatedWord; break; }
        const uint32_t word = UNI(ld32u(base + off));
        if (word == 0)           { status = kBodyEndMark; end = off + 4; break; }
        if (i == maxBlocks)      { status = kBodyFull;          break; }
        const uint32_t size = word & 0x7FFFFFFFu;           // 0x80000000: a stored record of size 0, not an end mark (descriptor/data.go:12)
        if (size > (uint32_t)bsz) { status = kBodySizeOverflow; break; }
        const int64_t need = (int64_t)size + tail;
        if (need > nBytes - off) { status = kBodyTruncatedBlock; break; }
        WL(held, i & 63, off);
        off += need; ++i;
        if ((i & 63) == 0) {
            const int64_t g = (int64_t)i - 64;
            LANES({ recOff[g + LANE] = held[I_]; })
        }
    }
    return status;
}

// The padding behind the walk(s): the partial last group of the i listed records, and recOff[i .. maxBlocks] = pad, 64 entries a store.
DEV void wave_pad_rec_off(const int i, const int64_t pad, const int maxBlocks, int64_t* recOff, LVREF(int64_t, held))
{
    const int64_t g0 = (int64_t)(i & ~63), last = (int64_t)maxBlocks;
    const int     part = i & 63;
    LANES({
        const int64_t k = g0 + LANE;
        if (k <= last) recOff[k] = LANE < part ? held[I_] : pad;
    })
    for (int64_t g = g0 + 64; g <= last; g += 64) {
        LANES({
            const int64_t k = g + LANE;
            if (k <= last) recOff[k] = pad;
        })
    }
}

// recOff: maxBlocks + 1 entries.  On every exit recOff[0 .. nBlocks) are the listed records' offsets and
// recOff[nBlocks .. maxBlocks] the end of the last listed one.  0 <= maxBlocks <= 0x7FFFFFFE.
DEV void wave_index_body(const uint8_t* body, const int64_t bodyBytes, const int bsz, const bool checksum, const int maxBlocks,
                         int64_t* recOff, BodyIndex* info)
{
    int64_t off = 0, end = 0;
    int     i = 0;
    LV(int64_t, held);
    LANES({ held[I_] = 0; })
    const int status = wave_walk_records(body, bodyBytes, bsz, checksum, maxBlocks, kBodyEndOfBytes, recOff, held, off, i, end);
    wave_pad_rec_off(i, off, maxBlocks, recOff, held);
    LANES({
        if (LANE == 0) { info->end = end; info->nBlocks = i; info->status = status; }
    })
}

}  // namespace plz4
