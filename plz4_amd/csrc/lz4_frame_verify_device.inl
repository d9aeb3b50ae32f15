// lz4_frame_verify_device.inl -- the verdict on every frame of a decoded stream that lies in device memory: the back half of the
// reference's Reader (content checksum: async/reader.go:236-241, sync/reader.go:56-67; content size: rdr/rdr.go:91-101) as device
// code, for plz4hip_dev_verify_frames.
//
// The stream index (lz4_stream_index_device.inl) left a table of frames and ONE recOff; one record decode left result[i] bytes of
// plaintext at dst + i * dstStride with status[i].  What is still to be said of a frame -- did every block decode, do its bytes hash
// to the stored content checksum, are there as many as the header promised -- is said here, without a host in the loop:
//
//   * XXH32 has no combine operator: a frame is one serial chain of four accumulators.  But frames are independent of each other,
//     so a wave serves SIXTEEN of them, lane 4g + l owning accumulator l of frame 16w + g (the lane layout of wave_xxh32_x16);
//   * a frame's plaintext is not contiguous: it comes in pieces, one per record.  piece_update below is the streaming form of the
//     x16 chain: per lane the accumulator, the lane's own dword of the pending stripe (lane l: bytes 4l .. 4l + 3) and the
//     group's fill, 0 .. 15 -- the XXHZero.Write rule of wave_xxh32_stream_update with its state in registers;
//   * every lane walks its frame's records itself: the four lanes of a group read the same status / result words and take the same
//     branches, so nothing crosses lanes until the frame's end, where the group's first lane gathers four accumulators and four
//     pending dwords with SHFL, does the tail, the avalanche and the compares, and stores the 32-byte verdict;
//   * no LDS, no workspace, no atomics: the stream verdict is k_verify_summary's, one wave behind this kernel on the same stream.
//
// One frame is one chain: a stream of few huge frames runs at one chain's rate per frame, and the frames of one wave finish with its
// longest.  Nothing changes that for XXH32.
#pragma once
#include "lz4_device.inl"
#include "lz4_stream_index_device.inl"

namespace plz4 {

// a frame's verdict (== PLZ4HIP_FRAME_* of include/plz4hip.h; plz4hip.hip asserts it)
enum : int {
    kFrameOk          = 0,
    kFrameSkippable   = 1,
    kFrameRange       = 2,
    kFrameBlock       = 3,
    kFrameIncomplete  = 4,
    kFrameContentHash = 5,
    kFrameContentSize = 6
};

struct FrameVerdict {                                        // == plz4hip_frame_verdict
    uint64_t contentSz;
    uint32_t contentSum;
    int32_t  status, firstBad, blockStatus;
    int32_t  reserved[2];
};
struct StreamVerdict {                                       // == plz4hip_stream_verdict
    int64_t contentBytes;
    int32_t firstBadFrame, status, nFrames, nOk, nSkippable, reserved;
};

// The ring of this kernel: every lane keeps kVerifyDepth of its own dwords in flight, as wave_xxh32_x16 does.
constexpr int kVerifyDepth = 64;

// One lane's share of the streaming chain of its frame: a -- its accumulator, pend -- its dword of the pending stripe (bytes that are
// not there yet are 0), fill -- how many bytes of that stripe are there (the same in the four lanes of a group).
struct PieceChain { uint32_t a, pend, fill; };

// byte k (0 .. 3) of lane l's dword of a stripe that starts at t, if it lies below `end` bytes of the stripe and not below `from`
DEV uint32_t piece_bytes(const uint8_t* t, const int l, const int from, const int end)
{
    uint32_t w = 0;
    _Pragma("unroll")
    for (int k = 0; k < 4; ++k) {
        const int b = 4 * l + k;
        if (b >= from && b < end) w |= (uint32_t)t[b - from] << 8 * k;
    }
    return w;
}

// the n bytes at p go into the chain (n >= 0; lane l = LANE & 3).  Plain per-lane code: it is called inside LANES(...).
// No load touches a byte at or beyond p + n.
DEV void piece_update(PieceChain& c, const uint8_t* p, int n, const int l)
{
    if (c.fill) {                                                           // 1. complete the pending stripe byte-wise
        const int fill = (int)c.fill;
        const int take = min_(16 - fill, n);
        c.pend |= piece_bytes(p, l, fill, fill + take);
        c.fill = (uint32_t)(fill + take);
        if (c.fill < 16u) return;                                           // (the piece is used up: take == n)
        c.a = xxh32_round(c.a, c.pend);
        c.pend = 0; c.fill = 0;
        p += take; n -= take;
    }
    const int stripes = n >> 4;                                             // 2. whole stripes straight from the piece
    uint32_t a = c.a;
    const uint8_t* q = p + 4 * l;
    int s = 0;
    if (stripes >= kVerifyDepth) {                                          // 3. the ring, where all of its stripes lie inside
        uint32_t x[kVerifyDepth];
        _Pragma("unroll")
        for (int j = 0; j < kVerifyDepth; ++j) x[j] = ld32u(q + 16 * j);
        for (; s + 2 * kVerifyDepth <= stripes; s += kVerifyDepth) {        // stripes s + D .. s + 2D - 1 exist: refill as we go
            const uint8_t* const qn = q + 16 * (size_t)kVerifyDepth;
            _Pragma("unroll")
            for (int j = 0; j < kVerifyDepth; ++j) { a = xxh32_round(a, x[j]); x[j] = ld32u(qn + 16 * j); }
            q = qn;
        }
        _Pragma("unroll")
        for (int j = 0; j < kVerifyDepth; ++j) a = xxh32_round(a, x[j]);
        q += 16 * (size_t)kVerifyDepth; s += kVerifyDepth;
    }
    for (; s + 8 <= stripes; s += 8) {                                      // fewer than 2 * depth left: 8 loads in flight
        const uint32_t x0 = ld32u(q), x1 = ld32u(q + 16), x2 = ld32u(q + 32), x3 = ld32u(q + 48);
        const uint32_t x4 = ld32u(q + 64), x5 = ld32u(q + 80), x6 = ld32u(q + 96), x7 = ld32u(q + 112);
        a = xxh32_round(a, x0); a = xxh32_round(a, x1); a = xxh32_round(a, x2); a = xxh32_round(a, x3);
        a = xxh32_round(a, x4); a = xxh32_round(a, x5); a = xxh32_round(a, x6); a = xxh32_round(a, x7);
        q += 128;
    }
    for (; s < stripes; ++s) { a = xxh32_round(a, ld32u(q)); q += 16; }
    c.a = a;
    const int tail = n & 15;                                                // 4. the tail becomes the pending stripe
    if (tail) {
        const uint8_t* const t = p + ((size_t)stripes << 4);
        c.pend = 4 * l + 4 <= tail ? ld32u(t + 4 * l) : piece_bytes(t, l, 0, tail);
        c.fill = (uint32_t)tail;
    }
}

// XXHZero.Sum32 from the four accumulators, the four dwords of the pending stripe and the byte count
DEV uint32_t piece_sum(const uint32_t a0, const uint32_t a1, const uint32_t a2, const uint32_t a3, const uint32_t w0, const uint32_t w1,
                       const uint32_t w2, const uint32_t w3, const uint32_t fill, const uint64_t total)
{
    uint32_t h = (uint32_t)total;
    if (total >= 16) h += rotl32(a0, 1) + rotl32(a1, 7) + rotl32(a2, 12) + rotl32(a3, 18);
    else h += XP5;
    const uint32_t words = fill >> 2;
    if (words > 0) h = rotl32(h + w0 * XP3, 17) * XP4;
    if (words > 1) h = rotl32(h + w1 * XP3, 17) * XP4;
    if (words > 2) h = rotl32(h + w2 * XP3, 17) * XP4;
    uint32_t w = words == 0 ? w0 : words == 1 ? w1 : words == 2 ? w2 : w3;  // (a select chain, no indexed array)
    for (uint32_t k = fill & 3u; k; --k) { h = rotl32(h + (w & 0xFFu) * XP5, 11) * XP1; w >>= 8; }
    h ^= h >> 15; h *= XP2; h ^= h >> 13; h *= XP3; h ^= h >> 16;
    return h;
}

// Wave `wave` of `nWaves`: frames 16w .. 16w + 15 for w = wave, wave + nWaves, ... while 16w < nFrames.  The rules and their order:
// the table at plz4hip_dev_verify_frames in include/plz4hip.h.  0 <= maxRecs <= 0x7FFFFFFE, 0 <= dstCap <= dstStride.
DEV void wave_verify_frames(const FrameIndex* frames, const StreamIndex* info, const int maxFrames, const uint8_t* dst,
                            const int64_t dstStride, const int dstCap, const int32_t* result, const int32_t* status, const int maxRecs,
                            FrameVerdict* verdicts, const int wave, const int nWaves)
{
    const int nFrames = max_(0, min_((int)UNI((uint32_t)info->nFrames), maxFrames));
    for (int64_t w = wave; 16 * w < nFrames; w += nWaves) {
        LV(uint32_t, acc); LV(uint32_t, pend); LV(uint32_t, fill);
        LV(uint64_t, size); LV(uint64_t, wantSz);
        LV(uint32_t, wantSum); LV(uint32_t, what);                          // what: FLG | hashed << 8
        LV(int, verdict); LV(int, firstBad); LV(int, blockStatus);
        LANES({
            const int l = LANE & 3;
            const int64_t f = 16 * w + (LANE >> 2);
            PieceChain c;
            c.a = (l == 0) ? XP1 + XP2 : (l == 1) ? XP2 : (l == 2) ? 0u : 0u - XP1;
            c.pend = 0; c.fill = 0;
            uint64_t sz = 0;
            int v = -1, bad = -1, bst = 0;
            uint32_t flg = 0, hashed = 0;
            wantSz[I_] = 0; wantSum[I_] = 0;
            if (f < nFrames) {
                const FrameIndex* const e = frames + f;
                if (e->kind == 1) v = kFrameSkippable;
                else {
                    const int firstRec = e->firstRec, nRecs = e->nRecs;
                    const bool complete = e->status == kBodyEndMark;
                    flg = e->flags;
                    hashed = (complete && (flg & 4u)) ? 1u : 0u;
                    wantSz[I_] = e->contentSz; wantSum[I_] = e->contentSum;
                    if (firstRec < 0 || nRecs < 0 || (int64_t)firstRec + nRecs > (int64_t)maxRecs) v = kFrameRange;
                    else {
                        for (int i = firstRec; i < firstRec + nRecs; ++i) {
                            const int st = status[i];
                            if (st != 0) { v = kFrameBlock; bad = i; bst = st; break; }     // (0: PLZ4HIP_BLK_OK)
                            const int r = result[i];
                            if (r < 0 || r > dstCap) { v = kFrameRange; bad = i; break; }
                            sz += (uint64_t)r;
                            if (hashed) piece_update(c, dst + (int64_t)i * dstStride, r, l);
                        }
                        if (v < 0 && !complete) v = kFrameIncomplete;
                    }
                }
            }
            acc[I_] = c.a; pend[I_] = c.pend; fill[I_] = c.fill; size[I_] = sz;
            what[I_] = flg | hashed << 8;
            verdict[I_] = v; firstBad[I_] = bad; blockStatus[I_] = bst;
        })
        // the group's first lane gathers the four chains and the pending stripe
        LV(uint32_t, a1); LV(uint32_t, a2); LV(uint32_t, a3); LV(uint32_t, w1); LV(uint32_t, w2); LV(uint32_t, w3);
        LANES({ a1[I_] = SHFL(acc, (LANE & ~3) + 1); })
        LANES({ a2[I_] = SHFL(acc, (LANE & ~3) + 2); })
        LANES({ a3[I_] = SHFL(acc, (LANE & ~3) + 3); })
        LANES({ w1[I_] = SHFL(pend, (LANE & ~3) + 1); })
        LANES({ w2[I_] = SHFL(pend, (LANE & ~3) + 2); })
        LANES({ w3[I_] = SHFL(pend, (LANE & ~3) + 3); })
        LANES({
            const int64_t f = 16 * w + (LANE >> 2);
            if ((LANE & 3) == 0 && f < nFrames) {
                int v = verdict[I_];
                uint64_t sz = size[I_];
                uint32_t sum = 0;
                const uint32_t flg = what[I_] & 0xFFu;
                if (v != kFrameSkippable) {
                    if (what[I_] >> 8) {
                        sum = piece_sum(acc[I_], a1[I_], a2[I_], a3[I_], pend[I_], w1[I_], w2[I_], w3[I_], fill[I_], sz);
                        if (v < 0 && sum != wantSum[I_]) v = kFrameContentHash;
                    }
                    if (v < 0 && (flg & 8u) && sz != wantSz[I_]) v = kFrameContentSize;
                    if (v < 0) v = kFrameOk;
                } else sz = 0;
                FrameVerdict* const o = verdicts + f;
                o->contentSz = sz; o->contentSum = sum; o->status = v; o->firstBad = firstBad[I_]; o->blockStatus = blockStatus[I_];
                o->reserved[0] = 0; o->reserved[1] = 0;
            }
        })
    }
}

// The stream verdict over verdicts[0 .. nFrames): one wave, 64 entries a step; ballots for the first bad entry and the counts, a
// 64-bit scan for the bytes in front of and in it.  No atomics, no init kernel: it runs behind k_verify_frames on the same stream.
DEV void wave_verify_summary(const StreamIndex* info, const int maxFrames, const FrameVerdict* verdicts, StreamVerdict* sv)
{
    const int nFrames = max_(0, min_((int)UNI((uint32_t)info->nFrames), maxFrames));
    int64_t bytes = 0;
    int firstBadFrame = -1, badStatus = 0, nOk = 0, nSkip = 0;
    for (int base = 0; base < nFrames; base += 64) {
        LV(int, st); LV(uint64_t, sz);
        LANES({
            const bool in = LANE < nFrames - base;
            st[I_] = in ? verdicts[base + LANE].status : -1;
            sz[I_] = in ? verdicts[base + LANE].contentSz : 0;
        })
        nOk += __builtin_popcountll(BALLOT(st[I_] == kFrameOk));
        nSkip += __builtin_popcountll(BALLOT(st[I_] == kFrameSkippable));
        if (firstBadFrame < 0) {
            const uint64_t bad = BALLOT(st[I_] > kFrameSkippable);
            SCAN_INCL64(sz);
            const int last = bad ? ctz64(bad) : 63;
            bytes += (int64_t)RL(sz, last);
            if (bad) { firstBadFrame = base + last; badStatus = RL(st, last); }
        }
    }
    LANES({
        if (LANE == 0) {
            sv->contentBytes = bytes; sv->firstBadFrame = firstBadFrame; sv->status = badStatus; sv->nFrames = nFrames; sv->nOk = nOk;
            sv->nSkippable = nSkip; sv->reserved = 0;
        }
    })
}

}  // namespace plz4
