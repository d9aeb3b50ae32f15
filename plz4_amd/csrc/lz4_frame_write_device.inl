// lz4_frame_write_device.inl -- whole LZ4 frames around a block section that lies in device memory: the reference writer's header
// (header/write.go:23-73), end mark and content checksum (trailer/trailer.go, blk/frame.go) as device code, for
// plz4hip_dev_write_frames.  The dual of lz4_frame_verify_device.inl: the same walk over a frame's pieces, but over the plaintext the
// encoder read, and the sum is stored where the verifier compares it.
//
// The encoder left `body` and recOff[0 .. nBlocks]; frame f of the stream owns records [f * k, min((f + 1) * k, nBlocks)) and lies
// at f * (H + T) + recOff[f * k]: every place in the stream is host arithmetic plus ONE recOff entry, so nothing is scanned.
//
//   * wave_frame_edges: sixteen frames to a wavefront, lane 4g + l owning accumulator l of frame 16w + g (the layout of
//     wave_verify_frames).  Every lane walks its frame's records itself -- the range tests, the size word, then the block's plaintext
//     into piece_update -- so nothing crosses lanes until the frame's end, where the group's first lane gathers the four chains with
//     SHFL and stores header, end mark, sum and the 64-byte table entry.  The outRecOff entries go out from the walk, record
//     first + j by lane j & 3 of the group.
//   * wave_frame_move: record i goes to out + outRecOff[i], 16 bytes a lane and step, unaligned on both sides; every wave derives
//     the verdict on the room and on its own record again before it touches a byte.
//   * wave_frame_summary: one wave folds the table's findings into info.
//   * no LDS, no workspace, no atomics, no init kernel.  A frame with a bad record is marked in its table entry:
//     status = -1 - (that record's index), where a written frame has PLZ4HIP_BODY_END_MARK (0); the summary folds those.
//
// Every write to `out` is tested against outCap by the one who writes, in 64 bits, whatever the tables hold.
#pragma once
#include "lz4_frame_verify_device.inl"

namespace plz4 {

// == PLZ4HIP_WRITE_* of include/plz4hip.h; plz4hip.hip asserts it
enum : int { kWriteOk = 0, kWriteNoRoom = 1, kWriteRecord = 2 };

struct WriteInfo {                                           // == plz4hip_write_info
    int64_t end;
    int32_t nFrames, nRecs, status, firstBadRec;
    int32_t reserved[2];
};

// what the host worked out for the call (by value into every kernel).  k: records per frame, >= 1 (one frame: max(nBlocks, 1));
// H, T: a header's and a trailer's bytes; flg, bd: the header's FLG and BD bytes.
struct FrameWriteGeom {
    int64_t  srcBytes, srcStride, bodyBytes, outCap, k;
    int32_t  bsz, nBlocks, nFrames, H, T, bck;
    uint32_t flg, bd, dictId;
    int32_t  pad;
};

// The host arithmetic of the call (GEOMETRY and BYTES of the header's table) for arguments that passed its checks -- host code, here so
// that the launcher and the lane emulation share it.  bsz: one of the four block sizes.
static inline FrameWriteGeom frame_write_geom(const int bsz, const bool bck, const bool linked, const bool cck, const bool csize, const bool hasDict,
                                              const uint32_t dictId, const int64_t srcBytes, const int64_t srcStride, const int64_t bodyBytes,
                                              const int blocksPerFrame, const int64_t outCap)
{
    FrameWriteGeom g{};
    int id = 4;
    while (id < 7 && bsz != 65536 << 2 * (id - 4)) ++id;
    const int64_t nb = srcBytes / bsz + (srcBytes % bsz != 0);
    g.srcBytes = srcBytes; g.srcStride = srcStride; g.bodyBytes = bodyBytes; g.outCap = outCap;
    g.bsz = bsz; g.nBlocks = (int32_t)nb;
    g.k = blocksPerFrame ? blocksPerFrame : (nb ? nb : 1);
    const int64_t nf = (nb + g.k - 1) / g.k;
    g.nFrames = nf ? (int32_t)nf : 1;
    g.H = 7 + (csize ? 8 : 0) + (hasDict ? 4 : 0);
    g.T = 4 + (cck ? 4 : 0);
    g.bck = bck ? 1 : 0;
    g.flg = 0x40u | (linked ? 0u : 0x20u) | (bck ? 0x10u : 0u) | (csize ? 8u : 0u) | (cck ? 4u : 0u) | (hasDict ? 1u : 0u);
    g.bd = (uint32_t)id << 4;
    g.dictId = hasDict ? dictId : 0u;
    return g;
}

// is there a stream end, and room for it?  kWriteOk: E <= outCap; kWriteNoRoom: E > outCap; kWriteRecord: recOff[nBlocks] lies
// outside [0, bodyBytes], E = -1 (then the last record at least is a bad one).  No record: recOff is not read.
DEV int frame_write_room(const FrameWriteGeom& g, const int64_t* recOff, int64_t& E)
{
    const int64_t tail = g.nBlocks ? (int64_t)UNI((uint64_t)recOff[g.nBlocks]) : 0;
    const int64_t edges = (int64_t)g.nFrames * (g.H + g.T);
    if (tail < 0 || tail > g.bodyBytes) { E = -1; return kWriteRecord; }
    E = edges + tail;
    return tail > g.outCap - edges ? kWriteNoRoom : kWriteOk;
}

// the record at body + [a, b): its bytes, or -1 for a bad one.  The size word is read only behind the range tests.
DEV int frame_write_record(const FrameWriteGeom& g, const uint8_t* body, const int64_t a, const int64_t b)
{
    const int64_t n = (int64_t)((uint64_t)b - (uint64_t)a);
    const int64_t edge = 4 + 4 * g.bck;
    bool ok = a >= 0 && b >= a && b <= g.bodyBytes && n >= edge;
    uint32_t w = 0;
    if (ok) w = ld32u(body + a);
    const int64_t size = (int64_t)(w & 0x7FFFFFFFu);
    ok = ok && size <= g.bsz && size + edge == n;
    return ok ? (int)n : -1;
}

// the frame header at p: H bytes.  The descriptor (FLG, BD, content size, dictionary id) as 16 little-endian bytes lo | hi; its
// checksum byte is the stream index's, word for word (sx_word, sx_byte: lz4_stream_index_device.inl).
DEV void frame_write_header(const FrameWriteGeom& g, uint8_t* p, const uint64_t contentSz)
{
    uint64_t lo = (uint64_t)g.flg | (uint64_t)g.bd << 8, hi = 0;
    int at = 2;
    if (g.flg & 8u) { lo |= contentSz << 16; hi = contentSz >> 48; at = 10; }
    if (g.flg & 1u) {
        if (at == 2) lo |= (uint64_t)g.dictId << 16;
        else         hi |= (uint64_t)g.dictId << 16;
        at += 4;
    }
    const int dlen = at;                                     // 2, 6, 10 or 14: whole words, then always two single bytes
    uint32_t h = 374761393u + (uint32_t)dlen;
    if (dlen >= 4)  h = sx_word(h, (uint32_t)lo);
    if (dlen >= 8)  h = sx_word(h, (uint32_t)(lo >> 32));
    if (dlen >= 12) h = sx_word(h, (uint32_t)hi);
    const int rest = 8 * (dlen & ~3);
    const uint32_t two = (uint32_t)((rest < 64 ? lo >> rest : hi >> (rest - 64)) & 0xFFFFu);
    h = sx_byte(sx_byte(h, two & 0xFFu), two >> 8);
    h ^= h >> 15; h *= 2246822519u; h ^= h >> 13; h *= 3266489917u; h ^= h >> 16;
    st32u(p, 0x184D2204u);
    for (int j = 0; j < dlen; ++j) p[4 + j] = (uint8_t)(j < 8 ? lo >> 8 * j : hi >> 8 * (j - 8));
    p[4 + dlen] = (uint8_t)(h >> 8);
}

// Wave `wave` of `nWaves`: frames 16w .. 16w + 15 for w = wave, wave + nWaves, ... while 16w < nFrames.  The rules: the table at
// plz4hip_dev_write_frames in include/plz4hip.h.
DEV void wave_frame_edges(const FrameWriteGeom& g, const uint8_t* src, const uint8_t* body, const int64_t* recOff, uint8_t* out,
                          FrameIndex* frames, int64_t* outRecOff, const int wave, const int nWaves)
{
    int64_t E;
    const int room = frame_write_room(g, recOff, E);
    if (room == kWriteNoRoom) return;                                       // (uniform over the whole grid)
    const int64_t HT = g.H + g.T;
    for (int64_t w = wave; 16 * w < g.nFrames; w += nWaves) {
        LV(uint32_t, acc); LV(uint32_t, pend); LV(uint32_t, fill); LV(int, firstBad);
        LANES({
            const int l = LANE & 3;
            const int64_t f = 16 * w + (LANE >> 2);
            PieceChain c;
            c.a = (l == 0) ? XP1 + XP2 : (l == 1) ? XP2 : (l == 2) ? 0u : 0u - XP1;
            c.pend = 0; c.fill = 0;
            int bad = -1;
            if (f < g.nFrames) {
                const int64_t first = f * g.k, last = min_<int64_t>(first + g.k, g.nBlocks);
                const int64_t shift = (f + 1) * g.H + f * g.T;
                int64_t a = first < last ? recOff[first] : 0;
                for (int64_t i = first; i < last; ++i) {
                    const int64_t b = recOff[i + 1];
                    if (((int)(i - first) & 3) == l) outRecOff[i] = (int64_t)((uint64_t)a + (uint64_t)shift);   // (a may be anything)
                    if (bad < 0) {
                        const int n = frame_write_record(g, body, a, b);
                        bad = n < 0 ? (int)i : bad;
                        if (n >= 0 && (g.flg & 4u))
                            piece_update(c, src + i * g.srcStride, (int)min_<int64_t>(g.bsz, g.srcBytes - i * g.bsz), l);
                    }
                    a = b;
                }
            }
            acc[I_] = c.a; pend[I_] = c.pend; fill[I_] = c.fill; firstBad[I_] = bad;
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
            if ((LANE & 3) == 0 && f < g.nFrames) {
                const int64_t first = f * g.k, last = min_<int64_t>(first + g.k, g.nBlocks);
                const int64_t from = g.nBlocks ? recOff[first] : 0, to = g.nBlocks ? recOff[last] : 0;
                const int64_t hdrOff = (int64_t)((uint64_t)(f * HT) + (uint64_t)from), end = (int64_t)((uint64_t)((f + 1) * HT) + (uint64_t)to);
                const uint64_t plain = (uint64_t)(min_<int64_t>(g.srcBytes, last * g.bsz) - first * g.bsz);
                const int bad = firstBad[I_];
                uint32_t sum = 0;
                if ((g.flg & 4u) && bad < 0)
                    sum = piece_sum(acc[I_], a1[I_], a2[I_], a3[I_], pend[I_], w1[I_], w2[I_], w3[I_], fill[I_], plain);
                if (room == kWriteOk && bad < 0 && end <= g.outCap) {       // (a written frame: hdrOff >= 0, its records in between)
                    frame_write_header(g, out + hdrOff, plain);
                    st32u(out + end - g.T, 0u);
                    if (g.flg & 4u) st32u(out + end - 4, sum);
                }
                FrameIndex* const e = frames + f;
                e->hdrOff = hdrOff; e->bodyOff = (int64_t)((uint64_t)hdrOff + (uint64_t)g.H); e->end = end;
                e->contentSz = (g.flg & 8u) ? plain : 0; e->dictId = (g.flg & 1u) ? g.dictId : 0u; e->contentSum = sum;
                e->firstRec = (int32_t)first; e->nRecs = (int32_t)(last - first); e->bsz = g.bsz;
                e->flags = (uint8_t)g.flg; e->blockDesc = (uint8_t)g.bd; e->kind = 0; e->nibble = 0;
                e->status = bad < 0 ? kBodyEndMark : -1 - bad; e->reserved = 0;
                if (f == g.nFrames - 1) outRecOff[g.nBlocks] = g.nBlocks ? (int64_t)((uint64_t)to + (uint64_t)((int64_t)g.nFrames * g.H + (int64_t)(g.nFrames - 1) * g.T)) : 0;
            }
        })
    }
}

// Record i, wave wv of the nWv that share it: 16 bytes a lane and step; the first of them moves the last n & 15 bytes one by one.
DEV void wave_frame_move(const FrameWriteGeom& g, const uint8_t* body, const int64_t* recOff, uint8_t* out, const int i, const int wv,
                         const int nWv)
{
    int64_t E;
    if (frame_write_room(g, recOff, E) != kWriteOk) return;
    const int64_t a = (int64_t)UNI((uint64_t)recOff[i]), b = (int64_t)UNI((uint64_t)recOff[i + 1]);
    const int n = frame_write_record(g, body, a, b);
    if (n < 0) return;
    const int64_t f = i / g.k;
    const int64_t at = a + (f + 1) * g.H + f * g.T;
    if ((int64_t)n > g.outCap - at) return;
    const uint8_t* const s = body + a;
    uint8_t* const d = out + at;
    const int full = n & ~15;
    LANES({
        for (int64_t p = ((int64_t)wv * 64 + LANE) * 16; p < full; p += (int64_t)nWv * 64 * 16) *(v16u_t*)(d + p) = *(const v16u_t*)(s + p);
    })
    if (wv == 0) LANES({ if (LANE < n - full) d[full + LANE] = s[full + LANE]; })
}

// info, by one wave behind the two: the verdict on the room from the same uniform values, else the lowest marked frame of the table.
DEV void wave_frame_summary(const FrameWriteGeom& g, const int64_t* recOff, const FrameIndex* frames, WriteInfo* info)
{
    int64_t E;
    const int room = frame_write_room(g, recOff, E);
    int firstBadRec = -1;
    if (room != kWriteNoRoom) {
        for (int64_t base = 0; base < g.nFrames && firstBadRec < 0; base += 64) {
            LV(int, st);
            LANES({ st[I_] = LANE < g.nFrames - base ? frames[base + LANE].status : 0; })
            const uint64_t bad = BALLOT(st[I_] < 0);
            if (bad) firstBadRec = -1 - RL(st, ctz64(bad));
        }
    }
    const int status = room != kWriteOk ? room : firstBadRec >= 0 ? kWriteRecord : kWriteOk;
    LANES({
        if (LANE == 0) {
            info->end = E; info->nFrames = g.nFrames; info->nRecs = g.nBlocks; info->status = status; info->firstBadRec = firstBadRec;
            info->reserved[0] = 0; info->reserved[1] = 0;
        }
    })
}

}  // namespace plz4
