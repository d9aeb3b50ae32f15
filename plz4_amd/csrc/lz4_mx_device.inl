// lz4_mx_device.inl -- the level-2 parse (hc_mid_parse, lz4hc_lazy_device.inl) of a call of few independent blocks cut across the
// whole chip: lz4_fx_device.inl's design for LZ4MID_compress.
//
// A level-2 block is one serial chain of dependent memory round trips: one wave walks it, however empty the chip is.  Here a block
// of up to 4 MiB is cut into pieces of `pb` bytes and every piece gets a wave of its own.
//
// Why a piece can be walked on its own: LZ4MID_compress inserts only the positions it searches, so its two tables depend on the walk;
// but right after a sequence is finished (the fills around the match made, anchor == ip: MidRun, lz4hc_lazy_device.inl) the rest of
// the walk depends on the anchor, the LIVE entries of the two tables and the input.  A walk restarted from such a post-match state
// gives exactly the records of the unbroken walk.  Piece k's entry state is the first post-match state at or beyond its start; its
// exit state the first one at or beyond its end -- which is piece k+1's entry state.
//
// The rounds, the parity of the exit states, the P-rounds argument and the gather: lz4_pieces_device.inl.  This flavour's guessed
// state is anchor = ip = start - warm over all-zero tables (what LZ4_initStreamHC leaves: every entry dead at any position), and a
// piece walks INSIDE its exit-state slot (the working tables are in device memory anyway).  What differs from level 1 is the
// warm-up: 16 Ki slots per table for a 64 Ki-position window, so a wrong entry of a guessed start lives for a whole window, where
// level 1's 4 Ki-slot table overwrites it sixteen times (rounds measured).
//
// Records of a piece: those that start in [entry anchor, end) -- at most pb / 4 -- and nothing else: the warm-up's records are dropped
// (they wrap inside the first 64 entries), a piece that runs on past its end because no post-match state comes writes none on the
// way, an incompressible block is piece 0 alone with a handful, one match that spans many pieces is one record of the piece it
// starts in.  A block of at most one piece is a block of one piece; a block below kMinLength has no records at all.
#pragma once
#include "lz4hc_lazy_device.inl"
#include "lz4_pieces_device.inl"

namespace plz4 {

// The level-2 flavour of piece_round (lz4_pieces_device.inl) on an independent block.  A state: both tables, kMxTab words.
struct MxFlavour {
    enum : int { kTab = kMxTab };
    static constexpr bool kPiece0 = true;
    typedef MidRun Run;
    DEVM int base() const { return 0; }
    DEVM bool guessed(int p0) const { return p0 > 0; }
    // two states at one anchor: same live entries of both tables (the parser's own test, lz4hc.c:578; dead ones never matter again)
    static DEVM bool same_state(const uint32_t* __restrict__ A, const uint32_t* __restrict__ B, int anchor)
    {
        const uint32_t idx = (uint32_t)anchor + kHcBase;
        LV(int, bad);
        LANES({
            int b = 0;
            for (int i = LANE; i < kMxTab; i += 64) {
                const uint32_t x = A[i], y = B[i];
                const bool lx = idx - x <= 65535u, ly = idx - y <= 65535u;
                b |= (int)((lx != ly) | (lx & (x != y)));
            }
            bad[I_] = b;
        })
        return BALLOT(bad[I_] != 0) == 0;
    }
    DEVM void arm(MidRun& run, uint32_t*) const { run.primed = 0; run.over = 0; }
    DEVM void from_start(MidRun&, uint32_t*) const {}
    DEVM void enter(MidRun& run, const uint32_t* T, uint32_t* myIn, uint32_t* work) const
    {
        run.primed = 1;
        LANES({ for (int i = LANE; i < kMxTab; i += 64) { const uint32_t v = T[i]; myIn[i] = v; work[i] = v; } })
        WAVE_FENCE();
    }
    DEVM int walk(const uint8_t* __restrict__ src, int n, uint64_t* rec, int recStride, int* lastAnchor, MidRun& run, uint32_t* work) const
    {
        const int ns = hc_mid_parse<false, uint32_t*, MidNoCtx, true>(src, n, work, work + 16384, rec, lastAnchor, 0, MidNoCtx(), &run);
        return run.over ? recStride : ns;                                  // (fails the block in the gather; an exact walk has room)
    }
};

// The flavour's round and gather by their earlier names and argument lists (kept for one revision only: the emulation sources of the revision before this
// one call them, and they are built against this tree whenever that revision's tests are run on it; nothing in this tree uses them --
// delete them with the next change)
DEV int mx_pieces(int n, int pb) { return piece_count<true>(n, pb); }
static inline int mx_rec_stride_host(int pb) { return piece_rec_stride(pb); }
DEV int mx_piece(const uint8_t* __restrict__ src, int n, int k, int round, int pb, int warm, PieceMeta* meta, uint32_t* tabIn, uint32_t* tabOut,
                 uint64_t* rec, int recStride)
{
    return piece_round(MxFlavour{}, src, n, k, round, pb, warm, meta, tabIn, tabOut, rec, recStride);
}
DEV int mx_gather(int n, int k, int pb, const PieceMeta* __restrict__ meta, const uint64_t* __restrict__ rec, int recStride,
                  uint64_t* __restrict__ seq, int seqCap, SeqInfo* info)
{
    return piece_gather<true>(n, k, pb, meta, rec, recStride, seq, seqCap, info);
}

}  // namespace plz4
