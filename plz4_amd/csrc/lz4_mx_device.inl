// lz4_mx_device.inl -- the level-2 parse (hc_mid_parse, lz4hc_lazy_device.inl) of a call of few blocks cut across the whole chip:
// lz4_fx_device.inl's design for LZ4MID_compress.  Independent blocks (MxFlavour), and blocks with history outside the block -- a
// dictionary, linked blocks -- behind their external segment (MxlFlavour).
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

// ... on a block BEHIND an external segment of pfx bytes (a linked block, a block > 4 KiB under an attached dictionary: hc_mid_parse's
// kD).  Positions are the parser's: the segment's first byte is 0, the block's first byte pfx (base()); records and lastAnchor are
// block-relative.  `src` is the block; the segment lies right in front of it.  Piece 0 -- and every piece whose start - warm is not
// beyond the block's first byte -- walks from the block's start over zeroed tables primed over the segment (exact); a guessed start
// begins over zeroed tables, primed as well while it lies within 64 KiB of the block's first byte (mid_guess_primes); a state handed
// on is installed as it is.  Why a restart is exact behind
// a segment as well: lz4hc_lazy_device.inl, at hc_mid_parse.
struct MxlFlavour : MxFlavour {
    int pfx;
    DEVM explicit MxlFlavour(int pfx_) : pfx(pfx_) {}
    DEVM int base() const { return pfx; }
    DEVM bool guessed(int p0) const { return p0 > pfx; }
    DEVM int walk(const uint8_t* __restrict__ blk, int n, uint64_t* rec, int recStride, int* lastAnchor, MidRun& run, uint32_t* work) const
    {
        const int ns = hc_mid_parse<true, uint32_t*, MidNoCtx, true>(blk, n, work, work + 16384, rec, lastAnchor, pfx, MidNoCtx(), &run);
        return run.over ? recStride : ns;
    }
};

}  // namespace plz4
