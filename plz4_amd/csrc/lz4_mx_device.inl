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
// The rounds are lz4_fx_device.inl's, unchanged (one launch each, grid (pieces, blocks)):
//   round 1   piece 0 walks from the block's start (exact).  Piece k > 0 starts `warm` bytes early from a guessed state (anchor = ip
//             = start - warm, all-zero tables: what LZ4_initStreamHC leaves, every entry dead at any position), records the state it
//             reaches at its start (inAnchor / tabIn) and keeps the records from there.
//   round r   piece k runs again iff piece k-1 ran in round r-1, did not reach the block's end, and its exit state differs from
//             piece k's recorded entry state (same anchor, same live entries); it then starts from that exit state.
// Exit states are kept per round parity: round r reads r-1's and writes r's, so no piece waits for another; a piece walks INSIDE its
// exit-table slot (the working tables are in device memory anyway).  Piece i is exact after round i + 1: P rounds are always
// enough.  What differs from level 1 is the warm-up: 16 Ki slots per table for a 64 Ki-position window, so a wrong entry of a guessed
// start lives for a whole window, where level 1's 4 Ki-slot table overwrites it sixteen times (rounds measured).
//
// Records of a piece: those that start in [entry anchor, end) -- at most pb / 4 -- and nothing else: the warm-up's records are dropped
// (they wrap inside the first 64 entries), a piece that runs on past its end because no post-match state comes writes none on the
// way, an incompressible block is piece 0 alone with a handful, one match that spans many pieces is one record of the piece it
// starts in.  A block of at most one piece is a block of one piece; a block below kMinLength has no records at all.
#pragma once
#include "lz4hc_lazy_device.inl"
#include "lz4_fx_device.inl"

namespace plz4 {

DEV int mx_pieces(int n, int pb) { return max_(fx_pieces(n, pb), 1); }
static inline int mx_rec_stride_host(int pb) { return fx_rec_stride_host(pb); }

// two states at one anchor: same live entries of both tables (the parser's own test, lz4hc.c:578; dead ones never matter again)
DEV bool mx_same_state(const uint32_t* __restrict__ A, const uint32_t* __restrict__ B, int anchor)
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

// One wave: piece k of an independent block of n bytes in round `round` (1, 2, ...).  meta / tabIn: P entries of the block; tabOut:
// 2 x P states (parity major); rec: P x recStride records.  Returns 1 when it walked.
DEV int mx_piece(const uint8_t* __restrict__ src, int n, int k, int round, int pb, int warm, FxPiece* meta, uint32_t* tabIn, uint32_t* tabOut,
                 uint64_t* rec, int recStride)
{
    const int P = mx_pieces(n, pb);
    if (k >= P) return 0;
    const int par = round & 1, start = k * pb;
    FxPiece* const me = meta + k;
    uint32_t* const myIn = tabIn + (int64_t)k * kMxTab;
    uint32_t* const work = tabOut + ((int64_t)par * P + k) * kMxTab;
    MidRun run;
    run.entryAnchor = -1; run.primed = 0; run.cp = -1; run.cpTab = myIn; run.cpAnchor = -1;
    run.end = min_(n, start + pb); run.outAnchor = -1; run.seqCap = recStride - 1; run.fin = 0; run.over = 0;
    if (round == 1) {
        if (k > 0) {
            run.cp = start;
            if (start - warm > 0) run.entryAnchor = start - warm;          // (else from the block's start: exact)
        }
    } else {
        bool go = false;
        if (k > 0 && meta[k - 1].ran[par ^ 1] && !meta[k - 1].outFin[par ^ 1]) {
            const int a = meta[k - 1].outAnchor[par ^ 1];
            const uint32_t* T = tabOut + ((int64_t)(par ^ 1) * P + k - 1) * kMxTab;
            if (a != me->inAnchor || !mx_same_state(T, myIn, a)) {
                go = true;
                run.entryAnchor = a; run.primed = 1;
                LANES({ for (int i = LANE; i < kMxTab; i += 64) { const uint32_t v = T[i]; myIn[i] = v; work[i] = v; } })
                WAVE_FENCE();
            }
        }
        if (!go) {
            LANES({ if (LANE == 0) me->ran[par] = 0; })
            return 0;
        }
    }
    int lastAnchor = 0;
    int ns = hc_mid_parse<false, uint32_t*, MidNoCtx, true>(src, n, work, work + 16384, rec + (int64_t)k * recStride, &lastAnchor, 0, MidNoCtx(), &run);
    if (run.over) ns = recStride;                                          // (fails the block in the gather; an exact walk has room)
    const int inA = round == 1 ? (k > 0 ? run.cpAnchor : 0) : run.entryAnchor;
    const int runs = round == 1 ? 1 : me->runs + 1;
    WAVE_FENCE();
    LANES({
        if (LANE == 0) {
            me->inAnchor = inA; me->nseq = ns; me->fin = run.fin; me->lastAnchor = lastAnchor;
            me->runs = runs; me->lastRound = round;
            me->ran[par] = 1; me->outAnchor[par] = run.outAnchor; me->outFin[par] = run.fin;
        }
    })
    return 1;
}

// One wave: piece k's records into the block's record array, if the block's chain reaches it; the piece that reached the block's
// end writes the block's SeqInfo.  0: not in the chain, 1: in it, 2: the last of it.  The chain of pieces is laid out exactly as
// level 1's (a block always has a piece 0: fx_gather's kExt flavour counts pieces that way).
DEV int mx_gather(int n, int k, int pb, const FxPiece* __restrict__ meta, const uint64_t* __restrict__ rec, int recStride,
                  uint64_t* __restrict__ seq, int seqCap, SeqInfo* info)
{
    return fx_gather<true>(n, k, pb, meta, rec, recStride, seq, seqCap, info);
}

}  // namespace plz4
