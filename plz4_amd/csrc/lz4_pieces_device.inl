// lz4_pieces_device.inl -- the round protocol of the few-block parses: one block's serial parse cut into pieces, every piece on a
// wave of its own, re-run in rounds until every piece starts from the exact state its predecessor ends in.  Four flavours share
// it: levels 1 and 2, each on independent blocks and on blocks with history outside the block (lz4_fx_device.inl,
// lz4_mx_device.inl).  Those files say why, for their parser, a parse restarted from a post-match state (anchor + live
// table entries) gives exactly the records of the unbroken parse; everything below rests on that alone.
//
// A block of n bytes is cut into P pieces of `pb` bytes.  Piece k's entry state is the first post-match state at or beyond its
// start; its exit state the first one at or beyond its end -- which is piece k+1's entry state.
//
// Rounds (one launch each, grid (pieces, blocks)):
//   round 1   piece 0 parses from the block's start (exact).  Piece k > 0 starts `warm` bytes early from a guessed state (the
//             flavour's empty table), records the state it reaches at its start (inAnchor / tabIn) and keeps the records from there.
//   round r   piece k runs again iff piece k-1 ran in round r-1, did not reach the block's end, and its exit state differs from
//             piece k's recorded entry state (same anchor, same live entries); it then starts from that exit state.
// Parity: exit states are kept per round parity (tabOut[r & 1], ran / outAnchor / outFin [r & 1]): round r reads r-1's and writes
// r's, so no piece waits for another and the pieces of a round may run in any order.
// P rounds are always enough: piece 0 is exact after round 1 and, by induction, piece i after round i + 1 (its predecessor's exit
// state is final from round i on, and either equals the recorded entry state or starts the run that makes it so); a piece that is
// exact never runs again, and the rounds after the last change find nothing to do.
// A piece whose search runs past its end simply goes on to the next post-match state (or the block's end): the worst case is one
// exact walk of the rest of the block, as with one wave per block.
//
// What a piece keeps: its meta (PieceMeta), its entry state (tabIn), two exit states, and the records of its last run -- those that
// start at or beyond its entry anchor, at most recStride - 1 of them.  The gather (one wave per piece) lays the records of the chain
// 0, 1, ... up to the piece that reached the block's end out as the block's records.
//
// A flavour F supplies what differs:
//   kTab, kPiece0                words per state; whether a block always has a piece 0 (else a block of 0 bytes has no piece)
//   Run                          the parser's run descriptor (FxRun, MidRun)
//   base()                       the index of the block's first byte in the parser's coordinates
//   guessed(p0)                  round 1, piece k > 0: whether a start at p0 = start - warm is a guessed one (else the block's start)
//   same_state(A, B, anchor)     two states at one anchor: same live entries
//   arm(run, myOut)              the run descriptor's own fields, before the entry is decided (myOut: this round's exit-state slot)
//   from_start(run, tabIn)       round 1, once the start is decided
//   enter(run, T, myIn, myOut)   round r: install the predecessor's exit state T as the entry state
//   walk(...)                    the parse and its fix-ups; returns the records
#pragma once
#include "lz4_seq_device.inl"

namespace plz4 {

// per piece; fields [r & 1] belong to the round that wrote them
struct PieceMeta {
    int32_t inAnchor;          // the entry state the records are from (-1: none)
    int32_t nseq, fin, lastAnchor;      // last run: records, reached the block's end, where its last literals start
    int32_t runs, lastRound;
    int32_t ran[2], outAnchor[2], outFin[2];
};

template <bool kPiece0> DEV int piece_count(int n, int pb) { const int P = (n + pb - 1) / pb; return kPiece0 ? max_(P, 1) : P; }
// records a piece has room for (+ the dump entry): those of its own bytes, one that crosses its end, a batch of warm-up records
static inline int piece_rec_stride(int pb) { return ((pb / 4 + 80) + 7) & ~7; }

// One wave: piece k of a block of n bytes in round `round` (1, 2, ...).  meta / tabIn: P entries of the block; tabOut: 2 x P
// states (parity major); rec: P x recStride records.  Returns 1 when it parsed.
template <class F>
DEV int piece_round(const F& f, const uint8_t* __restrict__ src, int n, int k, int round, int pb, int warm, PieceMeta* meta, uint32_t* tabIn,
                    uint32_t* tabOut, uint64_t* rec, int recStride)
{
    const int P = piece_count<F::kPiece0>(n, pb);
    if (k >= P) return 0;
    const int bs = f.base();
    const int par = round & 1, start = bs + k * pb, nEnd = bs + n;
    PieceMeta* const me = meta + k;
    uint32_t* const myIn = tabIn + (int64_t)k * F::kTab;
    uint32_t* const myOut = tabOut + ((int64_t)par * P + k) * F::kTab;
    typename F::Run run;
    run.entryAnchor = -1; run.cp = -1; run.cpTab = myIn; run.cpAnchor = -1;
    run.end = min_(nEnd, start + pb); run.outAnchor = -1; run.seqCap = recStride - 1; run.fin = 0;
    f.arm(run, myOut);
    if (round == 1) {
        if (k > 0) {
            run.cp = start;
            const int p0 = start - warm;
            if (f.guessed(p0)) run.entryAnchor = p0;                     // (else from the block's start: exact)
        }
        f.from_start(run, tabIn);
    } else {
        bool go = false;
        if (k > 0 && meta[k - 1].ran[par ^ 1] && !meta[k - 1].outFin[par ^ 1]) {
            const int a = meta[k - 1].outAnchor[par ^ 1];
            const uint32_t* T = tabOut + ((int64_t)(par ^ 1) * P + k - 1) * F::kTab;
            if (a != me->inAnchor || !F::same_state(T, myIn, a)) {
                go = true;
                run.entryAnchor = a;
                f.enter(run, T, myIn, myOut);
            }
        }
        if (!go) {
            LANES({ if (LANE == 0) me->ran[par] = 0; })
            return 0;
        }
    }
    int lastAnchor = 0;
    const int ns = f.walk(src, n, rec + (int64_t)k * recStride, recStride, &lastAnchor, run, myOut);
    const int inA = round == 1 ? (k > 0 ? run.cpAnchor : bs) : run.entryAnchor;
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
// end writes the block's SeqInfo.  Returns 0: not in the chain, 1: in it, 2: the last of it.  (Counts beyond the room of a piece
// or of the block cannot come out of an exact parse; they would fail the block -- kSeqEngineFailed -- rather than be written.)
template <bool kPiece0>
DEV int piece_gather(int n, int k, int pb, const PieceMeta* __restrict__ meta, const uint64_t* __restrict__ rec, int recStride,
                     uint64_t* __restrict__ seq, int seqCap, SeqInfo* info)
{
    const int P = piece_count<kPiece0>(n, pb);
    if (k >= P) return 0;
    int off = 0;
    bool over = false;
    for (int j0 = 0; j0 < k; j0 += 64) {
        LV(int, c); LV(int, f);
        LANES({ const int j = j0 + LANE; c[I_] = j < k ? meta[j].nseq : 0; f[I_] = j < k ? meta[j].fin : 0; })
        if (BALLOT(f[I_] != 0)) return 0;
        over |= BALLOT(c[I_] >= recStride) != 0;
        SCAN_INCL(c);
        off += RL(c, 63);
    }
    const int ns = meta[k].nseq, fin = meta[k].fin;
    const bool room = !over && ns < recStride && off + ns <= seqCap;
    const uint64_t* r = rec + (int64_t)k * recStride;
    if (room) LANES({ for (int j = LANE; j < ns; j += 64) seq[off + j] = r[j]; })
    if (fin) {
        const int la = meta[k].lastAnchor;
        LANES({ if (LANE == 0) { SeqInfo inf; inf.nseq = room ? off + ns : kSeqEngineFailed; inf.lastAnchor = la; inf.total = 0; inf.stored = 0; *info = inf; } })
    }
    return fin ? 2 : 1;
}

}  // namespace plz4
