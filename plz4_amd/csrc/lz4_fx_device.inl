// lz4_fx_device.inl -- the level-1 parse (lz4_seq_device.inl) of a call of few blocks cut across the whole chip.
//
// A level-1 block is one serial chain: one wave parses it, however empty the chip is (1 x 4 MiB: ~70 ms).  Here a block of
// kFxMinLen..4 MiB (liblz4's byU32 tables, lz4.c:1389) is cut into pieces of `pb` bytes and every piece gets a wave of its own.
//
// Why a piece can be parsed on its own: right after a match (anchor = the match's end, lz4.c:1230-1233) the rest of liblz4's parse
// depends on the anchor, the LIVE part of the table -- an entry is live iff index + 65535 >= current (lz4.c:1090, :1274), and a dead
// entry never comes back -- and the input.  The catch-up stops at the anchor (lz4.c:1107-1109) and limitedOutput never feeds back.
// So a parse restarted from such a post-match state (anchor + table) gives exactly the records of the unbroken parse.  Piece k's
// entry state is the first post-match state at or beyond its start; its exit state the first one at or beyond its end -- which is
// piece k+1's entry state.
//
// The rounds, the parity of the exit states, the P-rounds argument, what a piece keeps and the gather: lz4_pieces_device.inl.  Here:
// the level-1 flavour of that protocol (a guessed state is every slot "position 0"), and what blocks with history need around it.
//
// Blocks with history outside the block (kExt: linked blocks, blocks under a dictionary context -- LZ4_compress_fast_continue as
// wave_encode_block_ext plays it) take the same rounds.  For the encoder they are no chain: block i needs the last <= 64 KiB of
// block i-1's PLAINTEXT, which the call's input holds, so every block and every piece starts at once.  fxl_prep (one wave per
// block) copies the segment right in front of the block and writes the table liblz4 starts the block with -- LZ4_loadDict over
// the tail, the dictionary context's table, or an empty one -- as piece 0's entry table (tabIn of piece 0, which the independent
// flavour never uses): piece 0 is exact in round 1 as before, pieces k > 0 guess as before, and the round rule, the parity of
// the exit states, the gather and the P-rounds argument are the independent flavour's.  Anchors are liblz4 indices (the parser's
// positions, lz4_seq_device.inl), records and lastAnchor block coordinates.  A block shorter than one piece is a block of one
// piece (these blocks take byU32 tables at any length); blocks <= 4 KiB under a dictionary context (two tables, kDictCtxLookup)
// are not this path's: they get an empty parse here and wave_encode_block_dict behind the emit stage.
#pragma once
#include "lz4_seq_device.inl"
#include "lz4_pieces_device.inl"

namespace plz4 {

enum : int { kFxTab = kHashBytes / 4, kFxMinLen = k64KLimit };

// The level-1 flavour of piece_round (lz4_pieces_device.inl).  A state: the 4 Ki-slot table.  kExt: src = the block (its segment in
// front of it, piece 0's entry table in tabIn: fxl_prep), bs = liblz4's index of its first byte; such a block always has a piece 0.
template <bool kExt = false> struct FxFlavour {
    enum : int { kTab = kFxTab };
    static constexpr bool kPiece0 = kExt;
    typedef FxRun Run;
    uint32_t* lds;             // 16 KiB owned by the wave
    int bs;
    DEVM int base() const { return kExt ? bs : 0; }
    DEVM bool guessed(int p0) const { return p0 >= base() + 64; }
    // two states at one anchor: same live entries (dead ones never matter again).  kExt: the flavour's shift, anchor = its index.
    static DEVM bool same_state(const uint32_t* __restrict__ A, const uint32_t* __restrict__ B, int anchor)
    {
        LV(int, bad);
        LANES({
            int b = 0;
            for (int i = LANE; i < kFxTab; i += 64) {
                const uint32_t x = A[i], y = B[i];
                const bool lx = (x >> (kExt ? 9 : 10)) + kMaxDist >= (uint32_t)anchor, ly = (y >> (kExt ? 9 : 10)) + kMaxDist >= (uint32_t)anchor;
                b |= (int)((lx != ly) | (lx & (x != y)));
            }
            bad[I_] = b;
        })
        return BALLOT(bad[I_] != 0) == 0;
    }
    DEVM void arm(FxRun& run, uint32_t* myOut) const { run.entryTab = nullptr; run.outTab = myOut; run.bs = base(); }
    DEVM void from_start(FxRun& run, uint32_t* tabIn) const
    {
        // the block's start: the table liblz4 starts it with.  (The pointer is said to be wave-uniform: as one of three values that
        // meet at the parser's "is there a table" question, the compiler otherwise keeps it in vector registers and fails on that question.)
        if (kExt && run.entryAnchor < 0) run.entryTab = (const uint32_t*)(uintptr_t)UNI((uint64_t)(uintptr_t)tabIn);
    }
    DEVM void enter(FxRun& run, const uint32_t* T, uint32_t* myIn, uint32_t*) const
    {
        run.entryTab = T;
        LANES({ for (int i = LANE; i < kFxTab; i += 64) myIn[i] = T[i]; })
    }
    DEVM int walk(const uint8_t* __restrict__ src, int n, uint64_t* rec, int, int* lastAnchor, FxRun& run, uint32_t*) const
    {
        const int ns = wave_parse_l1_tt<false, 2, true, kExt>(src - base(), base() + n, lds, rec, lastAnchor, nullptr, &run);
        if (kExt && n < kMinLength) run.fin = 1;                         // (no parse at all: the block is its last literals)
        return ns;
    }
};

// ---- blocks with history outside the block
struct FxlBlk { int32_t pfx, bs; };       // the segment's bytes (-1: not this path's block) and liblz4's index of the block's first byte

// One wave: the table liblz4 starts a block with under `mode` (kDict*, lz4_device.inl), into `lds` (16 KiB owned by the wave) as
// index << 9 | tag.  seg: the pfx bytes of the external segment (the previous block's tail or the dictionary; wherever they lie),
// dictTable: the dictionary context's LZ4_loadDictSlow table.  LZ4_loadDict over the segment, every 3rd position, the largest index
// per slot (lz4.c:1621-1628); the context's table, copied and tagged (lz4.c:1762-1768); else every slot "index 0".  Indices: the
// segment ends at 64 KiB, so delta = 64 KiB - pfx and every entry is 0 or a position of the segment.
DEV void fxl_table(const uint8_t* blk, int n, int mode, const uint8_t* __restrict__ seg, int pfx, const uint32_t* __restrict__ dictTable, uint32_t* lds)
{
    uint32_t e0 = 0;
    if (mode == kDictFreshPrefix && n >= 4) e0 = seq_tag(UNI(ld32u(blk))) & 0x1FFu;                      // "index 0" is the block's first byte
    const uint32_t delta = 65536u - (uint32_t)pfx;
    if (mode == kDictCtxCopy) {
        LANES({ for (int i = LANE; i < kFxTab; i += 64) {
            const uint32_t idx = dictTable[i];
            lds[i] = idx >= delta ? ((idx << 9) | (seq_tag(ld32u(seg + (idx - delta))) & 0x1FFu)) : 0u;
        } })
    } else {
        LANES({ for (int i = LANE; i < kFxTab; i += 64) lds[i] = e0; })
        if (mode == kDictLoad) {
            LDS_FENCE();
            const int cnt = (pfx - 8) / 3 + 1;
            LANES({ for (int k = LANE; k < cnt; k += 64) {
                const uint64_t s8 = ld64u(seg + 3 * k);
                lds_max(&lds[seq_hash<false>(s8)], (((uint32_t)(3 * k) + delta) << 9) | (seq_tag((uint32_t)s8) & 0x1FFu));
            } })
        }
    }
    LDS_FENCE();
}
// pfx / bs of a block under `mode` with a segment of segLen bytes
DEV FxlBlk fxl_blk_of(int mode, int segLen)
{
    FxlBlk b; b.pfx = 0; b.bs = 65536;
    if (mode == kDictCtxLookup) { b.pfx = -1; return b; }
    if (mode == kDictFreshPrefix) b.bs = 0;
    if (mode == kDictLoad || mode == kDictCtxCopy) b.pfx = segLen;
    return b;
}

// One wave: how block `blk` of n bytes starts under `mode` (seg / segLen: the previous block's tail or the dictionary).  The segment
// is copied right in front of the block -- the caller has left 64 KiB there; a segment that already lies there (the tail of the
// block before in contiguous plaintext) stays where it is: its neighbours read it meanwhile -- and the table liblz4 starts the
// block with (fxl_table) goes to tabG (16 KiB of global memory).  lds: 16 KiB owned by the wave.
DEV FxlBlk fxl_prep(uint8_t* blk, int n, int mode, const uint8_t* __restrict__ seg, int segLen, const uint32_t* __restrict__ dictTable,
                    uint32_t* __restrict__ tabG, uint32_t* lds)
{
    const FxlBlk b = fxl_blk_of(mode, segLen);
    if (b.pfx < 0) return b;
    fxl_table(blk, n, mode, seg, b.pfx, dictTable, lds);
    LANES({ for (int i = LANE; i < kFxTab; i += 64) tabG[i] = lds[i]; })
    if (b.pfx > 0 && seg != blk - b.pfx) wave_copy(blk - b.pfx, seg, b.pfx);
    return b;
}

// ---- many blocks with history outside the block: one wave per block, the whole block in ONE exact run of the kExt parse (the
// bulk flavour: no pieces, no rounds, no guessed states).  The segment is laid in front of the block unless it lies there already,
// the table liblz4 starts the block with is built straight into the wave's LDS table (fxl_table; no trip through global memory),
// and the parser takes it as it stands (kPrimed).  Records and lastAnchor are the staged path's, in the block's coordinates; the
// kSeg emit stage runs behind it with b->pfx.  Returns the records (kSeqEngineFailed: the run did not reach the block's end, which
// an exact run always does); a block that is not this path's (b->pfx < 0: <= 4 KiB under a dictionary context) has none.
DEV int l1x_block(uint8_t* blk, int n, int mode, const uint8_t* __restrict__ seg, int segLen, const uint32_t* __restrict__ dictTable,
                  uint64_t* __restrict__ rec, int seqCap, int* lastAnchor, FxlBlk* b, uint32_t* lds)
{
    *b = fxl_blk_of(mode, segLen);
    *lastAnchor = 0;
    if (b->pfx < 0) return 0;
    if (b->pfx > 0 && seg != blk - b->pfx) { wave_copy(blk - b->pfx, seg, b->pfx); WAVE_FENCE(); }
    fxl_table(blk, n, mode, blk - b->pfx, b->pfx, dictTable, lds);
    FxRun run;
    run.entryAnchor = -1; run.entryTab = nullptr; run.cp = -1; run.cpTab = nullptr; run.cpAnchor = -1;
    run.end = b->bs + n; run.outTab = nullptr; run.outAnchor = -1;          // (no post-match state lies at the block's end: nothing is saved)
    run.seqCap = seqCap; run.fin = 0; run.bs = b->bs;
    const int ns = wave_parse_l1_tt<false, 2, true, true, true>(blk - b->bs, b->bs + n, lds, rec, lastAnchor, nullptr, &run);
    if (n >= kMinLength && !run.fin) return kSeqEngineFailed;
    return ns <= seqCap ? ns : kSeqEngineFailed;
}

}  // namespace plz4
