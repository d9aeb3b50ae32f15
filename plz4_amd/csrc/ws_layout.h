// One layout per device workspace: the size that is reserved and the offsets the pointers are bound from come out of the same takes.
// Host only, no HIP call: pure functions of a call's shape.  Included behind the device .inl files whose element types and stride
// helpers it uses (plz4hip.hip; tests/emu/emu_ws_layout.cpp compiles it with g++ -DPLZ4_EMU).
#pragma once
#include <vector>

namespace plz4 {

inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// A running offset.  take<T>(count, align): the array's offset; the next one starts `count` elements further on, rounded up to
// `align` bytes (256 unless the arrays are packed).  per_block: an array of `each` elements for every one of `blocks` blocks, which
// also counts towards what one block more costs.  log (tests): every take as it was made.
struct WsTake { size_t off, count, size, align; };
struct Carver {
    std::vector<WsTake>* log = nullptr;
    size_t at = 0, perBlock = 0;
    template <class T> size_t take(size_t count, size_t align = 256)
    {
        const size_t off = at;
        at = off + round_up(count * sizeof(T), align);
        if (log) log->push_back({off, count, sizeof(T), alignof(T)});
        return off;
    }
    template <class T> size_t per_block(size_t blocks, size_t each, size_t align = 256)
    {
        perBlock += each * sizeof(T);
        return take<T>(blocks * each, align);
    }
};

// ---------------------------------------------------------------------------------------------------- group sizing
// Blocks per group when nb blocks run in groups of at most grp, all of equal size.
inline int equal_groups(int64_t nb, int64_t grp) { const int64_t n = (nb + grp - 1) / grp; return (int)((nb + n - 1) / n); }

// Reserve; refused -> half the group; below one block -> give up.  reserve(per, &refused) returns 0 or the call's error, which ends
// the loop and is handed on in *rc.  Returns the blocks per group that were granted, 0 when not even one block was.
template <class Reserve> int fit_groups(int nb, int64_t grp, bool halveUp, Reserve&& reserve, int* rc)
{
    *rc = 0;
    while (grp >= 1) {
        const int per = equal_groups(nb, grp);
        bool refused = false;
        if ((*rc = reserve(per, &refused)) != 0) return 0;
        if (!refused) return per;
        if (grp == 1) break;
        grp = halveUp ? (grp + 1) / 2 : grp / 2;
    }
    return 0;
}

// What an HC call may take for its per-block workspaces (chains, lists, search results) when PLZ4HIP_HC_BUDGET_GIB does not say:
// a quarter of what is free, at most 64 GiB.  A library call that by default walks off with most of the card is not a drop-in
// (round 2 took three quarters); callers that own the GPU raise the budget, and plz4hip_ctx_trim gives the memory back.  More
// blocks per group is faster for these kernels (they live on blocks in flight), so a dedicated machine should set it.
inline size_t hc_default_budget(size_t freeBytes) { const size_t q = freeBytes / 4, cap = (size_t)64 << 30; return q < cap ? q : cap; }

// ... of what is free and whatever the ctx holds already, unless PLZ4HIP_HC_BUDGET_GIB (budgetGiB >= 1) says otherwise
inline size_t hc_budget(size_t freeB, size_t held, long budgetGiB)
{
    size_t budget = hc_default_budget(freeB + held);
    if (budgetGiB >= 1) budget = (size_t)budgetGiB << 30;
    return budget < held ? held : budget;
}

// The first guess of a level-12 / lazy call's group: what the budget holds, or PLZ4HIP_HC12_GROUP (group >= 1), within [1, nb].
inline int64_t hc_first_group(size_t freeB, size_t held, long budgetGiB, int group, size_t perBlock, int nb)
{
    int64_t grp = (int64_t)(hc_budget(freeB, held, budgetGiB) / perBlock);
    if (group >= 1) grp = group;
    if (grp < 1) grp = 1;
    return grp > nb ? nb : grp;
}

// Level 1: half of what is free (PLZ4HIP_L1_BUDGET_GIB, then _MIB, >= 1: that much), 64 bytes per block for the arrays' rounding.
// May be 0: not even one block.
inline int64_t l1_first_group(size_t freeB, size_t held, long budgetGiB, long budgetMiB, size_t perBlock, int nb)
{
    size_t budget = (freeB + held) / 2;
    if (budgetGiB >= 1) budget = (size_t)budgetGiB << 30;
    if (budgetMiB >= 1) budget = (size_t)budgetMiB << 20;
    if (budget < held) budget = held;
    const int64_t grp = (int64_t)(budget / (perBlock + 64));
    return grp > nb ? nb : grp;
}

// ---------------------------------------------------------------------------------------------------- level 1 (launch_l1)
// [SeqInfo per][chunk bytes per x maxChunks][chunk offsets likewise][records 8 B x seqStride][bk 1 B x seqStride][l1x: FxlBlk per]
struct L1Layout { size_t seqStride; int maxChunks; size_t perBlock, offInfo, offChunkBytes, offChunkOff, offSeq, offBk, offBlk, total; };
inline L1Layout l1_layout(int per, int maxLen, bool l1x, std::vector<WsTake>* log = nullptr)
{
    L1Layout L{};
    L.seqStride = round_up((size_t)(maxLen > 0 ? maxLen : 0) / 4 + 3, 64);     // + the dump entry (lz4_seq_device.inl)
    L.maxChunks = (int)((L.seqStride + kSeqChunk - 1) / kSeqChunk);
    Carver c{log};
    const size_t n = (size_t)per;
    L.offInfo = c.per_block<SeqInfo>(n, 1);
    L.offChunkBytes = c.per_block<uint32_t>(n, (size_t)L.maxChunks);
    L.offChunkOff = c.per_block<uint32_t>(n, (size_t)L.maxChunks);
    L.offSeq = c.per_block<uint64_t>(n, L.seqStride, 8);
    L.offBk = c.per_block<uint8_t>(n, L.seqStride, 8);
    if (l1x) L.offBlk = c.per_block<FxlBlk>(n, 1, 1);                           // (the bulk route: behind the group's records)
    L.perBlock = c.perBlock; L.total = c.at;
    return L;
}

// ---------------------------------------------------------------------------------------------------- few-block parses (c->fx, c->mx)
// [PieceMeta per piece][state in][states out x 2][records recStride per piece][hist: FxlBlk per block]; a state: tabWords words
// (kFxTab: level 1's table, 16 KiB; kMxTab: level 2's two tables, 128 KiB)
struct PieceLayout { size_t offMeta, offIn, offOut, offRec, offBlk, total; };
inline PieceLayout piece_layout(int per, int P, int recStride, int tabWords, bool hist, std::vector<WsTake>* log = nullptr)
{
    PieceLayout L{};
    Carver c{log};
    const size_t nP = (size_t)per * (size_t)P;
    L.offMeta = c.take<PieceMeta>(nP);
    L.offIn = c.take<uint32_t>(nP * (size_t)tabWords, 4);
    L.offOut = c.take<uint32_t>(2 * nP * (size_t)tabWords, 4);
    L.offRec = c.take<uint64_t>(nP * (size_t)recStride, 8);
    L.offBlk = c.at;
    if (hist) L.offBlk = c.take<FxlBlk>((size_t)per);
    L.total = c.at;
    return L;
}

// ---------------------------------------------------------------------------------------------------- HC levels 3..12 (c->h12)
// Level 12 on independent blocks without dictionary runs in three phases per group of blocks (lz4hc12_device.inl):
// chain -> search results -> parser.  Per block the group workspace holds the chain (2 B per position) and F (8 B per position).
// [0, 256): the error flag (zeroed when the workspace is allocated, sticky); the chains start behind it.  ws: the parse waves' global
// price-table slots.  info / chunk*: the emit stage's small arrays (levels 3..9); rec ... pieces: segments (lazy).
constexpr int kLzMaxSegs = 512;
struct HcLayout { int64_t chainStride, fStride, recStride; int maxChunks, group; size_t perBlock;
                  size_t offErr, offChain, offRank, offList, offOffsets, offF, offWs, offInfo, offChunkB, offChunkO,
                         offRec, offBridge, offMeta, offStarts, offPieces, total; };
inline HcLayout hc_layout(int group, int maxLen, bool lazy, bool needF, int parseWaves, std::vector<WsTake>* log = nullptr)
{
    HcLayout L{};
    L.group = group;
    L.chainStride = (int64_t)round_up((size_t)maxLen + 1, 1024);
    L.fStride = (int64_t)round_up((size_t)(maxLen > 11 ? maxLen - 11 : 1), 64);
    if (!needF) L.fStride = (int64_t)round_up((size_t)maxLen / 4 + 64, 64);     // no search results there: only the block's final records
    L.maxChunks = (int)((round_up((size_t)maxLen / 4 + 3, 64) + kSeqChunk - 1) / kSeqChunk);
    L.recStride = (int64_t)round_up((size_t)maxLen / 4 + (size_t)kLzMaxSegs * 80, 64);
    Carver c{log};
    const size_t n = (size_t)group;
    L.offErr = c.take<int32_t>(1);
    L.offChain = c.per_block<uint16_t>(n, (size_t)L.chainStride);
    L.offRank = c.per_block<uint32_t>(n, (size_t)L.chainStride);
    L.offList = c.per_block<uint32_t>(n, (size_t)L.chainStride + 8);
    L.offOffsets = c.per_block<uint32_t>(n, (size_t)kHcHashEntries);
    L.offF = c.per_block<Hc12F>(n, (size_t)L.fStride);
    L.offWs = c.take<uint8_t>((size_t)parseWaves * kHc12WsGlobalBytes);
    L.offInfo = c.per_block<SeqInfo>(n, 1);
    L.offChunkB = c.per_block<uint32_t>(n, (size_t)L.maxChunks);
    L.offChunkO = c.per_block<uint32_t>(n, (size_t)L.maxChunks);
    L.offRec = c.at;
    if (lazy) {
        L.offRec = c.per_block<uint64_t>(n, (size_t)L.recStride);
        L.offBridge = c.per_block<uint64_t>(n, (size_t)L.recStride);
        L.offMeta = c.per_block<LzSegMeta>(n, kLzMaxSegs);
        L.offStarts = c.per_block<uint64_t>(n, (size_t)kLzMaxSegs * kLzStarts);
        L.offPieces = c.per_block<LzPiece>(n, 2 * kLzMaxSegs);
    }
    L.perBlock = c.perBlock; L.total = c.at;
    return L;
}

// ---------------------------------------------------------------------------------------------------- lists in pieces (c->hb)
// [counts per (block, piece, hash)][first list slot per (block, piece, hash)]: 2 x 128 KiB per piece (lz4hc_lists_device.inl)
struct HbLayout { size_t pieceStride, offCnt, offSlot, total; };            // pieceStride: entries per piece
inline HbLayout hb_layout(int per, int P, std::vector<WsTake>* log = nullptr)
{
    HbLayout L{};
    L.pieceStride = (size_t)kHcHashEntries;
    Carver c{log};
    const size_t nP = (size_t)per * (size_t)P;
    L.offCnt = c.take<uint32_t>(nP * L.pieceStride);
    L.offSlot = c.take<uint32_t>(nP * L.pieceStride);
    L.total = c.at;
    return L;
}

// ------------------------------------------------------------------------- HC chain / lists up front (c->h12, the one-thread parsers)
// [error flag 256][chain 2 B per position][lists: rank 4 B][list 4 B, + 8][offsets per hash].  What is reserved is not the sum of the
// takes but slack + per x perBlock: the flag and a 256-byte rounding of each of the four arrays.
struct HcPreLayout { int64_t stride; size_t perBlock, slack, offChain, offRank, offList, offOffsets, total; };
inline HcPreLayout hc_pre_layout(int per, int maxLen, bool lists, std::vector<WsTake>* log = nullptr)
{
    HcPreLayout L{};
    L.stride = (int64_t)round_up((size_t)maxLen + 1, 1024);
    L.slack = 256 + 4 * 256;
    Carver c{log};
    const size_t n = (size_t)per;
    c.take<int32_t>(1);
    L.offChain = c.per_block<uint16_t>(n, (size_t)L.stride);
    if (lists) {
        L.offRank = c.per_block<uint32_t>(n, (size_t)L.stride);
        L.offList = c.per_block<uint32_t>(n, (size_t)L.stride + 8);
        L.offOffsets = c.per_block<uint32_t>(n, (size_t)kHcHashEntries);
    }
    L.perBlock = c.perBlock; L.total = L.slack + n * L.perBlock;
    return L;
}

// Blocks per launch, groups of equal size, in `room` bytes (0: not one); PLZ4HIP_HC_GROUP (group >= 1) only ever lowers it.
inline int hc_pre_group(size_t room, const HcPreLayout& one, int group, int nb)
{
    int64_t g = room > one.slack ? (int64_t)((room - one.slack) / one.perBlock) : 0;
    if (group >= 1 && group < g) g = group;
    if (g < 1) return 0;
    return equal_groups(nb, g > nb ? nb : g);
}

// Which of the two a call gets.  A group has to keep the chip busy: below 2048 blocks in flight the lists lose to the chain alone over
// more blocks at levels 4..9; the optimal parser's levels gain an order of magnitude and take them in any case.
struct HcPrePlan { int perLists, perChain; bool lists; };
inline HcPrePlan hc_pre_plan(size_t freeB, size_t held, long budgetGiB, int group, bool listsOff, int level, int nb, int maxLen)
{
    HcPrePlan p{};
    const size_t budget = hc_budget(freeB, held, budgetGiB);
    p.perLists = (level >= 4 && !listsOff) ? hc_pre_group(budget, hc_pre_layout(1, maxLen, true), group, nb) : 0;
    p.perChain = hc_pre_group(budget, hc_pre_layout(1, maxLen, false), group, nb);
    p.lists = p.perLists >= 1 && (p.perLists == nb || p.perLists >= (level >= 10 ? 256 : 2048) || p.perChain < 1);
    return p;
}

// ---------------------------------------------------------------------------------------------------- few-block decode (c->dx)
// [T 8 B x tStride][pointers 4 B x pStride][units maxSeg][DxInfo] [records: source offset, length, checksum verdict]
// [hist: first, chain, good, moved x rounds + 1] [grouped: one word per chain].  wb: the blocks the regions are sized for (the call, or
// the largest group); nb: the blocks of the group that is bound, whose record and link arrays are packed by its own count.
struct DxLayout { size_t tStride, pStride; int maxSeg; size_t offT, offPtr, offUnits, offInfo, offSrcOff, offLen, offHashBad,
                  offFirst, offChain, offGood, offMoved, offDead, total; };
inline DxLayout dx_layout(int wb, int nb, int64_t maxIn, int64_t maxOut, bool hist, bool records, int nChGrouped, std::vector<WsTake>* log = nullptr)
{
    DxLayout L{};
    L.tStride = dx_t_stride(maxIn); L.pStride = dx_ptr_stride(maxOut); L.maxSeg = dx_max_seg(maxIn);
    Carver c{log};
    const size_t w = (size_t)wb;
    L.offT = c.take<uint64_t>(w * L.tStride);
    L.offPtr = c.take<uint32_t>(w * L.pStride);
    L.offUnits = c.take<DxUnit>(w * (size_t)L.maxSeg);
    L.offInfo = c.take<DxInfo>(w);
    const auto rec = [&](Carver& r, size_t n) { L.offSrcOff = r.take<int64_t>(n, 8); L.offLen = r.take<int32_t>(n, 4); L.offHashBad = r.take<int32_t>(n, 4); };
    const auto link = [&](Carver& r, size_t n) { L.offFirst = r.take<int32_t>(n, 4); L.offChain = r.take<int32_t>(n, 4); L.offGood = r.take<int32_t>(n, 4);
                                                 L.offMoved = r.take<uint32_t>(n * (kDxlMaxRounds + 1), 4); };
    // a region: as long as its arrays are for wb blocks, the arrays packed for nb
    const auto region = [&](auto&& arrays, bool bound) {
        Carver sized{nullptr, c.at}; arrays(sized, w);
        Carver packed{bound ? log : nullptr, c.at}; arrays(packed, (size_t)nb);
        c.at += round_up(sized.at - c.at, 256);
    };
    region(rec, records);
    if (!records) L.offSrcOff = L.offLen = L.offHashBad = 0;
    if (hist) region(link, true);
    L.offDead = c.at;
    if (nChGrouped > 0) L.offDead = c.take<int32_t>((size_t)nChGrouped);
    L.total = c.at;
    return L;
}

// ---------------------------------------------------------------------------------------------------- raw blocks above 4 MiB (c->dx)
// [T][pointers][units][DxInfo][group tables 8 B x kDxSeg per group][entries per group][listed runs][DxbInfo]
struct DxbLayout { size_t tStride, pStride, tgStride; int maxSeg, groups, room; size_t offT, offPtr, offUnits, offInfo, offTG, offEnt, offRuns, offBi, total; };
inline DxbLayout dxb_layout(int nb, int64_t maxIn, int64_t maxOut, int G, int thr, std::vector<WsTake>* log = nullptr)
{
    DxbLayout L{};
    L.maxSeg = dx_max_seg(maxIn); L.groups = dxb_groups(L.maxSeg, G); L.room = dxb_run_room(maxIn, maxOut, thr);
    L.tStride = dx_t_stride(maxIn); L.pStride = dxb_ptr_stride(maxOut); L.tgStride = (size_t)L.groups * kDxSeg;
    Carver c{log};
    const size_t w = (size_t)nb;
    L.offT = c.take<uint64_t>(w * L.tStride);
    L.offPtr = c.take<uint32_t>(w * L.pStride);
    L.offUnits = c.take<DxUnit>(w * (size_t)L.maxSeg);
    L.offInfo = c.take<DxInfo>(w);
    L.offTG = c.take<uint64_t>(w * L.tgStride);
    L.offEnt = c.take<DxbEntry>(w * (size_t)L.groups);
    L.offRuns = c.take<DxRun>(w * (size_t)L.room);
    L.offBi = c.take<DxbInfo>(w);
    L.total = c.at;
    return L;
}

// ---------------------------------------------------------------------------------------------------- host staging (a slot's buffers)
// Layout of one chunk in a slot (same offsets in the pinned host buffer and in the device buffer):
//   [srcLen n][dstCap n][result n][status n][outLen n][outOff n+1 (int64)] | inputs at inStride | outputs at outStride
// and, device only, the outputs once more back to back (compacted) -- that is what travels back over PCIe.  A call with a dictionary
// or linked blocks has behind them: [prevTail 64 KiB][per chain: window 2 x 64 KiB][windowLen per chain][chainFirst]
// gap: bytes of scratch in front of every input block (HC with a dictionary / linked blocks: the external segment goes there)
struct Staging { size_t offA, offB, offRes, offSt, offLen, offOff, offIn, offOut, offPack, offExtra, offWin, offWinLen, offFirst, winBytes, total;
                 int64_t inStride, outStride; size_t gap; };
inline Staging staging_layout(int n, int maxIn, int maxOut, size_t gap, bool dictMode, int nCh, std::vector<WsTake>* log = nullptr)
{
    Staging s{};
    s.gap = gap;
    s.inStride = (int64_t)round_up((size_t)maxIn + gap + 16, 16);
    s.outStride = (int64_t)round_up((size_t)maxOut + 16, 16);
    Carver c{log};
    const size_t nn = (size_t)n;
    s.offA = c.take<int32_t>(nn); s.offB = c.take<int32_t>(nn); s.offRes = c.take<int32_t>(nn); s.offSt = c.take<int32_t>(nn);
    s.offLen = c.take<int32_t>(nn);
    s.offOff = c.take<int64_t>(nn + 1);
    s.offIn = c.take<uint8_t>(nn * (size_t)s.inStride, 1);
    s.offOut = c.take<uint8_t>(nn * (size_t)s.outStride, 1);
    s.offPack = c.take<uint8_t>(nn * (size_t)s.outStride, 1);
    s.offExtra = c.at;
    if (dictMode) {
        s.offExtra = c.take<uint8_t>(65536, 1);
        s.offWin = c.take<uint8_t>((size_t)nCh * 131072, 1);
        s.offWinLen = c.take<int32_t>((size_t)nCh);
        s.offFirst = c.take<int32_t>((size_t)nCh + 1);
        s.winBytes = c.at - s.offWin;
    }
    s.total = c.at;
    return s;
}

}  // namespace plz4
