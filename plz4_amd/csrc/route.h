// Which kernels a call runs: the PLZ4HIP_* switches of the three launchers as typed values, and the route of a call as a pure function
// of its shape, the switches and what the reservations granted.  Host only, no HIP call, no getenv: the switches are read once per
// launcher call (read_*_switches, plz4hip.hip) and handed in.  Included behind ws_layout.h (plz4hip.hip; tests/emu/emu_routes.cpp
// compiles it with g++ -DPLZ4_EMU).  What a refusal means stays with the launcher: it says what was granted and is told the fallback.
#pragma once
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace plz4 {

constexpr int kUnset = INT_MIN;            // a switch that is not in the environment, where that differs from every value

// ---------------------------------------------------------------------------------------------------- few-block parses: the cut
// What a call that takes a few-block parse (lz4_pieces_device.inl) asks for before anything is reserved: pieces of `piece` bytes,
// guessed starts `warm` bytes early, P pieces per block of maxLen.
struct PieceCut { bool on; int piece, warm, P; };
inline PieceCut piece_cut(bool on, int maxLen, int pieceKiB, int warmKiB)
{
    PieceCut c{};
    c.on = on;
    if (on) { c.piece = pieceKiB << 10; c.warm = warmKiB << 10; c.P = (maxLen + c.piece - 1) / c.piece; }
    return c;
}
// PLZ4HIP_*_PIECE_KIB in 1..4096, PLZ4HIP_*_WARMUP_KIB in 0..4096; anything else leaves the default
template <class Get> void parse_piece_kib(Get&& get, const char* pieceName, const char* warmName, int* pieceKiB, int* warmKiB)
{
    if (const char* v = get(pieceName)) { const int x = (int)atol(v); if (x >= 1 && x <= 4096) *pieceKiB = x; }
    if (const char* v = get(warmName)) { const int x = (int)atol(v); if (x >= 0 && x <= 4096) *warmKiB = x; }
}

// ---------------------------------------------------------------------------------------------------- level 1 (launch_l1)
constexpr int  kFxMaxBlocks = 128;         // PLZ4HIP_FX_MAX_BLOCKS: the few-block level-1 parse up to this many blocks (profiles/fx_rate.json)
constexpr bool kL1xDefault = true;         // PLZ4HIP_L1X unset: the staged design (profiles/l1x_rate.json)
struct L1Switches {
    bool fused = false;                    // PLZ4HIP_L1_FUSED (set, whatever its value)
    int  fxLinked = kUnset;                // PLZ4HIP_FX_LINKED (0: history outside the block never takes the few-block parse)
    int  fxMax = kFxMaxBlocks;             // PLZ4HIP_FX_MAX_BLOCKS (0: off)
    int  fxPieceKiB = 64, fxWarmKiB = 64;  // PLZ4HIP_FX_PIECE_KIB in 1..4096, PLZ4HIP_FX_WARMUP_KIB in 0..4096
    int  l1x = kUnset;                     // PLZ4HIP_L1X (0: the one-kernel encoder; anything else: staged)
    bool oneWorkspace = false;             // PLZ4HIP_L1_WORKSPACES=1
    long budgetGiB = 0, budgetMiB = 0;     // PLZ4HIP_L1_BUDGET_GIB / _MIB (tests: force groups)
    bool noGate = false;                   // PLZ4HIP_EXP_NO_GATE
    int  duplexP = 1, duplexD = 1, duplexPrio = 3;   // PLZ4HIP_DUPLEX "P,D" (unparsable: 1,1), PLZ4HIP_DUPLEX_PRIO
};

// Whether a level-1 call of nb blocks with history outside the block (a dictionary, linked blocks) takes the few-block parse: at
// most fxMax blocks, the largest of kFxMinLen .. 4 MiB, and PLZ4HIP_FX_LINKED not 0.
inline bool fxl_wanted(const L1Switches& sw, int nb, int maxLen)
{
    if (sw.fxLinked == 0) return false;
    return nb <= sw.fxMax && maxLen >= kFxMinLen && maxLen <= kSeqMaxBlock && !sw.fused;
}
// Whether such a call of MANY blocks from device-resident plaintext takes the staged design (k_l1x_parse + the kSeg emit stage) or the
// one-kernel encoder.
inline bool l1x_on(const L1Switches& sw) { return !sw.fused && (sw.l1x == kUnset ? kL1xDefault : sw.l1x != 0); }

// mid: level 2's walk as the parser (launch_hc).  rider: a record decode shares the parse launch.  hist: history outside the block;
// l1x: ... from a device-resident entry point (the bulk staged route exists).  body: records straight into a frame body.
enum class L1Route { Fused, DictKernels, Parse, Duplex, Mid, Fx, Fxl, L1x, MidDeclined, NoMemBody };
struct L1Shape { int nb, maxLen; bool raw, mid, rider, hist, l1x, body, ctx; };     // ctx: a dictionary context of dictLen >= 8
// What the call asks for before anything is reserved.  staged: the group workspace (else the fused / dictionary kernels, which need
// none); fx: the few-block parse, with its cut (piece_cut).
struct L1Want { bool staged, fx; int piece, warm, P; PieceCut cut() const { return PieceCut{fx, piece, warm, P}; } };
inline L1Want l1_want(const L1Shape& k, const L1Switches& sw)
{
    L1Want w{};
    const bool inRange = k.maxLen > 0 && k.maxLen <= kSeqMaxBlock && !sw.fused;
    const bool fxl = fxl_wanted(sw, k.nb, k.maxLen);
    // history outside the block: staged for the few-block parse, and for the bulk route where the entry point has one
    w.staged = inRange && (!k.hist || fxl || (k.l1x && l1x_on(sw)));
    const bool fx = w.staged && !k.mid && !k.rider && k.nb <= sw.fxMax && k.maxLen >= kFxMinLen && k.maxLen <= kSeqMaxBlock && (!(k.hist || k.l1x) || fxl);
    const PieceCut c = piece_cut(fx, k.maxLen, sw.fxPieceKiB, sw.fxWarmKiB);
    w.fx = c.on; w.piece = c.piece; w.warm = c.warm; w.P = c.P;
    return w;
}
// The route, given what was granted: ws -- a group workspace of at least one block; fx -- the few-block parse's own.  Duplex is the
// first group's launch only (the others: Parse).
inline L1Route l1_route(const L1Shape& k, const L1Switches& sw, const L1Want& w, bool wsGranted, bool fxGranted)
{
    const L1Route dict = k.body ? L1Route::NoMemBody : L1Route::DictKernels;
    if (!w.staged || !wsGranted) return k.hist ? dict : k.body ? L1Route::NoMemBody : k.mid ? L1Route::MidDeclined : L1Route::Fused;
    const bool fx = w.fx && fxGranted;
    if (k.hist && !fx && !(k.l1x && l1x_on(sw))) return dict;
    if (k.mid) return L1Route::Mid;
    if (fx) return k.hist ? L1Route::Fxl : L1Route::Fx;
    if (k.hist) return L1Route::L1x;
    return k.rider ? L1Route::Duplex : L1Route::Parse;
}

// ---------------------------------------------------------------------------------------------------- HC levels 2..12 (launch_hc)
// PLZ4HIP_HB_MAX_BLOCKS / PLZ4HIP_HB_PIECE_KIB: chain and lists of few blocks built in pieces across the chip (hb_want below).
// 64 blocks: the largest measured count at which the pieces beat one wave per block by more than both spreads, kernels alone and
// through host buffers, at level 3 (profiles/hb_rate.json, 4 MiB T blocks: 38.8 against 71.3 ms kernels alone, 52.1 against 85.5
// through host buffers; at 128 the kernels alone still win, 72.7 against 89.3, but host buffers, 99.6 against 116.8, lie inside
// their spreads of 11.5 + 15.8; at 256 the pieces lose, 140.1 against 126.2) and do not lose at level 9 (53.9 against 86.4, 69.7
// against 100.4).  64 KiB pieces: the fastest at 1 block (profiles/hb_rate_pieces.json, level 3, kernels alone: 16 KiB 8.60, 32 KiB
// 6.90, 64 KiB 6.29, 128 KiB 6.41 ms) and within a fifth of the fastest at 64 blocks (38.9 against 128 KiB's 37.8).
constexpr int kHbMaxBlocks = 64;
constexpr int kHbPieceKiB = 64;
struct HcSwitches {
    int  hcx = kUnset;                     // PLZ4HIP_HCX (0: no block goes to k_hcx)
    bool extOff = false, midOff = false, lazyOff = false, preOff = false, listsOff = false;   // PLZ4HIP_HC_{EXT,MID,LAZY,PRE,LISTS}_OFF
    bool h12Off = false, h12Lazy = false, h12SegOff = false;                                  // PLZ4HIP_HC12_OFF, _LAZY, _SEG_OFF
    int  minSeg = 8192;                    // PLZ4HIP_HC_MIN_SEG >= 64 (tests: many segments in small blocks)
    int  segs = kLzMaxSegs;                // PLZ4HIP_HC_SEGS in 1..kLzMaxSegs
    int  gather = 12, idle = 16;           // PLZ4HIP_HC12_GATHER, PLZ4HIP_HC12_IDLE
    int  overlapMin = 2048;                // PLZ4HIP_HC_OVERLAP_MIN (tests: the pipeline on a handful of blocks)
    bool overlapOff = false;               // PLZ4HIP_HC_OVERLAP_OFF
    int  overlapGroups = 4;                // PLZ4HIP_HC_OVERLAP_GROUPS >= 2
    long budgetGiB = 0;                    // PLZ4HIP_HC_BUDGET_GIB
    int  h12Group = 0, group = 0;          // PLZ4HIP_HC12_GROUP, PLZ4HIP_HC_GROUP
    int  hbMax = kHbMaxBlocks;             // PLZ4HIP_HB_MAX_BLOCKS (0: off)
    int  hbPieceKiB = kHbPieceKiB;         // PLZ4HIP_HB_PIECE_KIB, clamped to 1..4096 (tests: many pieces in small blocks)
};

// (blocks of 8 MiB and more -- raw block API only -- keep the one-thread-per-block kernel: the writer packs positions into 23 bits)
inline bool use_h12(const HcSwitches& sw, int level, bool hcEx, int maxLen) { return level >= 12 && !hcEx && maxLen < (1 << 23) && !sw.h12Off; }
// levels 3..11, independent blocks up to 4 MiB: segments walked at once, stitched, record emit (lz4hc_lazy_device.inl)
// (PLZ4HIP_HC12_LAZY, an experiment switch: level 12 on the same walk)
inline bool use_lazy(const HcSwitches& sw, int level, bool hcEx, int maxLen)
{
    return level >= 3 && (level <= 11 || sw.h12Lazy) && !hcEx && maxLen > 0 && maxLen <= kSeqMaxBlock && !sw.lazyOff;
}

// HcxOnly: a call of nothing but blocks <= 4 KiB under a dictionary context, one k_hcx launch.  MidStaged: level 2 on the staged
// level-1 call.  Segmented: the walk in segments (lazy: levels 3..11; lazyEx: behind external segments, levels 3..12; seg12: level
// 12's optimal parser; none of them: level 12's three phases, one wave per block).  OneThread: the one-thread parsers, `pre`: with
// chain (and lists) built up front.
enum class HcRoute { HcxOnly, MidStaged, Segmented, OneThread };
struct HcShape { int level, nb, maxLen; bool raw, hcEx, dict, dictCtx, linked, hcxStart; };   // dict: a.dict; dictCtx: a.dictLen >= 0
struct HcPlan {
    HcRoute route;
    bool hcx;                              // the blocks <= 4 KiB under a dictionary context are k_hcx's (a.hcx)
    bool lazy, lazyEx, seg12, segs, pre;
    bool prepExt;                          // k_hc_ext_prep in front
    bool ctxBlocks;                        // behind the emit stage: the context's small blocks (k_hcx, or the one-thread parser)
    bool hcxBehind;                        // OneThread: k_hcx behind the one-thread kernels, which passed its blocks over
    int  lzMinSeg, lzSegs, gather, idle;   // Segmented: a.lzMinSeg, a.lzSegs, a.h12Gather, a.h12Idle
};
// midDeclined: the staged level-1 call found no workspace (k_hc_ext_prep has run): every block on the one-thread parser
inline HcPlan hc_route(const HcShape& k, const HcSwitches& sw, bool midDeclined = false)
{
    HcPlan p{};
    const bool anyDict = k.dict || k.dictCtx;
    const bool fits = k.maxLen > 0 && k.maxLen <= kSeqMaxBlock;
    p.hcx = k.hcEx && anyDict && k.hcxStart && k.level >= kHcxMinLevel && k.level <= kHcxMaxLevel && sw.hcx != 0;
    if (p.hcx && k.maxLen <= kHcxMaxBlock && (k.raw || !k.linked)) { p.route = HcRoute::HcxOnly; return p; }
    const bool extOk = k.hcEx && fits && !sw.extOff;
    if (k.level == 2 && (!k.hcEx || extOk) && fits && !sw.midOff && !midDeclined) {
        p.route = HcRoute::MidStaged; p.prepExt = k.hcEx; p.ctxBlocks = k.hcEx && anyDict;
        return p;
    }
    p.lazyEx = extOk && k.level >= 3;
    p.lazy = use_lazy(sw, k.level, k.hcEx, k.maxLen) || p.lazyEx;
    if (p.lazy || use_h12(sw, k.level, k.hcEx, k.maxLen)) {
        p.route = HcRoute::Segmented;
        p.seg12 = !p.lazy && fits && !sw.h12SegOff;
        p.segs = p.lazy || p.seg12;
        p.prepExt = p.lazyEx; p.ctxBlocks = p.lazyEx && anyDict;
        p.lzMinSeg = p.segs ? sw.minSeg : 0; p.lzSegs = p.segs ? sw.segs : 0;
        p.gather = sw.gather; p.idle = sw.idle;
        return p;
    }
    p.route = HcRoute::OneThread;
    p.pre = k.level >= 3 && !k.hcEx && k.maxLen >= 4096 && !sw.preOff;
    p.hcxBehind = p.hcx;
    return p;
}

// ---------------------------------------------------------------------------------------------------- level 2, few blocks (launch_l1)
// HcRoute::MidStaged on independent blocks: the walk cut into pieces across the chip (lz4_mx_device.inl) instead of k_hc_mid's one
// wave per block.  The pieces walk about three times the block's bytes, which is free only while the chip has idle waves.
// PLZ4HIP_MX_MAX_BLOCKS: 512, the largest measured count at which the pieces beat one wave per block by more than both spreads, kernels
// alone and through host buffers (profiles/mx_rate.json, 4 MiB T blocks: 663 against 984 ms; at 1024 the kernels alone tie, 1 222 ms,
// at 2048 they lose, 2 357 against 1 556).  The workspace of such a call is 5 bytes per input byte (10 GiB at 512 x 4 MiB).
constexpr int kMxMaxBlocks = 512;
// PLZ4HIP_MXL_MAX_BLOCKS: the same bar for blocks with history outside the block (a dictionary, linked blocks: mxl_want), measured
// on its own: 512 (profiles/mxl_rate.json, 4 MiB linked T blocks behind a 64 KiB dictionary: 681 against 1 023 ms kernels alone, 762
// against 1 136 through host buffers; at 1024 the kernels alone lose, 1 250 against 1 213, while host buffers still win).
constexpr int kMxlMaxBlocks = 512;
struct MxSwitches {
    int maxBlocks = kMxMaxBlocks;          // PLZ4HIP_MX_MAX_BLOCKS (0: off)
    int pieceKiB = 128, warmKiB = 256;     // PLZ4HIP_MX_PIECE_KIB in 1..4096, PLZ4HIP_MX_WARMUP_KIB in 0..4096 (rounds per choice)
    int mxlMaxBlocks = kMxlMaxBlocks;      // PLZ4HIP_MXL_MAX_BLOCKS (0: off): the same walk behind external segments (mxl_want)
};
struct MxShape { int level, nb, maxLen; bool hcEx, rider; };
// What the call asks for before anything is reserved: mx -- the walk in pieces, with its cut (piece_cut).
struct MxWant { bool mx; int piece, warm, P; PieceCut cut() const { return PieceCut{mx, piece, warm, P}; } };
inline MxWant mx_want(const MxShape& k, const MxSwitches& sw)
{
    // (a call whose largest block is one piece has nothing to cut: one wave per block either way, so it keeps today's launch)
    const bool mx = k.level == 2 && !k.hcEx && !k.rider && k.nb >= 1 && k.nb <= sw.maxBlocks && k.maxLen > (sw.pieceKiB << 10) && k.maxLen <= kSeqMaxBlock;
    const PieceCut c = piece_cut(mx, k.maxLen, sw.pieceKiB, sw.warmKiB);
    return MxWant{c.on, c.piece, c.warm, c.P};
}
// The same question for a level-2 call whose blocks have history outside the block (hcEx: a dictionary, linked blocks; k_hc_mid<true>
// otherwise): no rider, 1 .. mxlMaxBlocks blocks, the largest above one piece and at most 4 MiB.  Piece and warm-up are mx_want's.
inline MxWant mxl_want(const MxShape& k, const MxSwitches& sw)
{
    const bool mx = k.level == 2 && k.hcEx && !k.rider && k.nb >= 1 && k.nb <= sw.mxlMaxBlocks && k.maxLen > (sw.pieceKiB << 10) && k.maxLen <= kSeqMaxBlock;
    const PieceCut c = piece_cut(mx, k.maxLen, sw.pieceKiB, sw.warmKiB);
    return MxWant{c.on, c.piece, c.warm, c.P};
}
// ... and given what was granted: the staged call's group workspace and the pieces' own.  false: today's k_hc_mid launch.
inline bool mx_route(const MxWant& w, bool stagedGranted, bool mxGranted) { return w.mx && stagedGranted && mxGranted; }

// The groups of the segmented route over a workspace of `group` blocks (HcLayout::group).  Without overlap: groups of equal size.
// With it (the list builder of group g+1 beside the walk of group g, over the two halves of the workspace) only the first group's
// builder is exposed, so the groups start at an eighth and double (a builder takes about half the time of the walk over the same
// blocks) until they have the full size.
struct HcGroups { bool overlap; int per, nGroups; std::vector<int> gStart, gSize; };
inline HcGroups hc_groups(int nb, int group, bool lazy, const HcSwitches& sw)
{
    HcGroups g{};
    g.nGroups = (nb + group - 1) / group;
    g.per = (nb + g.nGroups - 1) / g.nGroups;
    g.overlap = lazy && nb >= sw.overlapMin && nb >= 2 && group >= 2 && !sw.overlapOff;      // (two groups' worth of workspace)
    if (g.overlap) {
        const int want = sw.overlapGroups;
        int tgt = group / 2 < (nb + want - 1) / want ? group / 2 : (nb + want - 1) / want;
        if (tgt < 1) tgt = 1;
        g.nGroups = (nb + tgt - 1) / tgt;
        g.per = (nb + g.nGroups - 1) / g.nGroups;
    }
    for (int at = 0, sz = g.overlap ? (g.per / 8 > 0 ? g.per / 8 : 1) : g.per; at < nb; ) {
        const int n = nb - at < sz ? nb - at : sz;
        g.gStart.push_back(at); g.gSize.push_back(n);
        at += n;
        sz = sz * 2 < g.per ? sz * 2 : g.per;
    }
    g.nGroups = (int)g.gStart.size();
    return g;
}

// ---------------------------------------------------------------------------------------------------- levels 3..12, few blocks (hc_segmented)
// HcRoute::Segmented: chain, rank and list built in pieces of the positions by many workgroups per block (lz4hc_lists_device.inl:
// count, scan, fill, chain) instead of k_hc12_hist + k_hc12_chain's one wave per block.  The arrays are the same; everything behind
// the builder is untouched.  The pieces cost two 128 KiB tables each in device memory and a table set-up per piece, which pays only
// while the chip has idle CUs: at most hbMax blocks, the default following kMxMaxBlocks' rule (the largest measured count at which
// the pieces beat one wave per block by more than both spreads, kernels alone and through host buffers).
// maxLen: the largest block; span: the largest segment + block (the positions the lists are built over); overlap: HcGroups::overlap,
// the builder beside the walk, which lives on the builder being one wave per CU.
struct HbShape { int level, nb, maxLen, span; bool segmented, overlap; };
struct HbWant { bool on; int piece, P; };                                   // pieces of `piece` positions, P per block of `span`
inline HbWant hb_want(const HbShape& k, const HcSwitches& sw)
{
    HbWant w{};
    const int piece = sw.hbPieceKiB << 10;
    // (a call whose largest block is one piece has nothing to cut; raw blocks above 4 MiB keep today's builder)
    w.on = k.segmented && k.level >= 3 && k.level <= 12 && !k.overlap && k.nb >= 1 && k.nb <= sw.hbMax
        && k.maxLen > 0 && k.maxLen <= kSeqMaxBlock && k.span > piece;
    if (w.on) { w.piece = piece; w.P = (k.span + piece - 1) / piece; }
    return w;
}
// ... and given what was granted: the pieces' own workspace.  false: today's k_hc12_hist + k_hc12_chain.
inline bool hb_route(const HbWant& w, bool granted) { return w.on && granted; }

// ---------------------------------------------------------------------------------------------------- decode (launch_decode)
constexpr int    kDxlGroupBlocks = 128;                                     // the fastest of 16 / 32 / 64 / 128 on a 256-block chain
constexpr double kDxlMsPerBlock = 0.33, kWalkMsPerBlock = 59.0;             // t_dx, t_wave: 4 MiB blocks; both scale with the block alike
constexpr int    kDxlGroupChains = 1024;                                    // chains a group's pointer space has room for
struct DxSwitches {
    int  dxMax = 128;                      // PLZ4HIP_DX_MAX_BLOCKS (0: off)
    int  linked = kUnset;                  // PLZ4HIP_DX_LINKED (0: history outside the block keeps the one-wave kernels)
    int  groupBlocks = kUnset;             // PLZ4HIP_DXL_GROUP_BLOCKS (set: forced, also for calls that fit one pass; 0: no groups)
    int  big = kUnset;                     // PLZ4HIP_DX_BIG (0: off)
    long long bigMaxMiB = 1024;            // PLZ4HIP_DX_BIG_MAX_MIB
    int  bigGroup = 0, bigRunKiB = 0;      // PLZ4HIP_DX_BIG_GROUP in 2..kDxbMaxGroup, PLZ4HIP_DX_BIG_RUN_KIB in 1..2^20 (0: the default)
};
enum { kHistNone = 0, kHistDict = 1, kHistLinked = 2 };
// OneWave: the tail kernel alone.  Dx: the few-block stage train (hist: the dxl flavour).  DxGrouped: ... per group of G consecutive
// blocks of a linked call.  DxBig: raw blocks above kDxMaxOut, the dxb stages.  Behind all of them the tail kernel sweeps up.
enum class DxRoute { OneWave, Dx, DxGrouped, DxBig };
enum class DxTail { Raw, Rec, RecDx, RawDict, RecDict, RecLinked, None };    // None: a linked call the stage train has finished
// longest: the longest chain's blocks (linked).  hostFirst: the chains' first blocks are known to the host (or there is one chain).
struct DxShape { int nb; int64_t maxIn, maxOut; bool records; int hist; bool window; int nChains, longest; bool hostFirst; };
// Before anything is reserved.  G > 0: cut the call into groups of G blocks (dxl_group) -- taken iff every group holds at most
// kDxlGroupChains chains and there are two or more.  big: the dxb stages with bigG, thr, rounds (instead of dx, not beside it).
struct DxWant { bool dx; int G; bool big; int bigG, thr, rounds; };
inline DxWant dx_want(const DxShape& k, const DxSwitches& sw)
{
    DxWant w{};
    const bool dxShape = k.maxIn >= 16384 && k.maxIn <= (int64_t)(6 << 20) && k.maxOut >= 1;
    w.dx = k.nb <= sw.dxMax && dxShape;
    bool dxl = true;
    if (k.hist) {
        if (sw.linked == 0) dxl = false;
        if (k.hist == kHistLinked && (!k.records || !k.window || k.nChains < 1)) dxl = false;
        if (!dxl) w.dx = false;
    }
    if (k.hist == kHistLinked && dxl && dxShape && sw.dxMax > 0 && k.hostFirst) {
        int G = sw.groupBlocks == kUnset ? kDxlGroupBlocks : sw.groupBlocks;
        const bool forced = sw.groupBlocks != kUnset;
        // the pointer space: blocks x stride + chains x 64 Ki stays below 2^31 (bit 31 tags a distance)
        const int64_t room = ((int64_t)1 << 31) - (int64_t)kDxlGroupChains * kDxlHist - 1, pStride = (int64_t)dx_ptr_stride(k.maxOut);
        if (G > 0 && (int64_t)G * pStride > room) G = (int)(room / pStride);
        // many short chains are better served by one wave per chain
        if (G > 0 && (forced ? k.nb > G : !w.dx) && (double)k.nb * kDxlMsPerBlock <= (double)k.longest * kWalkMsPerBlock && k.nb > G) w.G = G;
    }
    if (!k.hist && !k.records && k.nb <= sw.dxMax && k.maxOut > (int64_t)kDxMaxOut && k.maxIn >= 16384) {
        const int64_t bigMax = sw.bigMaxMiB > 1024 ? 1024 : sw.bigMaxMiB;  // (positions are 31-bit)
        const int64_t capMax = (bigMax << 20) + 8;
        if (sw.big != 0 && k.maxOut <= capMax && k.maxIn <= capMax + capMax / 255 + 64) {
            w.big = true; w.dx = false;
            w.bigG = sw.bigGroup ? sw.bigGroup : dxb_group_for(dx_max_seg(k.maxIn));
            w.thr = sw.bigRunKiB ? sw.bigRunKiB << 10 : (int)kDxbThr;
            w.rounds = dxb_rounds(k.maxOut);
        }
    }
    return w;
}
// The route once the groups are cut (groupsOk) and the workspace was asked for (granted).  A cut call is dx's whatever w.dx said.
struct DxPlan { DxRoute route; DxTail tail; };
inline DxPlan dx_route(const DxShape& k, const DxWant& w, bool groupsOk, bool granted)
{
    DxPlan p{};
    const bool grouped = w.G > 0 && groupsOk;
    const bool dx = (w.dx || grouped) && granted;
    p.route = w.big && granted ? DxRoute::DxBig : !dx ? DxRoute::OneWave : grouped ? DxRoute::DxGrouped : DxRoute::Dx;
    p.tail = k.hist == kHistLinked ? (dx ? DxTail::None : DxTail::RecLinked)
           : k.hist ? (k.records ? DxTail::RecDict : DxTail::RawDict)
           : k.records ? (dx ? DxTail::RecDx : DxTail::Rec) : DxTail::Raw;
    return p;
}

// ---------------------------------------------------------------------------------------------------- the switches out of an environment
// get(name): the variable's text or null (read_*_switches: getenv; tests/emu/emu_routes.cpp: a table).  Every value is parsed and
// clamped here, so that the route functions and the launchers see what holds.
template <class Get> L1Switches parse_l1_switches(Get&& get)
{
    const auto num = [&](const char* n, long unset) { const char* v = get(n); return v ? atol(v) : unset; };
    L1Switches sw;
    sw.fused = get("PLZ4HIP_L1_FUSED") != nullptr;
    sw.fxLinked = (int)num("PLZ4HIP_FX_LINKED", kUnset);
    if (const char* v = get("PLZ4HIP_FX_MAX_BLOCKS")) sw.fxMax = atoi(v);
    parse_piece_kib(get, "PLZ4HIP_FX_PIECE_KIB", "PLZ4HIP_FX_WARMUP_KIB", &sw.fxPieceKiB, &sw.fxWarmKiB);
    sw.l1x = (int)num("PLZ4HIP_L1X", kUnset);
    sw.oneWorkspace = num("PLZ4HIP_L1_WORKSPACES", 0) == 1;
    sw.budgetGiB = num("PLZ4HIP_L1_BUDGET_GIB", 0);
    sw.budgetMiB = num("PLZ4HIP_L1_BUDGET_MIB", 0);
    sw.noGate = get("PLZ4HIP_EXP_NO_GATE") != nullptr;
    if (const char* v = get("PLZ4HIP_DUPLEX")) { if (sscanf(v, "%d,%d", &sw.duplexP, &sw.duplexD) != 2) { sw.duplexP = 1; sw.duplexD = 1; } }
    sw.duplexPrio = (int)num("PLZ4HIP_DUPLEX_PRIO", 3);
    return sw;
}
template <class Get> HcSwitches parse_hc_switches(Get&& get)
{
    const auto num = [&](const char* n, long unset) { const char* v = get(n); return v ? atol(v) : unset; };
    const auto set = [&](const char* n) { return get(n) != nullptr; };
    HcSwitches sw;
    sw.hcx = (int)num("PLZ4HIP_HCX", kUnset);
    sw.extOff = set("PLZ4HIP_HC_EXT_OFF"); sw.midOff = set("PLZ4HIP_HC_MID_OFF"); sw.lazyOff = set("PLZ4HIP_HC_LAZY_OFF");
    sw.preOff = set("PLZ4HIP_HC_PRE_OFF"); sw.listsOff = set("PLZ4HIP_HC_LISTS_OFF");
    sw.h12Off = set("PLZ4HIP_HC12_OFF"); sw.h12Lazy = set("PLZ4HIP_HC12_LAZY"); sw.h12SegOff = set("PLZ4HIP_HC12_SEG_OFF");
    { const int m = (int)num("PLZ4HIP_HC_MIN_SEG", 0); if (m >= 64) sw.minSeg = m; }
    { const int n = (int)num("PLZ4HIP_HC_SEGS", kLzMaxSegs); sw.segs = n < 1 ? 1 : (n > kLzMaxSegs ? kLzMaxSegs : n); }
    sw.gather = (int)num("PLZ4HIP_HC12_GATHER", 12); sw.idle = (int)num("PLZ4HIP_HC12_IDLE", 16);
    sw.overlapMin = (int)num("PLZ4HIP_HC_OVERLAP_MIN", 2048);
    sw.overlapOff = set("PLZ4HIP_HC_OVERLAP_OFF");
    { const int w = (int)num("PLZ4HIP_HC_OVERLAP_GROUPS", 4); sw.overlapGroups = w < 2 ? 2 : w; }
    sw.budgetGiB = num("PLZ4HIP_HC_BUDGET_GIB", 0);
    sw.h12Group = (int)num("PLZ4HIP_HC12_GROUP", 0); sw.group = (int)num("PLZ4HIP_HC_GROUP", 0);
    { const long m = num("PLZ4HIP_HB_MAX_BLOCKS", kHbMaxBlocks); sw.hbMax = m < 0 ? 0 : (m > 65535 ? 65535 : (int)m); }   // (the blocks are the grid's y)
    { const long p = num("PLZ4HIP_HB_PIECE_KIB", kHbPieceKiB); sw.hbPieceKiB = p < 1 ? 1 : (p > 4096 ? 4096 : (int)p); }
    return sw;
}
template <class Get> MxSwitches parse_mx_switches(Get&& get)
{
    const auto num = [&](const char* n, int unset) { const char* v = get(n); return v ? atoi(v) : unset; };
    MxSwitches sw;
    sw.maxBlocks = num("PLZ4HIP_MX_MAX_BLOCKS", kMxMaxBlocks);
    if (sw.maxBlocks > 65535) sw.maxBlocks = 65535;                            // (the blocks of a group are the grid's y)
    sw.mxlMaxBlocks = num("PLZ4HIP_MXL_MAX_BLOCKS", kMxlMaxBlocks);
    if (sw.mxlMaxBlocks > 65535) sw.mxlMaxBlocks = 65535;
    parse_piece_kib(get, "PLZ4HIP_MX_PIECE_KIB", "PLZ4HIP_MX_WARMUP_KIB", &sw.pieceKiB, &sw.warmKiB);
    return sw;
}
template <class Get> DxSwitches parse_dx_switches(Get&& get)
{
    const auto num = [&](const char* n, int unset) { const char* v = get(n); return v ? atoi(v) : unset; };
    DxSwitches sw;
    sw.dxMax = num("PLZ4HIP_DX_MAX_BLOCKS", 128);
    sw.linked = num("PLZ4HIP_DX_LINKED", kUnset);
    sw.groupBlocks = num("PLZ4HIP_DXL_GROUP_BLOCKS", kUnset);
    sw.big = num("PLZ4HIP_DX_BIG", kUnset);
    if (const char* v = get("PLZ4HIP_DX_BIG_MAX_MIB")) sw.bigMaxMiB = atoll(v);
    { const int g = num("PLZ4HIP_DX_BIG_GROUP", 0); if (g >= 2 && g <= kDxbMaxGroup) sw.bigGroup = g; }
    { const int k = num("PLZ4HIP_DX_BIG_RUN_KIB", 0); if (k >= 1 && k <= (1 << 20)) sw.bigRunKiB = k; }
    return sw;
}

}  // namespace plz4
