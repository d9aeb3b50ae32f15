// The stage train of the few-block decoders over ONE call of nb blocks (lz4_dx_device.inl: the table at its head), launch by launch
// as plz4hip.hip enqueues them, on the lane-emulated device code, for the three flavours (DxF, DxbF, DxlF).  Shared by the
// emulations the tests load (emu_kernels.cpp, emu_dx_big.cpp, emu_dxl.cpp, emu_dxl_groups.cpp, emu_dx_train.cpp) and the sanitizer
// programs (decode_bounds_main.cpp, dx_big_bounds_main.cpp).  The workspace is what launch_decode reserves: dx_layout / dxb_layout
// (ws_layout.h) with launch_decode's arguments, every array a heap allocation of exactly its take, uninitialised as the device's
// is, so a sanitizer sees every access outside one.  Every stage is the body the kernel runs (dx_stage_*, dxb_stage_*), over the
// kernel's whole grid -- every unit and every chunk of every block, flagged or not -- segments, chunks and blocks from the top down:
// the order in which no wave finds a neighbour's work done.  Test infrastructure only.
#pragma once
#include "../../plz4_amd/csrc/lz4_device.inl"
#include "../../plz4_amd/csrc/lz4_seq_device.inl"
#include "../../plz4_amd/csrc/lz4hc_device.inl"
#include "../../plz4_amd/csrc/lz4hc12_device.inl"
#include "../../plz4_amd/csrc/lz4hc_lazy_device.inl"
#include "../../plz4_amd/csrc/lz4hcx_device.inl"
#include "../../plz4_amd/csrc/lz4_dx_device.inl"
#include "../../plz4_amd/csrc/lz4_fx_device.inl"
#include "../../plz4_amd/csrc/lz4_mx_device.inl"
#include "../../plz4_amd/csrc/ws_layout.h"
#include <stdlib.h>
#include <string.h>
#include <vector>

namespace plz4 {

// what the C entries answer for a block: left to the one-wave decoder; units that do not meet (a bug); a run list beyond its room
enum : int { kDxEmuLeft = -999999, kDxEmuUnitsDisagree = -888888, kDxEmuListOverrun = -777777 };

// The call as dx_src / dx_len / cap_of give it to the kernels: block b is len[b] bytes at src[b] (exactly that many readable; < 0:
// not a compressed block) and has cap[b] bytes at dst + b * dstStride.
struct DxEmuCall { int nb; const uint8_t* const* src; const int32_t* len; const int32_t* cap; uint8_t* dst; int64_t dstStride; };

// One heap allocation per take of a layout, found again by the take's offset
struct DxEmuWs {
    std::vector<WsTake> log; std::vector<void*> mem;
    DxEmuWs() {}
    DxEmuWs(const DxEmuWs&) = delete;
    ~DxEmuWs() { for (void* p : mem) free(p); }
    void alloc()
    {
        for (const WsTake& t : log) {
            const size_t bytes = t.count * t.size;
            void* p = malloc(bytes ? bytes : 1); if (!p) abort();
            memset(p, 0xEE, bytes);
            mem.push_back(p);
        }
    }
    template <class T> T* at(size_t off) const
    {
        for (size_t i = 0; i < log.size(); ++i) if (log[i].off == off && log[i].count && log[i].size == sizeof(T)) return (T*)mem[i];
        abort();
    }
};

struct DxEmuTrain {
    DxEmuCall c{}; DxEmuWs ws;
    int64_t tStride = 0, pStride = 0; int maxSeg = 0, chunks = 0;
    uint64_t* T = nullptr; uint32_t* ptr = nullptr; DxUnit* units = nullptr; DxInfo* info = nullptr;
    uint32_t* moved = nullptr;                                              // DxlF: the call's rows of moved[]
    DxbInfo* bi = nullptr; DxbLayout big{};                                 // DxbF
    int launched = 0;                                                       // jump rounds
    bool disagree = false;                                                  // a unit did not stop where the next one starts

    // L: the DxLayout / DxbLayout that filled ws.log; outB: the output bytes the per-byte grids cover
    template <class Layout> void bind(const DxEmuCall& call, const Layout& L, int64_t outB)
    {
        c = call; ws.alloc();
        tStride = (int64_t)L.tStride; pStride = (int64_t)L.pStride; maxSeg = L.maxSeg; chunks = (int)((outB + 1023) / 1024);
        T = ws.at<uint64_t>(L.offT); ptr = ws.at<uint32_t>(L.offPtr); units = ws.at<DxUnit>(L.offUnits); info = ws.at<DxInfo>(L.offInfo);
    }
    DxBlk blk(int b) const                                                  // dx_blk of plz4hip.hip
    {
        DxBlk k;
        k.src = c.src[b]; k.n = c.len[b]; k.dst = c.dst + (int64_t)b * c.dstStride; k.cap = c.cap[b];
        k.T = T + (int64_t)b * tStride; k.ptr = ptr + (int64_t)b * pStride; k.units = units + (int64_t)b * maxSeg;
        k.tStride = tStride; k.pStride = pStride; k.maxSeg = maxSeg; k.info = info + b; k.b = b;
        return k;
    }
    void tables() { for (int b = c.nb - 1; b >= 0; --b) for (int j = maxSeg - 1; j >= 0; --j) dx_stage_tables(blk(b), j, (uint32_t)maxSeg); }
    void stitch() { for (int b = c.nb - 1; b >= 0; --b) dx_stage_stitch(blk(b)); }
    // f(b): the flavour for block b, as K::flavour(a, b) makes it
    template <class Of> void fill(Of&& f)
    {
        for (int b = c.nb - 1; b >= 0; --b) for (int j = maxSeg - 1; j >= 0; --j) disagree |= dx_stage_fill(f(b), blk(b), j) == kDxFillDisagree;
    }
    template <class Of> void jump(Of&& f, int rounds)
    {
        launched = rounds;
        for (int r = 0; r < rounds; ++r) for (int b = c.nb - 1; b >= 0; --b)
            for (int64_t p0 = (int64_t)chunks * 1024 - 256; p0 >= 0; p0 -= 256) dx_stage_jump(f(b), blk(b), r, (int)p0);
    }
    template <class Of> void gather(Of&& f)
    {
        for (int b = 0; b < c.nb; ++b) for (int64_t p0 = 0; p0 < (int64_t)chunks * 1024; p0 += 256) dx_stage_gather(f(b), blk(b), (int)p0);
    }
    // what the verdict behind the gather reads: the block's size, or kDxEmuLeft
    int answer(int b) const { return info[b].bad ? (int)kDxEmuLeft : info[b].outLen; }
    // the rounds of a block's row of moved[] in which something moved
    static int moving(const uint32_t* row, int rounds) { int r = 0; while (r < rounds && row[r]) ++r; return r; }
};

// launch_dx_train without history (Dx): maxIn / maxOut as launch_decode has them; rounds > 0: that many instead of the rule's
inline void dx_emu_train(DxF, DxEmuTrain& t, const DxEmuCall& c, int64_t maxIn, int64_t maxOut, int rounds = 0)
{
    const DxLayout L = dx_layout(c.nb, c.nb, maxIn, maxOut, false, false, 0, &t.ws.log);
    t.bind(c, L, maxOut < kDxMaxOut ? maxOut : (int64_t)kDxMaxOut);
    const auto f = [](int) { return DxF{}; };
    t.tables(); t.stitch(); t.fill(f);
    t.jump(f, rounds > 0 ? rounds : DxF::rounds(c.nb, maxOut));
    t.gather(f);
}

// launch_dxb (DxBig): G segments to a group, runs of thr bytes or more listed, as dx_want gives them
inline void dx_emu_train(DxbF, DxEmuTrain& t, const DxEmuCall& c, int64_t maxIn, int64_t maxOut, int G, int thr, int rounds = 0)
{
    const DxbLayout L = t.big = dxb_layout(c.nb, maxIn, maxOut, G, thr, &t.ws.log);
    t.bind(c, L, maxOut);
    uint64_t* const TG = t.ws.at<uint64_t>(L.offTG); DxbEntry* const ent = t.ws.at<DxbEntry>(L.offEnt);
    DxRun* const list = t.ws.at<DxRun>(L.offRuns); DxbInfo* const bi = t.bi = t.ws.at<DxbInfo>(L.offBi);
    const auto f = [&](int b) { return DxbF{TG + (int64_t)b * L.tgStride, ent + (int64_t)b * L.groups, G, list + (int64_t)b * L.room, L.room, thr, bi + b}; };
    t.tables();
    for (int b = c.nb - 1; b >= 0; --b) for (int w = L.groups * 128 - 1; w >= 0; --w) dxb_stage_compose(f(b), t.blk(b), w >> 7, w & 127);
    for (int b = c.nb - 1; b >= 0; --b) dxb_stage_hop(f(b), t.blk(b));
    for (int b = c.nb - 1; b >= 0; --b) for (int g = L.groups - 1; g >= 0; --g) dxb_stage_units(f(b), t.blk(b), g);
    t.fill(f);
    for (int b = 0; b < c.nb; ++b) {                                        // k_dxb_runs
        if (t.info[b].bad) continue;
        const DxBlk k = t.blk(b); const DxRun* const l = f(b).list;
        const uint32_t nr = min_(bi[b].runs, (uint32_t)L.room);
        for (uint32_t i = 0; i < nr; ++i) for (uint32_t p = dxb_run_pieces(l[i]); p-- > 0;) dxb_run_piece(l[i], p, k.src, k.dst, k.ptr);
    }
    t.jump(f, rounds > 0 ? rounds : DxbF::rounds(c.nb, maxOut));
    t.gather(f);
}

// launch_dx_train with history (Dx or one group of DxGrouped): wb: the blocks the layout is sized for, nChGrouped: the chains of a
// grouped call.  call: the history and the blocks' first / chain arrays, the rest is filled in here.  link(): what k_dxl_link flags
// (a chain known to have ended), between the stitch and the fill.  Leaves the blocks' rows of moved[] in t.moved.
template <class Link>
inline void dx_emu_train(DxlF, DxEmuTrain& t, const DxEmuCall& c, DxlCall& call, int wb, int64_t maxIn, int64_t maxOut, bool records, int nChGrouped,
                         Link&& link, int rounds = 0)
{
    const DxLayout L = dx_layout(wb, c.nb, maxIn, maxOut, true, records, nChGrouped, &t.ws.log);
    t.bind(c, L, maxOut < kDxMaxOut ? maxOut : (int64_t)kDxMaxOut);
    t.moved = t.ws.at<uint32_t>(L.offMoved);
    call.ptr = t.ptr; call.P = t.pStride; call.nb = c.nb; call.info = t.info; call.len = c.len; call.dst = c.dst; call.dstStride = c.dstStride;
    const auto f = [&](int) { return DxlF{call, t.moved}; };
    t.tables(); t.stitch();
    link();                                                                 // k_dxl_link
    for (int64_t i = 0; i < (int64_t)c.nb * (kDxlMaxRounds + 1); ++i) t.moved[i] = 0;
    t.fill(f);
    for (int b = c.nb - 1; b >= 0; --b)                                     // k_dxl_resolve: every entry of every block, flagged ones included
        for (int64_t p0 = t.pStride - 256; p0 >= 0; p0 -= 256) if (!dxl_resolve(call, b, (int)p0, (int)t.pStride)) dx_flag(&t.info[b].bad);
    t.jump(f, rounds > 0 ? rounds : DxlF::rounds(c.nb, maxOut));
    t.gather(f);
}

// A call of raw blocks through the train of flavour fl -- 0: DxF; 1: DxbF at the call's default group size and run threshold; 2: DxlF,
// independent blocks under the dictionary dict (chains of one) -- with the workspace laid out for maxIn / maxOut, whatever the
// blocks' own sizes are.  answer[b]: the block's size, or kDxEmuLeft.  Returns 0, or kDxEmuUnitsDisagree.
inline int dx_emu_raw_call(const int fl, const DxEmuCall& c, const int64_t maxIn, const int64_t maxOut, const uint8_t* dict, const int dictLen,
                           const int rounds, int32_t* answer)
{
    DxEmuTrain t;
    if (fl == 0) dx_emu_train(DxF{}, t, c, maxIn, maxOut, rounds);
    else if (fl == 1) dx_emu_train(DxbF{}, t, c, maxIn, maxOut, dxb_group_for(dx_max_seg(maxIn)), kDxbThr, rounds);
    else {
        DxlCall call{};
        call.hist = dict; call.histLenAll = dictLen;
        dx_emu_train(DxlF{}, t, c, call, c.nb, maxIn, maxOut, false, 0, [] {}, rounds);
    }
    for (int b = 0; b < c.nb; ++b) {
        answer[b] = t.answer(b);
        if (fl == 2 && !dxl_converged(t.moved + (int64_t)b * (kDxlMaxRounds + 1), t.launched)) answer[b] = kDxEmuLeft;   // (k_dxl_verdict)
    }
    return t.disagree ? (int)kDxEmuUnitsDisagree : 0;
}

// exactly n elements, none behind them
template <class T> struct DxEmuHeap {
    T* p; size_t n;
    explicit DxEmuHeap(size_t n_) : n(n_) { p = (T*)malloc((n ? n : 1) * sizeof(T)); if (!p) abort(); }
    DxEmuHeap(const DxEmuHeap&) = delete;
    ~DxEmuHeap() { free(p); }
};

// ONE raw block of a big-path call whose strides are maxIn / maxOut (emu_dx_big.cpp, dx_big_bounds_main.cpp).  src: exactly n readable
// bytes; dst: exactly cap writable bytes.  G, thr: 0: the call's defaults.  Returns the block's size or one of kDxEmu*.
// groups: the ones the hop walks (those in front of the tail unit); taken: the round that saw nothing move included.
struct DxbEmuStats { int launched, taken, runs, groups, room; };
inline int dxb_emu_block(const uint8_t* src, const int n, uint8_t* dst, const int cap, const int64_t maxIn, const int64_t maxOut, int G, int thr,
                         DxbEmuStats* st)
{
    if (G <= 0) G = dxb_group_for(dx_max_seg(maxIn));
    if (thr <= 0) thr = kDxbThr;
    DxEmuTrain t;
    const int32_t len = n, room = cap;
    dx_emu_train(DxbF{}, t, DxEmuCall{1, &src, &len, &room, dst, 0}, maxIn, maxOut, G, thr);
    st->launched = t.launched; st->taken = 0; st->runs = 0; st->groups = (dx_tail_from(dx_segments(n)) + G - 1) / G; st->room = t.big.room;
    if (t.disagree) return kDxEmuUnitsDisagree;
    if (t.info[0].bad) return kDxEmuLeft;
    if (t.bi[0].runs > (uint32_t)t.big.room) return kDxEmuListOverrun;         // (a full list flags the block in the fill)
    st->runs = (int)t.bi[0].runs; st->taken = dxl_rounds_of(t.bi[0].moved, t.launched);
    return t.info[0].outLen;
}

}  // namespace plz4
