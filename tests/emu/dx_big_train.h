// The stage train of launch_decode for ONE raw block of a call on the big path (blocks above kDxMaxOut; dxb_* in
// plz4_amd/csrc/lz4_dx_device.inl), kernel by kernel as plz4hip.hip enqueues them, on the lane-emulated device code.  Shared by the
// emulation the tests load (emu_dx_big.cpp) and the sanitizer program (dx_big_bounds_main.cpp): every workspace is a heap allocation
// of exactly what launch_decode reserves for a block of a call whose strides are maxIn / maxOut, so a sanitizer sees every access
// outside one.  Test infrastructure only.
#pragma once
#include "../../plz4_amd/csrc/lz4_dx_device.inl"
#include <stdlib.h>
#include <string.h>

namespace dxbig {
using namespace plz4;

enum : int { kLeft = -999999, kUnitsDisagree = -888888, kListOverrun = -777777 };

struct Stats { int launched, taken, runs, groups, room; };     // groups: the ones the hop walks (those in front of the tail unit)

template <class T> struct Heap {
    T* p; size_t n;
    explicit Heap(size_t n_) : n(n_) { p = (T*)malloc((n ? n : 1) * sizeof(T)); if (!p) abort(); }
    Heap(const Heap&) = delete;
    ~Heap() { free(p); }
};

// src: exactly n readable bytes; dst: exactly cap writable bytes.  G: segments per group (0: the call's default); thr: the run
// threshold in bytes (0: the default).  Returns the block's size, or kLeft: the block is the one-wave decoder's.
static inline int train(const uint8_t* src, const int n, uint8_t* dst, const int cap, const int64_t maxIn, const int64_t maxOut,
                        int G, int thr, Stats* st)
{
    const int maxSeg = dx_max_seg(maxIn);
    if (G <= 0) G = dxb_group_for(maxSeg);
    if (thr <= 0) thr = kDxbThr;
    const size_t tStride = dx_t_stride(maxIn), pStride = dxb_ptr_stride(maxOut);
    const int groups = dxb_groups(maxSeg, G), room = dxb_run_room(maxIn, maxOut, thr), launched = dxb_rounds(maxOut);
    Heap<uint64_t> T(tStride), TG((size_t)groups * kDxSeg);
    Heap<uint32_t> ptr(pStride);
    Heap<DxUnit> units((size_t)maxSeg);
    Heap<DxbEntry> ent((size_t)groups);
    Heap<DxRun> list((size_t)room);
    uint32_t count = 0;
    st->launched = launched; st->taken = 0; st->runs = 0; st->groups = groups; st->room = room;
    const int nseg = dx_segments(n), jt = dx_tail_from(nseg);
    st->groups = (jt + G - 1) / G;
    for (size_t p = 0; p < pStride; ++p) ptr.p[p] = (uint32_t)p;                                       // k_dx_tables
    const bool misfit = nseg > maxSeg || (int64_t)n > (int64_t)tStride - 64 || (int64_t)cap > (int64_t)pStride - 64;
    if (n > 0 && !misfit) {
        for (int j = nseg - 1; j >= 0; --j) dx_segment_table(src, n, j, T.p);
        for (int g = groups - 1; g >= 0; --g)                                                          // k_dxb_compose
            if ((g + 1) * G <= jt) for (int sub = 127; sub >= 0; --sub) dxb_compose(T.p, TG.p, n, g, G, sub);
    }
    if (misfit || dxb_hop(src, n, cap, T.p, TG.p, ent.p, units.p, nseg, G) != 0) return kLeft;        // k_dxb_hop
    for (int g = groups - 1; g >= 0; --g) if (g * G < jt) dxb_group_units(src, n, T.p, ent.p, units.p, nseg, G, g);   // k_dxb_units
    DxRuns runs; runs.list = list.p; runs.count = &count; runs.room = room; runs.thr = thr;
    int64_t outLen = -1;
    for (int j = jt; j >= 0; --j) {                                                                    // k_dxb_fill
        if (j < jt && units.p[j].ip < 0) continue;
        const int64_t r = wave_dx_fill<false, true>(src, n, dst, cap, ptr.p, units.p[j].ip, units.p[j].op, units.p[j].stop, j == jt, &runs);
        if (r < 0) return kLeft;
        if (j == jt) outLen = r;
        else { int k = j + 1; while (k < jt && units.p[k].ip < 0) ++k; if (units.p[k].op != (int)r) return kUnitsDisagree; }
    }
    if (count > (uint32_t)room) return kListOverrun;                                                   // (a full list flags the block in the fill)
    st->runs = (int)count;
    for (uint32_t i = 0; i < count; ++i)                                                               // k_dxb_runs
        for (uint32_t c = dxb_run_pieces(list.p[i]); c-- > 0;) dxb_run_piece(list.p[i], c, src, dst, ptr.p);
    int r = 0;
    for (; r < launched; ++r) {                                                                        // k_dxb_jump
        bool moved = false;
        // (from the top down: no pointer sees one that was moved in this round -- the slowest the unordered workgroups can be)
        for (int p0 = (((int)outLen - 1) / 256) * 256; p0 >= 0; p0 -= 256) moved |= dx_jump(ptr.p, p0, (int)outLen);
        if (!moved) { ++r; break; }
    }
    st->taken = r;                                                                                     // (the round that saw nothing move included)
    for (int p0 = 0; p0 < (int)outLen; p0 += 256) dx_gather(dst, ptr.p, p0, (int)outLen);              // k_dxb_gather
    return (int)outLen;
}

}  // namespace dxbig
