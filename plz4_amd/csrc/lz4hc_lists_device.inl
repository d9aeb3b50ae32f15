// lz4hc_lists_device.inl -- chain, rank and list of lz4hc12_device.inl's phase 1, built in pieces by many workgroups per block.
//
// The arrays are a stable counting sort of a block's inserted positions by their hash (lz4hc12_device.inl:9-15, :55-61), so nothing
// about them is serial: cut the positions into pieces of `piece` positions and
//   count  per (block, piece): how many of the piece's positions every hash has                              (hb_count)
//   scan   per block: offsets[h] = the exclusive prefix of the totals over the hashes -- the array k_hc12_hist writes -- and per
//          (piece, hash) the piece's first list slot: offsets[h] + the counts of the pieces in front         (hb_total, hb_slots)
//   fill   per (block, piece), one wave: the step of hc12_build_lists over the piece's positions, the cursors starting at the
//          piece's slots: rank[p] and list[slot] = p | kHc12First                                            (hb_fill)
//   chain  per position: the distance to the list entry below its own, unless its entry carries the flag     (hb_chain)
// Every stage is a launch of its own; no workgroup waits for another one.  What comes out is what k_hc12_hist + k_hc12_chain write:
// the slot of a position is offsets[h] + the number of inserted positions of its hash below it, whoever counts them.
//
// Per-wave code on wave.h's macros: tests/emu/emu_hb.cpp compiles the same text with g++ and compares every array with
// hc12_build_lists's.
#pragma once
#include "lz4hc12_device.inl"

namespace plz4 {

// whether position p is inserted: four bytes to hash, and not one of an external segment's last three (hc12_build_lists)
DEV bool hb_inserted(int p, int nIns, int skipLo, int skipHi) { return p < nIns && !(p >= skipLo && p < skipHi); }

// ------------------------------------------------------------------------------------------ count
// One wave's share of a piece: the positions from + 64 j + lane, j = 0, stride / 64, ..., below `to`, counted per hash into `tab`
// (32768 counters in LDS, zeroed by the caller; the waves of a workgroup share it).
DEV void hb_count(const uint8_t* __restrict__ src, const int nIns, const int skipLo, const int skipHi,
                  const int from, const int to, const int stride, uint32_t* tab)
{
    for (int b = from; b < to; b += stride) {
        LANES({
            const int p = b + LANE;
            if (p < to && hb_inserted(p, nIns, skipLo, skipHi)) (void)lds_add_rtn(&tab[hc12_hash(ld32u(src + p))], 1u);
        })
    }
}

// ------------------------------------------------------------------------------------------ scan (per-thread code, one hash each)
// cnt / slot: the block's [piece][hash] arrays.  The total of hash h over the block's P pieces ...
DEV uint32_t hb_total(const uint32_t* __restrict__ cnt, const int P, const int h)
{
    uint32_t s = 0;
    for (int k = 0; k < P; ++k) s += cnt[(size_t)k * kHcHashEntries + h];
    return s;
}
// ... and, once offsets[h] = `run` is known, where every piece's positions of hash h start in the list
DEV void hb_slots(const uint32_t* __restrict__ cnt, uint32_t* __restrict__ slot, const int P, const int h, uint32_t run)
{
    for (int k = 0; k < P; ++k) { const size_t at = (size_t)k * kHcHashEntries + h; const uint32_t c = cnt[at]; slot[at] = run; run += c; }
}

// ------------------------------------------------------------------------------------------ fill
// One wave, the positions [lo, hi) of the block (lo % 1024 == 0; lo >= 1024 unless it is the first piece).  hc12_build_lists's two
// passes, tables and step, with two differences: the cursors start at the piece's slots (`slot`: this piece's 32768 entries), and
// the table of last positions starts at 1 -- "a position in front of this piece", below every value a piece behind the first one
// commits -- for a hash that an earlier piece holds, which is the case iff the piece's slot is not offsets[h].  A position then
// carries kHc12First iff nothing of its hash lies below it in the whole block, i.e. iff its slot is offsets[h].  The chain is not
// written here: a predecessor may lie in another piece (hb_chain).
DEV void hb_fill(const uint8_t* __restrict__ src, const int n, const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ slot,
                 uint32_t* __restrict__ rank, uint32_t* __restrict__ list, const int lo, const int hi,
                 uint32_t* lastT, uint32_t* curT, const int skipLo, const int skipHi)
{
    const int nAll = n >= 4 ? n - 3 : 0;
    const int nIns = nAll < hi ? nAll : hi;                    // this piece's positions end here
    for (int half = 0; half < 2; ++half) {
        LANES({
            for (int i = LANE; i < kHcHashEntries / 2; i += 64) {
                const int hh = half * (kHcHashEntries / 2) + i;
                const uint32_t s = slot[hh];
                curT[i] = s; lastT[i] = s != offsets[hh] ? 1u : 0u;
            }
        })
        LDS_FENCE();
        auto words = [&](LVREF(uint32_t, w), int b) { LANES({ const int p = b + LANE; w[I_] = p < nIns ? ld32u(src + p) : 0u; }) };
        auto step = [&](const int base, LVREF(uint32_t, w)) {
            LV(uint32_t, h); LV(uint32_t, prev); LV(uint32_t, sl); LV(int, act);
            LANES({
                const int p = base + LANE;
                act[I_] = 0; h[I_] = 0; prev[I_] = 0; sl[I_] = 0;
                if (hb_inserted(p, nIns, skipLo, skipHi)) {
                    const uint32_t hv = hc12_hash(w[I_]);
                    if ((int)(hv >> 14) == half) {
                        act[I_] = 1; h[I_] = hv & 16383u;
                        prev[I_] = lds_max_rtn(&lastT[h[I_]], (uint32_t)p + 1u);
                        sl[I_] = lds_add_rtn(&curT[h[I_]], 1u);
                    }
                }
            })
            LDS_ORDER();
            {   // in lane order, a lane whose predecessor is in this batch sits right behind it in the list (hc12_build_lists)
                LV(uint32_t, ps);
                LANES({ ps[I_] = SHFL(sl, (prev[I_] > (uint32_t)base) ? (int)(prev[I_] - 1u - (uint32_t)base) : LANE); })
                if (BALLOT(act[I_] && (prev[I_] > (uint32_t)(base + LANE) || (prev[I_] > (uint32_t)base && sl[I_] != ps[I_] + 1u)))) {
                    LV(uint32_t, gmin); LV(uint32_t, smin); LV(uint32_t, near); LV(uint32_t, idx);
                    LANES({ gmin[I_] = prev[I_]; smin[I_] = sl[I_]; near[I_] = 0; idx[I_] = 0; })
                    for (int l = 0; l < 64; ++l) {
                        const uint32_t hl = RL(h, l), pl = RL(prev, l), sv = RL(sl, l); const int al = RL(act, l);
                        LANES({
                            if (al && act[I_] && h[I_] == hl) {
                                if (pl < gmin[I_]) gmin[I_] = pl;
                                if (sv < smin[I_]) smin[I_] = sv;
                                if (l < LANE) { near[I_] = (uint32_t)(base + l) + 1u; idx[I_]++; }
                            }
                        })
                    }
                    LANES({ prev[I_] = near[I_] ? near[I_] : gmin[I_]; sl[I_] = smin[I_] + idx[I_]; })
                }
            }
            LANES({
                const int p = base + LANE;
                if (act[I_]) {
                    rank[p] = sl[I_];
                    list[sl[I_]] = (uint32_t)p | (prev[I_] ? 0u : kHc12First);
                }
            })
        };
        // sixteen steps' words in flight, as in hc12_build_lists
#define HB_W16(F) F(0) F(1) F(2) F(3) F(4) F(5) F(6) F(7) F(8) F(9) F(10) F(11) F(12) F(13) F(14) F(15)
#define HB_DECL(k)  LV(uint32_t, w##k); LV(uint32_t, n##k);
#define HB_FIRST(k) words(w##k, lo + 64 * k);
#define HB_NEXT(k)  words(n##k, base + 1024 + 64 * k);
#define HB_STEP(k)  if (base + 64 * k < nIns) step(base + 64 * k, w##k);
#define HB_MOVE(k)  LANES({ w##k[I_] = n##k[I_]; })
        HB_W16(HB_DECL)
        HB_W16(HB_FIRST)
        for (int base = lo; base < nIns; base += 1024) {
            HB_W16(HB_NEXT)
            HB_W16(HB_STEP)
            HB_W16(HB_MOVE)
        }
#undef HB_W16
#undef HB_DECL
#undef HB_FIRST
#undef HB_NEXT
#undef HB_STEP
#undef HB_MOVE
        LDS_FENCE();
    }
}

// ------------------------------------------------------------------------------------------ chain
// One wave, the 64 positions from `base` (base + 64 <= nPad): chain[p] as lz4hc12_device.inl:55-58 defines it -- the distance to the
// previous inserted position of the same hash, which is the list entry below p's own unless p's carries the flag; 0 for "none
// within 65535" and for positions that are not inserted.
DEV void hb_chain(const int n, const int skipLo, const int skipHi, uint16_t* __restrict__ chain, const uint32_t* __restrict__ rank,
                  const uint32_t* __restrict__ list, const int base)
{
    const int nIns = n >= 4 ? n - 3 : 0;
    LANES({
        const int p = base + LANE;
        uint32_t d = 0;
        if (hb_inserted(p, nIns, skipLo, skipHi)) {
            const uint32_t r = rank[p];
            if (!(list[r] & kHc12First)) {
                const uint32_t dist = (uint32_t)p - (list[r - 1u] & ~kHc12First);
                d = dist <= 65535u ? dist : 0u;
            }
        }
        chain[p] = (uint16_t)d;
    })
}

}  // namespace plz4
