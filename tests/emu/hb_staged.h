// The four stages of plz4_amd/csrc/lz4hc_lists_device.inl run back to back on the CPU, as k_hb_count .. k_hb_chain run them (the same
// geometry: HbLayout's arrays, a 16-wave workgroup per piece for the count, a thread per hash for the scan, one wave per piece for
// the fill, a wave per 64 positions for the chain), beside the two things they are compared with: hc12_build_lists fed by the
// histogram, and a loop written from the definition.  Shared by emu_hb.cpp and hb_bounds_main.cpp (PLZ4_EMU is defined by them).
// Every array is a heap allocation of exactly the size the kernels' layouts give; the source has exactly n bytes.
#pragma once
#include "../../plz4_amd/csrc/lz4_device.inl"
#include "../../plz4_amd/csrc/lz4_seq_device.inl"
#include "../../plz4_amd/csrc/lz4hc_device.inl"
#include "../../plz4_amd/csrc/lz4hc12_device.inl"
#include "../../plz4_amd/csrc/lz4hc_lazy_device.inl"
#include "../../plz4_amd/csrc/lz4hcx_device.inl"
#include "../../plz4_amd/csrc/lz4_dx_device.inl"
#include "../../plz4_amd/csrc/lz4_fx_device.inl"
#include "../../plz4_amd/csrc/lz4hc_lists_device.inl"
#include "../../plz4_amd/csrc/ws_layout.h"
#include "../../plz4_amd/csrc/route.h"
#include <stdlib.h>
#include <string.h>

namespace hbt {
using namespace plz4;

struct Arrays {
    int n, nPad;
    uint8_t* src; uint16_t* chain; uint32_t* rank; uint32_t* listBase; uint32_t* offsets;
    uint32_t* list() const { return listBase + 8; }
    Arrays(const uint8_t* s, int n_) : n(n_)
    {
        nPad = (n + 1 + 1023) / 1024 * 1024;
        src = (uint8_t*)malloc(n > 0 ? (size_t)n : 1);
        if (n > 0) memcpy(src, s, (size_t)n);
        chain = (uint16_t*)malloc((size_t)nPad * 2); memset(chain, 0xA5, (size_t)nPad * 2);
        rank = (uint32_t*)malloc((size_t)nPad * 4); memset(rank, 0xA5, (size_t)nPad * 4);
        listBase = (uint32_t*)malloc(((size_t)nPad + 8) * 4); memset(listBase, 0xA5, ((size_t)nPad + 8) * 4);
        offsets = (uint32_t*)malloc((size_t)kHcHashEntries * 4); memset(offsets, 0xA5, (size_t)kHcHashEntries * 4);
    }
    ~Arrays() { free(src); free(chain); free(rank); free(listBase); free(offsets); }
    Arrays(const Arrays&) = delete;
};
inline int n_ins(int n) { return n >= 4 ? n - 3 : 0; }

// count -> scan -> fill -> chain; the pieces of count and fill in ascending or descending order
inline void staged(Arrays& A, int piece, int skipLo, int skipHi, bool piecesDescending)
{
    const int nIns = n_ins(A.n);
    const int P = (nIns + piece - 1) / piece;
    const HbLayout L = hb_layout(1, P > 0 ? P : 1);
    uint8_t* const ws = (uint8_t*)malloc(L.total);
    memset(ws, 0xA5, L.total);
    uint32_t* const cnt = (uint32_t*)(ws + L.offCnt);
    uint32_t* const slot = (uint32_t*)(ws + L.offSlot);
    uint32_t* const tab = (uint32_t*)malloc((size_t)kHcHashEntries * 4);
    uint32_t* const lastT = (uint32_t*)malloc((size_t)kHcHashEntries / 2 * 4);
    uint32_t* const curT = (uint32_t*)malloc((size_t)kHcHashEntries / 2 * 4);
    for (int j = 0; j < P; ++j) {
        const int k = piecesDescending ? P - 1 - j : j;
        memset(tab, 0, (size_t)kHcHashEntries * 4);
        for (int w = 0; w < 16; ++w) hb_count(A.src, nIns, skipLo, skipHi, k * piece + 64 * w, (k + 1) * piece, 1024, tab);
        memcpy(cnt + (size_t)k * kHcHashEntries, tab, (size_t)kHcHashEntries * 4);
    }
    {
        uint32_t run = 0;
        for (int h = 0; h < kHcHashEntries; ++h) { tab[h] = run; A.offsets[h] = run; run += hb_total(cnt, P, h); }
        for (int h = 0; h < kHcHashEntries; ++h) hb_slots(cnt, slot, P, h, tab[h]);
    }
    for (int j = 0; j < P; ++j) {
        const int k = piecesDescending ? P - 1 - j : j;
        hb_fill(A.src, A.n, A.offsets, slot + (size_t)k * kHcHashEntries, A.rank, A.list(), k * piece, (k + 1) * piece, lastT, curT, skipLo, skipHi);
    }
    for (int base = 0; base < A.nPad; base += 64) hb_chain(A.n, skipLo, skipHi, A.chain, A.rank, A.list(), base);
    free(ws); free(tab); free(lastT); free(curT);
}

// what k_hc12_hist + k_hc12_chain do (tests/emu/emu_kernels.cpp, H12Emu)
inline void one_wave(Arrays& A, int skipLo, int skipHi)
{
    const int nIns = n_ins(A.n);
    memset(A.offsets, 0, (size_t)kHcHashEntries * 4);
    for (int p = 0; p < nIns; ++p) if (!(p >= skipLo && p < skipHi)) A.offsets[hc12_hash(ld32u(A.src + p))]++;
    uint32_t run = 0;
    for (int h = 0; h < kHcHashEntries; ++h) { const uint32_t c = A.offsets[h]; A.offsets[h] = run; run += c; }
    uint32_t* lastT = (uint32_t*)malloc(kHcHashEntries / 2 * 4); uint32_t* curT = (uint32_t*)malloc(kHcHashEntries / 2 * 4);
    hc12_build_lists(A.src, A.n, A.offsets, A.chain, A.rank, A.list(), A.nPad, lastT, curT, skipLo, skipHi);
    free(lastT); free(curT);
}

// the definition: the last position per hash (the hash of lz4hc.c:120-122, written out once more)
inline uint32_t def_hash(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return (uint32_t)(v * 2654435761u) >> 17; }
inline void by_definition(Arrays& A, int skipLo, int skipHi)
{
    const int nIns = n_ins(A.n);
    std::vector<int> last(kHcHashEntries, -1), prev((size_t)nIns + 1, -1);
    std::vector<uint32_t> count(kHcHashEntries, 0);
    for (int p = 0; p < A.nPad; ++p) A.chain[p] = 0;
    for (int p = 0; p < nIns; ++p) {
        if (p >= skipLo && p < skipHi) continue;
        const uint32_t h = def_hash(A.src + p);
        prev[p] = last[h]; last[h] = p; count[h]++;
        A.chain[p] = (uint16_t)(prev[p] >= 0 && p - prev[p] <= 65535 ? p - prev[p] : 0);
    }
    uint32_t run = 0;
    for (int h = 0; h < kHcHashEntries; ++h) { A.offsets[h] = run; run += count[h]; }
    for (int p = 0; p < nIns; ++p) {
        if (p >= skipLo && p < skipHi) continue;
        A.rank[p] = prev[p] < 0 ? A.offsets[def_hash(A.src + p)] : A.rank[prev[p]] + 1u;
        A.list()[A.rank[p]] = (uint32_t)p | (prev[p] < 0 ? 0x80000000u : 0u);
    }
}

// 0: equal in offsets, chain[0, nPad), rank of every inserted position and list[0, count) with its flags; else which one differs
inline int differ(const Arrays& X, const Arrays& Y, int skipLo, int skipHi)
{
    const int nIns = n_ins(X.n);
    if (memcmp(X.offsets, Y.offsets, (size_t)kHcHashEntries * 4)) return 1;
    if (memcmp(X.chain, Y.chain, (size_t)X.nPad * 2)) return 2;
    uint32_t count = 0;
    for (int p = 0; p < nIns; ++p) if (!(p >= skipLo && p < skipHi)) { if (X.rank[p] != Y.rank[p]) return 3; count++; }
    if (memcmp(X.list(), Y.list(), (size_t)count * 4)) return 4;
    return 0;
}

// staged (both piece orders) against both references.  0: all equal; 10 * who + what otherwise
inline int compare(const uint8_t* src, int n, int piece, int skipLo, int skipHi)
{
    Arrays D(src, n), W(src, n);
    by_definition(D, skipLo, skipHi);
    one_wave(W, skipLo, skipHi);
    if (int r = differ(W, D, skipLo, skipHi)) return 10 + r;
    for (int desc = 0; desc < 2; ++desc) {
        Arrays S(src, n);
        staged(S, piece, skipLo, skipHi, desc != 0);
        if (int r = differ(S, D, skipLo, skipHi)) return 20 + 10 * desc + r;
        if (int r = differ(S, W, skipLo, skipHi)) return 40 + 10 * desc + r;
    }
    return 0;
}

}  // namespace hbt
