// The decoders on hostile input read no byte outside [src, src + n), the dictionary or window, and write no byte outside
// [dst, dst + cap): a program of its own for the address and undefined-behaviour sanitizers (never loaded into Python, never run on a
// GPU; the build + run line is in scripts/README.md).  Every buffer the device code sees is a heap allocation of exactly the size the
// product gives it -- the source at every start offset modulo 16 by padding in FRONT only, so that its end is the allocation's end;
// destination, dictionary, windows, LDS staging and the few-block path's workspaces with no padding at all -- and what a decoder
// answers is checked against the oracle (oracle/plz4_oracle.c), result codes included.  Paths:
//   1  wave_decode_block<true> and <false>, no dictionary                   (k_decode_rec, k_decode_raw)
//   2  the same against a dictionary of 1 .. 65536 bytes                     (k_decode_raw_dict, decode_one_record)
//   3  the few-block train on the caller's bytes in place                    (k_dx_tables .. k_dx_gather)
//   4  the train with history outside the block, one call of a few records   (k_dx_rec_prep, k_dxl_*; linked chain behind a window,
//      dictionary; a damaged block or a record with a lying size word at each place of the call)
//   5  the record head (rec_head) on records of 0 .. 11 bytes at the end of a body
// Inputs: blocks built sequence by sequence around the vector path's boundaries (tests/lz4blocks.py is the same generator), then
// truncated, bit-flipped, 0xFF-ed and with zeroed offsets, over the reference's end-of-output margins as capacities.
// `--long`: a wider set (minutes).  Prints one line of counts; exit status 1 on a wrong answer, the sanitizer's on a bad access.
#define PLZ4_EMU 1
#include "../../plz4_amd/csrc/lz4_dx_device.inl"
#include "../../oracle/plz4_oracle.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

int plz4_emu_descending = 0;

using namespace plz4;

namespace {

struct Rng {
    uint32_t s;
    uint32_t next() { s = s * 1664525u + 1013904223u; return s >> 8; }
    int below(int n) { return n > 0 ? (int)(next() % (uint32_t)n) : 0; }
    int range(int lo, int hi) { return lo + below(hi - lo); }                  // [lo, hi)
    double unit() { return next() / 16777216.0; }
};

// exactly n bytes that end where the allocation ends; `front` bytes of padding before them (0: they start where it starts, too)
struct Exact {
    uint8_t* base; uint8_t* p; size_t n;
    Exact(size_t n_, int front = 0) : n(n_)
    {
        if (n + (size_t)front == 0) front = 16;                                 // (malloc(0) may be null: keep a pointer whose every byte is out of bounds)
        base = (uint8_t*)malloc(n + (size_t)front);
        if (!base) { fprintf(stderr, "out of memory\n"); exit(2); }
        p = base + front;
    }
    Exact(const Exact&) = delete;
    ~Exact() { free(base); }
};

struct Block { std::vector<uint8_t> comp, plain; std::vector<int> offAt; };

const int kLL[] = {0, 0, 1, 2, 3, 5, 7, 12, 13, 14, 15, 16, 17, 30, 45, 47, 48, 49, 62, 63, 64, 100, 254 + 15, 255 + 15, 300, 600};
const int kML[] = {4, 4, 5, 6, 8, 12, 17, 18, 19, 20, 33, 64, 100, 272, 273, 274, 275, 528, 529, 1000};

void put_len(std::vector<uint8_t>& out, int v) { while (v >= 255) { out.push_back(255); v -= 255; } out.push_back((uint8_t)v); }

// a valid block of nseq sequences that ends the way liblz4 requires; dictLen > 0: a third of the offsets reach in front of the block,
// into the last bytes of dict (matches that start there end there or run on into the block)
Block make_block(Rng& r, int nseq, const uint8_t* dict = nullptr, int dictLen = 0)
{
    Block b;
    for (int s = 0; s < nseq; ++s) {
        int ll = r.unit() < 0.7 ? kLL[r.below(26)] : r.range(0, 40);
        const int ml = r.unit() < 0.6 ? kML[r.below(20)] : r.range(4, 40);
        if (b.plain.empty() && ll == 0 && dictLen == 0) ll = 1;
        const int have = (int)b.plain.size() + ll;
        const double kind = r.unit();
        int off;
        const int reach = have + dictLen < 65535 ? have + dictLen : 65535;
        if (dictLen > 0 && (have == 0 || (kind >= 0.67 && reach > have))) off = r.range(have + 1, reach + 1);
        else if (kind < 0.25) off = r.range(1, (have < 8 ? have : 8) + 1);
        else if (kind < 0.55) off = r.range(1, (have < 64 ? have : 64) + 1);
        else if (kind < 0.8)  off = r.range(1, (have < 2000 ? have : 2000) + 1);
        else                  off = r.range(1, (have < 65535 ? have : 65535) + 1);
        b.comp.push_back((uint8_t)(((ll < 15 ? ll : 15) << 4) | (ml - 4 < 15 ? ml - 4 : 15)));
        if (ll >= 15) put_len(b.comp, ll - 15);
        for (int i = 0; i < ll; ++i) { const uint8_t v = (uint8_t)r.next(); b.comp.push_back(v); b.plain.push_back(v); }
        b.offAt.push_back((int)b.comp.size());
        b.comp.push_back((uint8_t)(off & 0xFF)); b.comp.push_back((uint8_t)(off >> 8));
        if (ml - 4 >= 15) put_len(b.comp, ml - 4 - 15);
        const int start = (int)b.plain.size() - off;
        for (int i = 0; i < ml; ++i) b.plain.push_back(start + i < 0 ? dict[dictLen + start + i] : b.plain[(size_t)(start + i)]);
    }
    const int tail = r.range(12, 40);
    b.comp.push_back((uint8_t)((tail < 15 ? tail : 15) << 4));
    if (tail >= 15) put_len(b.comp, tail - 15);
    for (int i = 0; i < tail; ++i) { const uint8_t v = (uint8_t)r.next(); b.comp.push_back(v); b.plain.push_back(v); }
    return b;
}

long nWave = 0, nDict = 0, nDx = 0, nDxTaken = 0, nDxl = 0, nDxlTaken = 0, nHead = 0;
int  srcShift = 0;                                                          // the next source's start offset modulo 16

[[noreturn]] void wrong(const char* what, int caseNo, int n, int cap, int got, int want)
{
    fprintf(stderr, "WRONG ANSWER: %s, case %d: n %d cap %d: %d, the oracle says %d\n", what, caseNo, n, cap, got, want);
    exit(1);
}

// paths 1 and 2: both builds of the one-wave decoder and the oracle
void run_wave(const std::vector<uint8_t>& comp, int n, int cap, const uint8_t* dict, int dictLen, int caseNo)
{
    Exact src((size_t)n, srcShift++ & 15);
    if (n) memcpy(src.p, comp.data(), (size_t)n);
    Exact d1((size_t)cap), d2((size_t)cap), d3((size_t)cap), lds(kDecLdsBytes);
    const int want = dictLen > 0 ? orc_decompress_safe_dict(src.p, n, d3.p, cap, dict, dictLen) : orc_decompress_safe(src.p, n, d3.p, cap);
    const int r1 = wave_decode_block<true>(src.p, n, d1.p, cap, dict, dictLen, lds.p);
    const int r2 = wave_decode_block<false>(src.p, n, d2.p, cap, dict, dictLen);
    if (r1 != want) wrong("wave_decode_block<true>", caseNo, n, cap, r1, want);
    if (r2 != want) wrong("wave_decode_block<false>", caseNo, n, cap, r2, want);
    if (want > 0 && (memcmp(d1.p, d3.p, (size_t)want) || memcmp(d2.p, d3.p, (size_t)want))) wrong("wave_decode_block: bytes", caseNo, n, cap, r1, want);
    if (memcmp(src.p, comp.data(), (size_t)n)) wrong("wave_decode_block: source changed", caseNo, n, cap, r1, want);
    (dictLen > 0 ? nDict : nWave)++;
}

// path 3: the stage train of launch_decode for one block of a call whose longest input is maxIn and whose largest capacity is
// maxOut, on the caller's bytes; what it declines is the one-wave decoder's
void run_dx(const std::vector<uint8_t>& comp, int n, int cap, int caseNo)
{
    Exact src((size_t)n, srcShift++ & 15);
    if (n) memcpy(src.p, comp.data(), (size_t)n);
    const int64_t maxIn = n > 0 ? n : 1, maxOut = cap > 0 ? cap : 1;
    const size_t tStride = dx_t_stride(maxIn), pStride = dx_ptr_stride(maxOut);
    const int maxSeg = dx_max_seg(maxIn), nseg = dx_segments(n), jt = dx_tail_from(nseg);
    Exact Tb(tStride * 8), Pb(pStride * 4), Ub((size_t)maxSeg * sizeof(DxUnit)), dst((size_t)cap), d3((size_t)cap);
    uint64_t* const T = (uint64_t*)Tb.p; uint32_t* const ptr = (uint32_t*)Pb.p; DxUnit* const units = (DxUnit*)Ub.p;
    for (size_t p = 0; p < pStride; ++p) ptr[p] = (uint32_t)p;                         // k_dx_tables
    if (n > 0 && (int64_t)n <= (int64_t)tStride - 64) for (int j = nseg - 1; j >= 0; --j) dx_segment_table(src.p, n, j, T);
    int64_t outLen = -1;
    bool bad = nseg > maxSeg || (int64_t)n > (int64_t)tStride - 64 || (int64_t)cap > (int64_t)pStride - 64 || dx_stitch(src.p, n, cap, T, units, nseg) != 0;   // k_dx_stitch
    for (int j = jt; j >= 0 && !bad; --j) {                                             // k_dx_fill
        if (j < jt && units[j].ip < 0) continue;
        const int64_t r = wave_dx_fill(src.p, n, dst.p, cap, ptr, units[j].ip, units[j].op, units[j].stop, j == jt);
        if (r < 0) { bad = true; break; }
        if (j == jt) outLen = r;
        else { int k = j + 1; while (k < jt && units[k].ip < 0) ++k; if (units[k].op != (int)r) wrong("dx: units do not meet", caseNo, n, cap, (int)r, units[k].op); }
    }
    ++nDx;
    if (bad) return;
    for (int rounds = 0; rounds < kDxRounds; ++rounds) {                                // k_dx_jump
        bool moved = false;
        for (int p0 = (((int)outLen - 1) / 256) * 256; p0 >= 0; p0 -= 256) moved |= dx_jump(ptr, p0, (int)outLen);
        if (!moved) break;
    }
    for (int p0 = 0; p0 < (int)outLen; p0 += 256) dx_gather(dst.p, ptr, p0, (int)outLen);  // k_dx_gather
    const int want = orc_decompress_safe(src.p, n, d3.p, cap);
    if ((int)outLen != want) wrong("dx", caseNo, n, cap, (int)outLen, want);
    if (want > 0 && memcmp(dst.p, d3.p, (size_t)want)) wrong("dx: bytes", caseNo, n, cap, (int)outLen, want);
    ++nDxTaken;
}

// path 4: one call of nb records [LE32 size][payload] in a body of exactly their total length, as launch_decode runs it for blocks
// with history outside the block (emu_dxl.cpp is the same train on copies).  linked: one chain behind the window hist[0 .. histLen);
// else independent blocks under the dictionary hist.  Expected: the oracle block by block, the window kept as compress.DictT.Update
// keeps it; a chain's blocks behind its first bad one are CORRUPT with result 0.  lie >= 0: that record's size word says bsz + 1, so
// the frame reader turns it away (SIZE_OVERFLOW, result 0): its output, and in a chain that of every block behind it, stays as it was.
// The outputs lie at a stride of the largest capacity in one allocation, as the product's do, so the bytes between a block's capacity
// and the next block's output are prefilled and looked at afterwards.
void run_dxl(const std::vector<std::vector<uint8_t>>& recs, const std::vector<int>& caps, const bool linked, const uint8_t* hist, const int histLen,
             const int caseNo, const int lie = -1)
{
    const uint8_t kFill = 0xA5;
    const int nb = (int)recs.size();
    size_t total = 0; int bsz = 1, maxCap = 1;
    std::vector<int64_t> off(nb + 1, 0);
    for (int i = 0; i < nb; ++i) { off[i] = (int64_t)total; total += 4 + recs[i].size(); if ((int)recs[i].size() > bsz) bsz = (int)recs[i].size(); if (caps[i] > maxCap) maxCap = caps[i]; }
    off[nb] = (int64_t)total;
    Exact body(total, srcShift++ & 15);
    for (int i = 0; i < nb; ++i) { st32u(body.p + off[i], i == lie ? (uint32_t)bsz + 1u : (uint32_t)recs[i].size()); if (!recs[i].empty()) memcpy(body.p + off[i] + 4, recs[i].data(), recs[i].size()); }
    const size_t tStride = dx_t_stride(bsz), P = dx_ptr_stride(maxCap);
    const int maxSeg = dx_max_seg(bsz);
    const int64_t dstStride = maxCap;
    Exact Tb((size_t)nb * tStride * 8), Pb((size_t)nb * P * 4), Ub((size_t)nb * maxSeg * sizeof(DxUnit)), dst((size_t)nb * dstStride), win(131072), winRef(65536);
    Exact dictCopy(linked ? 0 : (size_t)histLen);
    std::vector<DxInfo> info(nb); std::vector<int32_t> len(nb), first(nb, 0), chain(nb, 0);
    std::vector<uint32_t> moved((size_t)nb * (kDxlMaxRounds + 1), 0);
    uint64_t* const T = (uint64_t*)Tb.p; uint32_t* const ptr = (uint32_t*)Pb.p; DxUnit* const units = (DxUnit*)Ub.p;
    int winLen = linked ? histLen : 0;
    memset(dst.p, kFill, (size_t)nb * (size_t)dstStride);
    if (linked) { if (histLen) memcpy(win.p, hist, (size_t)histLen); }
    else { if (histLen) memcpy(dictCopy.p, hist, (size_t)histLen); for (int i = 0; i < nb; ++i) first[i] = i; }
    DxlCall c;
    c.ptr = ptr; c.P = (int64_t)P; c.nb = nb; c.info = info.data(); c.len = len.data(); c.first = first.data(); c.chain = chain.data();
    if (linked) { c.hist = win.p; c.histStride = 131072; c.histLen = &winLen; c.histLenAll = 0; }
    else { c.hist = dictCopy.p; c.histStride = 0; c.histLen = nullptr; c.histLenAll = histLen; }
    c.dst = dst.p; c.dstStride = dstStride;
    for (int b = 0; b < nb; ++b) {
        len[b] = dx_rec_len(body.p + off[b], off[b + 1] - off[b], bsz, false, maxCap);  // k_dx_rec_prep
        const uint8_t* const s = body.p + off[b] + 4; const int n = len[b];
        for (size_t p = 0; p < P; ++p) ptr[(size_t)b * P + p] = (uint32_t)p;             // k_dx_tables, k_dx_stitch, k_dxl_fill
        const int nseg = dx_segments(n), jt = dx_tail_from(nseg);
        DxUnit* const u = units + (size_t)b * maxSeg;
        info[b].bad = 1; info[b].outLen = 0; info[b].tailFrom = jt;
        if (n <= 0) continue;
        for (int j = nseg - 1; j >= 0; --j) dx_segment_table(s, n, j, T + (size_t)b * tStride);
        if (linked && dxl_chain_dead(len.data(), 0, b, 0)) continue;                    // k_dxl_link
        if (nseg > maxSeg || caps[b] > (int64_t)P - 64 || dx_stitch(s, n, caps[b], T + (size_t)b * tStride, u, nseg) != 0) continue;
        bool bad = false;
        for (int j = jt; j >= 0 && !bad; --j) {
            if (j < jt && u[j].ip < 0) continue;
            const int64_t r = wave_dx_fill<true>(s, n, dst.p + (int64_t)b * dstStride, caps[b], ptr + (size_t)b * P, u[j].ip, u[j].op, u[j].stop, j == jt);
            if (r < 0) { bad = true; break; }
            if (j == jt) info[b].outLen = (int)r;
            else { int k = j + 1; while (k < jt && u[k].ip < 0) ++k; if (u[k].op != (int)r) wrong("dxl: units do not meet", caseNo, n, caps[b], (int)r, u[k].op); }
        }
        info[b].bad = bad ? 1 : 0;
    }
    for (int b = nb - 1; b >= 0; --b)                                                   // k_dxl_resolve
        for (int64_t p0 = 0; p0 < (int64_t)P; p0 += 256) if (!dxl_resolve(c, b, (int)p0, (int)P)) info[b].bad = 1;
    int rounds = 1;
    while (rounds < kDxlMaxRounds && ((int64_t)1 << (rounds - 1)) < (int64_t)nb * maxCap + kDxlHist) ++rounds;
    const uint32_t hist0 = dxl_hist0(c);
    for (int r = 0; r < rounds; ++r)                                                    // k_dxl_jump
        for (int b = nb - 1; b >= 0; --b) {
            uint32_t* const mv = &moved[(size_t)b * (kDxlMaxRounds + 1)];
            if (info[b].bad || (r > 0 && !mv[r - 1])) continue;
            const int outLen = info[b].outLen;
            for (int p0 = outLen > 0 ? ((outLen - 1) / 256) * 256 : -1; p0 >= 0; p0 -= 256)
                if (dxl_jump(ptr, hist0, (uint32_t)((int64_t)b * (int64_t)P), p0, outLen)) mv[r] = 1u;
        }
    for (int b = 0; b < nb; ++b) if (!info[b].bad) for (int p0 = 0; p0 < info[b].outLen; p0 += 256) dxl_gather(c, b, p0, info[b].outLen);   // k_dxl_gather
    std::vector<int32_t> result(nb, 0), status(nb, 0);
    DxlFin f; f.hashBad = nullptr; f.moved = moved.data(); f.rounds = rounds; f.result = result.data(); f.status = status.data();
    Exact lds(kDecLdsBytes);
    auto rec = [&](int i, const uint8_t* h, int hl, int* r, int* st, bool* stored) {     // decode_one_record, without checksums
        uint32_t word;
        const uint8_t* const rp = body.p + off[i];
        const int sz = rec_head<true>(rp, off[i + 1] - off[i], bsz, false, &word);
        *stored = false; *r = 0; *st = 0;
        if (sz < 0) { *st = 2; return; }
        *r = wave_decode_block<true>(rp + 4, sz, dst.p + (int64_t)i * dstStride, caps[i], h, hl, lds.p);
        if (*r < 0) *st = kDxlStCorrupt;
    };
    int taken = 0;
    if (linked) {                                                                       // k_dxl_finish
        int dead = 0, rr = 0;
        dxl_finish(c, f, rec, 0, nb, win.p, &winLen, &dead, &taken, &rr);
    } else {                                                                            // k_dxl_verdict, k_decode_rec_dict
        for (int b = 0; b < nb; ++b) {
            if (dxl_block_good(c, f, b)) { result[b] = info[b].outLen; status[b] = 0; ++taken; continue; }
            int r, st; bool stored;
            rec(b, histLen > 0 ? dictCopy.p : nullptr, histLen, &r, &st, &stored);
            result[b] = r; status[b] = st;
        }
    }
    // the oracle, block by block
    int wl = linked ? histLen : 0; bool dead = false;
    if (linked && histLen) memcpy(winRef.p, hist, (size_t)histLen);
    for (int b = 0; b < nb; ++b) {
        Exact d3((size_t)caps[b]);
        int want = 0, wantSt = kDxlStCorrupt;
        if (!dead && b == lie) { want = 0; wantSt = 2; }
        else if (!dead) {
            const uint8_t* const h = linked ? winRef.p : hist; const int hl = linked ? wl : histLen;
            want = hl > 0 ? orc_decompress_safe_dict(recs[b].data(), (int)recs[b].size(), d3.p, caps[b], h, hl)
                          : orc_decompress_safe(recs[b].data(), (int)recs[b].size(), d3.p, caps[b]);
            wantSt = want < 0 ? kDxlStCorrupt : 0;
        }
        if (result[b] != want || status[b] != wantSt) wrong(linked ? "dxl linked" : "dxl dictionary", caseNo, (int)recs[b].size(), caps[b], result[b], want);
        if (want > 0 && memcmp(dst.p + (int64_t)b * dstStride, d3.p, (size_t)want)) wrong("dxl: bytes", caseNo, (int)recs[b].size(), caps[b], result[b], want);
        {   // no byte behind the capacity, and none at all where the block is not decoded
            const uint8_t* const area = dst.p + (int64_t)b * dstStride;
            const bool alone = b == lie || (linked && lie >= 0 && b > lie);           // (behind a damaged payload the path has decoded side by side)
            for (int64_t q = alone ? 0 : caps[b]; q < dstStride; ++q)
                if (area[q] != kFill) wrong("dxl: a byte outside the block's output is written", caseNo, (int)recs[b].size(), caps[b], (int)q, b);
        }
        if (linked && wantSt) dead = true;
        if (linked && !dead && want > 0) {                                              // compress.DictT.Update
            std::vector<uint8_t> cat(winRef.p, winRef.p + wl);
            cat.insert(cat.end(), d3.p, d3.p + want);
            const size_t keep = cat.size() < 65536 ? cat.size() : 65536;
            memcpy(winRef.p, cat.data() + (cat.size() - keep), keep); wl = (int)keep;
        }
    }
    if (linked && (winLen != wl || memcmp(win.p, winRef.p, (size_t)wl))) wrong("dxl linked: the window", caseNo, nb, 0, winLen, wl);
    ++nDxl; nDxlTaken += taken;
}

// path 5: the record head on a record of recLen bytes at the very end of an exact-size body, then what its callers read behind it
void run_heads()
{
    const int bsz = 3;
    const uint32_t sizes[] = {0u, (uint32_t)bsz, (uint32_t)bsz + 1u, 0x7FFFFFFFu};
    for (int recLen = 0; recLen <= 11; ++recLen) for (int cks = 0; cks < 2; ++cks) for (int stored = 0; stored < 2; ++stored) for (uint32_t szw : sizes) {
        const int lead = 9;                                                 // a record in front: the short one is not the body's first
        Exact body((size_t)lead + (size_t)recLen, srcShift++ & 15);
        memset(body.p, 0x5A, (size_t)lead);
        const uint32_t w = szw | (stored ? 0x80000000u : 0u);
        uint8_t full[12]; memset(full, 0xC3, sizeof full); memcpy(full, &w, 4);
        memcpy(body.p + lead, full, (size_t)recLen);
        const uint8_t* const rec = body.p + lead;
        int want = -1;
        if (recLen >= 4 && (int64_t)szw <= bsz && (int64_t)szw + 4 + (cks ? 4 : 0) <= recLen) want = (int)szw;
        for (int uni = 0; uni < 2; ++uni) {
            uint32_t word = 0;
            const int got = uni ? rec_head<true>(rec, recLen, bsz, cks != 0, &word) : rec_head<false>(rec, recLen, bsz, cks != 0, &word);
            if (got != want || (recLen >= 4 && word != w)) wrong("rec_head", recLen, recLen, cks, got, want);
            if (got >= 0) {                                                  // payload and checksum word, as the decoders read them
                volatile uint32_t sink = wave_xxh32(rec + 4, got);
                if (cks) sink = sink ^ ld32u(rec + 4 + got);
                (void)sink;
            }
            ++nHead;
        }
    }
}

std::vector<int> capacities(int p)
{
    const int c[] = {p, p + 1, p + 8, p - 1, p - 5, p - 12, p - 32, p - 64, p / 2, p + 1088, 0};
    std::vector<int> out;
    for (int v : c) if (v >= 0) out.push_back(v);
    return out;
}

// the damaged copies of a block: (bytes, length)
struct Variant { std::vector<uint8_t> bytes; int n; };
std::vector<Variant> variants(Rng& r, const Block& b, const bool wide)
{
    std::vector<Variant> v;
    const int n = (int)b.comp.size();
    v.push_back({b.comp, n});
    if (n < 300) for (int k = 0; k < n; ++k) v.push_back({b.comp, k});       // truncated to every length
    else for (int k = 1; k <= 200 && k < n; ++k) v.push_back({b.comp, n - k});
    const int flips = wide ? 256 : (n < 2048 ? 24 : 12);
    for (int i = 0; i < flips; ++i) { Variant x{b.comp, n}; x.bytes[(size_t)r.below(n)] ^= (uint8_t)(1u << r.below(8)); v.push_back(x); }
    for (int i = 0; i < flips / 3; ++i) { Variant x{b.comp, n}; x.bytes[(size_t)r.below(n)] = 0xFF; v.push_back(x); }
    for (int i = 0; i < flips / 3 && !b.offAt.empty(); ++i) {                // an offset of 0
        Variant x{b.comp, n}; const int at = b.offAt[(size_t)r.below((int)b.offAt.size())]; x.bytes[(size_t)at] = 0; x.bytes[(size_t)at + 1] = 0; v.push_back(x);
    }
    return v;
}

}  // namespace

int main(int argc, char** argv)
{
    const bool wide = argc > 1 && !strcmp(argv[1], "--long");
    unsigned seed = 20260u;
    if (argc > 2) seed = (unsigned)strtoul(argv[2], nullptr, 10);
    Rng r{seed};
    int caseNo = 0;

    run_heads();

    // paths 1 and 3.  Small blocks stay below the vector path's entry (160 input bytes), the middle ones cross it (and 1088 output
    // bytes), the large ones are several 8 KiB segments of the few-block path.
    std::vector<int> shape;
    for (int i = 0; i < (wide ? 40 : 9); ++i) shape.push_back(r.range(1, 6));
    for (int i = 0; i < (wide ? 40 : 9); ++i) shape.push_back(r.range(8, 40));
    for (int i = 0; i < (wide ? 6 : 2); ++i) shape.push_back(r.range(450, 700));
    for (int nseq : shape) {
        const Block b = make_block(r, nseq);
        const int p = (int)b.plain.size();
        const std::vector<int> caps = capacities(p);
        const bool large = b.comp.size() > 16384;
        bool whole = true;
        for (const Variant& v : variants(r, b, wide)) {
            for (size_t k = 0; k < caps.size(); ++k) {
                // (a large block's damaged copies: p, p + 1, p + 8 and every margin below p; not p + 1088 and 0, which only the whole one takes)
                if (large && !whole && !wide && (caps[k] == p + 1088 || caps[k] == 0)) continue;
                plz4_emu_descending = caseNo & 1;
                run_wave(v.bytes, v.n, caps[k], nullptr, 0, caseNo);
                run_dx(v.bytes, v.n, caps[k], caseNo);
                ++caseNo;
            }
            whole = false;
        }
        {   // the valid block comes out whole where there is room
            Exact d((size_t)p);
            if (orc_decompress_safe(b.comp.data(), (int)b.comp.size(), d.p, p) != p || memcmp(d.p, b.plain.data(), (size_t)p)) wrong("the generator", caseNo, (int)b.comp.size(), p, 0, p);
        }
    }

    // path 2: dictionaries of exactly dictLen bytes (65536: the one length at which the offset needs no check)
    const int dictLens[] = {1, 7, 5000, 65535, 65536};
    for (int dictLen : dictLens) {
        Exact dict((size_t)dictLen);
        for (int i = 0; i < dictLen; ++i) dict.p[i] = (uint8_t)r.next();
        for (int rep = 0; rep < (wide ? 12 : 3); ++rep) {
            const Block b = make_block(r, rep == 0 ? r.range(1, 5) : r.range(6, 50), dict.p, dictLen);
            const int p = (int)b.plain.size();
            for (const Variant& v : variants(r, b, wide))
                for (int cap : capacities(p)) { plz4_emu_descending = caseNo & 1; run_wave(v.bytes, v.n, cap, dict.p, dictLen, caseNo); ++caseNo; }
            Exact d((size_t)p);
            if (orc_decompress_safe_dict(b.comp.data(), (int)b.comp.size(), d.p, p, dict.p, dictLen) != p || memcmp(d.p, b.plain.data(), (size_t)p)) wrong("the generator (dictionary)", caseNo, (int)b.comp.size(), p, 0, p);
        }
        if (dictLen < 65535) {
            // the first offset one byte past the dictionary: L literals, offset L + dictLen + 1; rejected
            for (int L : {0, 3, 20}) {
                std::vector<uint8_t> c;
                c.push_back((uint8_t)((L < 15 ? L : 15) << 4)); if (L >= 15) put_len(c, L - 15);
                for (int i = 0; i < L; ++i) c.push_back((uint8_t)r.next());
                const int off = L + dictLen + 1;
                c.push_back((uint8_t)(off & 0xFF)); c.push_back((uint8_t)(off >> 8));
                c.push_back(0xC0); for (int i = 0; i < 12; ++i) c.push_back((uint8_t)r.next());
                for (int cap : {L + 4 + 12, L + 4 + 12 + 100, L + 4 + 12 + 2000}) {
                    Exact d((size_t)cap);
                    if (orc_decompress_safe_dict(c.data(), (int)c.size(), d.p, cap, dict.p, dictLen) >= 0) wrong("an offset past the dictionary is accepted by the oracle", caseNo, (int)c.size(), cap, 0, -1);
                    run_wave(c, (int)c.size(), cap, dict.p, dictLen, caseNo); ++caseNo;
                }
            }
        }
    }

    // path 4: three linked blocks behind a seeded window, and three independent blocks against a dictionary; whole, and with one
    // block of the call damaged
    for (int linked = 0; linked < 2; ++linked) for (int histLen : {0, 7, 5000, 65536}) {
        if (!linked && histLen == 0) continue;
        Exact hist((size_t)histLen);
        for (int i = 0; i < histLen; ++i) hist.p[i] = (uint8_t)r.next();
        for (int rep = 0; rep < (wide ? 8 : 3); ++rep) {
            std::vector<Block> blocks; std::vector<uint8_t> w(hist.p, hist.p + histLen);
            for (int b = 0; b < 3; ++b) {
                const uint8_t* const h = linked ? w.data() : hist.p; const int hl = linked ? (int)w.size() : histLen;
                blocks.push_back(make_block(r, (rep == 0 && b == 1) ? r.range(450, 600) : r.range(4, 60), hl ? h : nullptr, hl));
                if (linked) { w.insert(w.end(), blocks[b].plain.begin(), blocks[b].plain.end()); if (w.size() > 65536) w.erase(w.begin(), w.end() - 65536); }
            }
            for (int dmg = -1; dmg < 3 * (wide ? 12 : 4); ++dmg) {
                std::vector<std::vector<uint8_t>> recs; std::vector<int> caps;
                for (int b = 0; b < 3; ++b) { recs.push_back(blocks[b].comp); caps.push_back((int)blocks[b].plain.size() + (dmg % 2 ? 8 : 0)); }
                if (dmg >= 0) {
                    std::vector<uint8_t>& x = recs[(size_t)(dmg % 3)];
                    switch ((dmg / 3) % 4) {
                    case 0: x[(size_t)r.below((int)x.size())] ^= (uint8_t)(1u << r.below(8)); break;
                    case 1: x.resize(x.size() - (size_t)r.range(1, x.size() < 200 ? (int)x.size() : 200)); break;
                    case 2: { const Block& bb = blocks[(size_t)(dmg % 3)]; const int at = bb.offAt[(size_t)r.below((int)bb.offAt.size())]; x[(size_t)at] = 0; x[(size_t)at + 1] = 0; break; }
                    default: caps[(size_t)(dmg % 3)] -= r.range(1, 13); break;
                    }
                }
                plz4_emu_descending = caseNo & 1;
                run_dxl(recs, caps, linked != 0, hist.p, histLen, caseNo); ++caseNo;
            }
            for (int lie = 0; lie < 3; ++lie) {                              // a record the frame reader turns away, at each place in the call
                std::vector<std::vector<uint8_t>> recs; std::vector<int> caps;
                for (int b = 0; b < 3; ++b) { recs.push_back(blocks[b].comp); caps.push_back((int)blocks[b].plain.size() + (lie == 1 ? 8 : 0)); }
                plz4_emu_descending = caseNo & 1;
                run_dxl(recs, caps, linked != 0, hist.p, histLen, caseNo, lie); ++caseNo;
            }
        }
    }

    printf("decode bounds: %ld one-wave decodes, %ld under a dictionary, %ld few-block runs (%ld answered), %ld calls with history (%ld blocks answered), "
           "%ld record heads: the oracle's answers, no access outside a buffer\n", nWave, nDict, nDx, nDxTaken, nDxl, nDxlTaken, nHead);
    return 0;
}
