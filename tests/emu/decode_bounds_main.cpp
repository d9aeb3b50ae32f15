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
//   6  the three flavours of the train on a call of two raw blocks laid out for the smaller one: the other on each side of every
//      term of the misfit rule (a row of T, a row of pointers, the units)
//   7  the three flavours on blocks of three and four segments with a unit that flags its block: the other units still run
// Paths 3, 4, 6 and 7 run the stage bodies the kernels run, over the kernels' grids (tests/emu/dx_train.h).
// Inputs: blocks built sequence by sequence around the vector path's boundaries (tests/lz4blocks.py is the same generator), then
// truncated, bit-flipped, 0xFF-ed and with zeroed offsets, over the reference's end-of-output margins as capacities.
// `--long`: a wider set (minutes).  Prints one line of counts; exit status 1 on a wrong answer, the sanitizer's on a bad access.
#define PLZ4_EMU 1
#include "dx_train.h"
#include "../../oracle/plz4_oracle.h"
#include <stdio.h>

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
    Exact dst((size_t)cap), d3((size_t)cap);
    DxEmuTrain t;
    const uint8_t* const sp = src.p; const int32_t len = n, room = cap;
    dx_emu_train(DxF{}, t, DxEmuCall{1, &sp, &len, &room, dst.p, 0}, n > 0 ? n : 1, cap > 0 ? cap : 1);
    if (t.disagree) wrong("dx: units do not meet", caseNo, n, cap, 0, 0);
    ++nDx;
    if (t.info[0].bad) return;
    const int outLen = t.info[0].outLen;
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
    const int64_t dstStride = maxCap;
    Exact dst((size_t)nb * dstStride), win(131072), winRef(65536);
    Exact dictCopy(linked ? 0 : (size_t)histLen);
    std::vector<int32_t> len(nb), first(nb, 0), chain(nb, 0), room(caps.begin(), caps.end());
    std::vector<const uint8_t*> src(nb);
    int winLen = linked ? histLen : 0;
    memset(dst.p, kFill, (size_t)nb * (size_t)dstStride);
    if (linked) { if (histLen) memcpy(win.p, hist, (size_t)histLen); }
    else { if (histLen) memcpy(dictCopy.p, hist, (size_t)histLen); for (int i = 0; i < nb; ++i) first[i] = i; }
    DxlCall c{};
    c.first = first.data(); c.chain = chain.data();
    if (linked) { c.hist = win.p; c.histStride = 131072; c.histLen = &winLen; c.histLenAll = 0; }
    else { c.hist = dictCopy.p; c.histStride = 0; c.histLen = nullptr; c.histLenAll = histLen; }
    for (int b = 0; b < nb; ++b) { len[b] = dx_rec_len(body.p + off[b], off[b + 1] - off[b], bsz, false, maxCap); src[b] = body.p + off[b] + 4; }   // k_dx_rec_prep
    DxEmuTrain t;
    DxInfo*& info = t.info;
    dx_emu_train(DxlF{}, t, DxEmuCall{nb, src.data(), len.data(), room.data(), dst.p, dstStride}, c, nb, bsz, maxCap, true, 0,
                 [&] { for (int b = 0; b < nb; ++b) if (linked && dxl_chain_dead(len.data(), 0, b, 0)) info[b].bad = 1; });   // k_dxl_link
    if (t.disagree) wrong("dxl: units do not meet", caseNo, nb, maxCap, 0, 0);
    const int rounds = t.launched;
    std::vector<int32_t> result(nb, 0), status(nb, 0);
    DxlFin f; f.hashBad = nullptr; f.moved = t.moved; f.rounds = rounds; f.result = result.data(); f.status = status.data();
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

// path 6: a call of two raw blocks whose workspace is laid out for maxIn / maxOut, through flavour fl of the train (dx_emu_raw_call:
// DxF, DxbF, DxlF under the dictionary dict).  Block 0 (x) is the one under test, block 1 the sibling that fits.  misfit: x is larger
// than the rows were sized for and must be left; else it must be answered.  The sibling is answered either way, and every answer is
// the oracle's.  Both outputs lie in one allocation at a stride of the larger capacity, source and outputs are exact.
long nMisfit = 0;
void run_pair(const int fl, const Block& x, const int capX, const Block& sib, const int64_t maxIn, const int64_t maxOut, const bool misfit,
              const uint8_t* dict, const int dictLen, const int caseNo)
{
    const Block* const blk[2] = {&x, &sib};
    const int32_t len[2] = {(int32_t)x.comp.size(), (int32_t)sib.comp.size()}, cap[2] = {capX, (int32_t)sib.plain.size()};
    Exact s0((size_t)len[0], srcShift++ & 15), s1((size_t)len[1], srcShift++ & 15);
    memcpy(s0.p, x.comp.data(), (size_t)len[0]); memcpy(s1.p, sib.comp.data(), (size_t)len[1]);
    const uint8_t* const src[2] = {s0.p, s1.p};
    const int64_t dstStride = cap[0] > cap[1] ? cap[0] : cap[1];
    Exact dst((size_t)(dstStride + cap[1]));
    int32_t answer[2] = {0, 0};
    if (dx_emu_raw_call(fl, DxEmuCall{2, src, len, cap, dst.p, dstStride}, maxIn, maxOut, fl == 2 ? dict : nullptr, fl == 2 ? dictLen : 0, 0, answer))
        wrong("pair: units do not meet", caseNo, len[0], capX, fl, 0);
    for (int b = 0; b < 2; ++b) {
        if (b == 0 && misfit) { if (answer[0] != kDxEmuLeft) wrong("pair: a misfit block is answered", caseNo, len[0], capX, answer[0], kDxEmuLeft); continue; }
        Exact ref((size_t)cap[b]);
        const int want = fl == 2 ? orc_decompress_safe_dict(src[b], len[b], ref.p, cap[b], dict, dictLen) : orc_decompress_safe(src[b], len[b], ref.p, cap[b]);
        if (answer[b] != want || want != (int)blk[b]->plain.size()) wrong(b ? "pair: the sibling" : "pair: the fitting block", caseNo, len[b], cap[b], answer[b], want);
        if (memcmp(dst.p + b * dstStride, ref.p, (size_t)want)) wrong("pair: bytes", caseNo, len[b], cap[b], answer[b], want);
    }
    ++nMisfit;
}
// a valid block whose compressed size is at least minComp, and is `mod` modulo 64 (mod < 0: any)
Block block_of(Rng& r, const int minComp, const int mod, const uint8_t* dict = nullptr, const int dictLen = 0)
{
    for (int nseq = minComp / 150 + 1;; ++nseq) {
        Block b = make_block(r, nseq, dict, dictLen);
        if ((int)b.comp.size() >= minComp && (mod < 0 || (int)b.comp.size() % 64 == mod)) return b;
    }
}
// both sides of every term of the misfit rule (dx_misfit, lz4_dx_device.inl), for the three flavours
void run_misfits(Rng& r, int& caseNo)
{
    Exact dict(5000);
    for (int i = 0; i < 5000; ++i) dict.p[i] = (uint8_t)r.next();
    for (int fl = 0; fl < 3; ++fl) {
        const uint8_t* const d = fl == 2 ? dict.p : nullptr; const int dl = fl == 2 ? 5000 : 0;
        const Block sib = block_of(r, 200, -1, d, dl);
        const Block x0 = block_of(r, 1500, 0, d, dl), x1 = block_of(r, 1500, 1, d, dl), x3 = block_of(r, 2 * kDxSeg + 64, -1, d, dl);
        // n == tStride - 64 and n == tStride - 63: a row of T for blocks of up to maxIn bytes has maxIn rounded up to 64, + 64 entries
        const int p0 = (int)x0.plain.size(), p1 = (int)x1.plain.size(), p3 = (int)x3.plain.size();
        if ((int)dx_t_stride((int64_t)x0.comp.size()) - 64 != (int)x0.comp.size() || (int)dx_t_stride((int64_t)x1.comp.size() - 1) - 63 != (int)x1.comp.size()) wrong("pair: the edge of T", caseNo, 0, 0, 0, 0);
        run_pair(fl, x0, p0, sib, (int64_t)x0.comp.size(), p0, false, d, dl, caseNo++);
        run_pair(fl, x1, p1, sib, (int64_t)x1.comp.size() - 1, p1, true, d, dl, caseNo++);
        // cap == pStride - 64 and cap == pStride - 63
        const int64_t P = fl == 1 ? (int64_t)dxb_ptr_stride(p0) : (int64_t)dx_ptr_stride(p0);
        run_pair(fl, x0, (int)P - 64, sib, (int64_t)x0.comp.size(), p0, false, d, dl, caseNo++);
        run_pair(fl, x0, (int)P - 63, sib, (int64_t)x0.comp.size(), p0, true, d, dl, caseNo++);
        // dx_segments(n) == maxSeg and == maxSeg + 1: three segments in a call laid out for three, and for two
        run_pair(fl, x3, p3, sib, (int64_t)x3.comp.size(), p3, false, d, dl, caseNo++);
        run_pair(fl, x3, p3, sib, 2 * kDxSeg, p3, true, d, dl, caseNo++);
    }
}

// path 7: a flagged unit does not stop the others.  Blocks of three and of four segments with an offset zeroed in the middle segment:
// the stitch follows the chain as ever, the unit that meets the offset flags the block, and the driver goes on through every unit
// of the grid as the kernel does (dx_stage_fill) -- the block is left, and no access leaves an allocation.
long nFlagged = 0;
void run_flagged(Rng& r, int& caseNo)
{
    for (int segs = 3; segs <= 4; ++segs) for (int fl = 0; fl < 3; ++fl) {
        Block b = block_of(r, (segs - 1) * kDxSeg + 64, -1);
        if (dx_segments((int)b.comp.size()) != segs) wrong("flagged: the generator", caseNo, (int)b.comp.size(), 0, dx_segments((int)b.comp.size()), segs);
        size_t k = 0;
        while (k < b.offAt.size() && b.offAt[k] < kDxSeg + kDxSeg / 2) ++k;
        if (k >= b.offAt.size() || b.offAt[k] >= 2 * kDxSeg) wrong("flagged: no offset in the middle segment", caseNo, (int)b.comp.size(), 0, 0, 0);
        b.comp[(size_t)b.offAt[k]] = 0; b.comp[(size_t)b.offAt[k] + 1] = 0;
        const int n = (int)b.comp.size(), cap = (int)b.plain.size();
        Exact src((size_t)n, srcShift++ & 15), dst((size_t)cap);
        memcpy(src.p, b.comp.data(), (size_t)n);
        const uint8_t* const sp = src.p; const int32_t len = n, room = cap; int32_t answer = 0;
        if (dx_emu_raw_call(fl, DxEmuCall{1, &sp, &len, &room, dst.p, 0}, n, cap, nullptr, 0, 0, &answer)) wrong("flagged: units do not meet", caseNo, n, cap, fl, 0);
        if (answer != kDxEmuLeft) wrong("flagged: the block is answered", caseNo, n, cap, answer, kDxEmuLeft);
        ++nFlagged; ++caseNo;
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

    plz4_emu_descending = 0;
    run_misfits(r, caseNo);
    run_flagged(r, caseNo);

    printf("decode bounds: %ld one-wave decodes, %ld under a dictionary, %ld few-block runs (%ld answered), %ld calls with history (%ld blocks answered), "
           "%ld record heads, %ld pairs around the misfit rule, %ld blocks with a flagged unit: the oracle's answers, no access outside a buffer\n",
           nWave, nDict, nDx, nDxTaken, nDxl, nDxlTaken, nHead, nMisfit, nFlagged);
    return 0;
}
