// The few-block decoder's big path (raw blocks above 4 MiB + 8; dxb_* in plz4_amd/csrc/lz4_dx_device.inl) on hostile input reads
// no byte outside [src, src + n) and writes none outside [dst, dst + cap), and every workspace access stays inside what
// launch_decode reserves: a program of its own for the address and undefined-behaviour sanitizers (never loaded into Python, never
// run on a GPU).  The stage train is tests/emu/dx_train.h: tables, pointers, units, the groups' composed rows and entries and
// the run list are heap allocations of exactly the reserved size, source and destination of exactly n and cap bytes.  What the
// train answers is checked against the oracle (oracle/plz4_oracle.c), and the run list never holds more than its reserved count.
// Inputs: blocks of 5-6 MiB built sequence by sequence around the vector path's boundaries (the generator of
// decode_bounds_main.cpp / tests/lz4blocks.py) with literal runs and matches of up to several hundred KiB between them, then
// truncated, bit-flipped, 0xFF-ed and with zeroed offsets, over the reference's end-of-output margins as capacities, at group
// sizes 2, 4 and the default and run thresholds of 4 KiB and the default.
// Prints one line of counts; exit status 1 on a wrong answer, the sanitizer's on a bad access.
#define PLZ4_EMU 1
#include "dx_train.h"
#include "../../oracle/plz4_oracle.h"
#include <stdio.h>
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

const int kLL[] = {0, 0, 1, 2, 3, 5, 7, 12, 13, 14, 15, 16, 17, 30, 45, 47, 48, 49, 62, 63, 64, 100, 254 + 15, 255 + 15, 300, 600};
const int kML[] = {4, 4, 5, 6, 8, 12, 17, 18, 19, 20, 33, 64, 100, 272, 273, 274, 275, 528, 529, 1000};

struct Block { std::vector<uint8_t> comp, plain; };

void put_len(std::vector<uint8_t>& out, int v) { while (v >= 255) { out.push_back(255); v -= 255; } out.push_back((uint8_t)v); }

void put_seq(Rng& r, Block& b, int ll, int ml, int off)
{
    b.comp.push_back((uint8_t)(((ll < 15 ? ll : 15) << 4) | (ml - 4 < 15 ? ml - 4 : 15)));
    if (ll >= 15) put_len(b.comp, ll - 15);
    for (int i = 0; i < ll; ++i) { const uint8_t v = (uint8_t)r.next(); b.comp.push_back(v); b.plain.push_back(v); }
    b.comp.push_back((uint8_t)(off & 0xFF)); b.comp.push_back((uint8_t)(off >> 8));
    if (ml - 4 >= 15) put_len(b.comp, ml - 4 - 15);
    const size_t start = b.plain.size() - (size_t)off;
    for (int i = 0; i < ml; ++i) b.plain.push_back(b.plain[start + (size_t)i]);
}

// a valid block of about `target` plaintext bytes; endsLong: the last sequence in front of the closing literals is a long one
Block make_block(Rng& r, int target, bool endsLong)
{
    Block b;
    for (;;) {
        for (int s = 0; s < 200; ++s) {
            int ll = r.unit() < 0.7 ? kLL[r.below(26)] : r.range(0, 40);
            const int ml = r.unit() < 0.6 ? kML[r.below(20)] : r.range(4, 40);
            if (b.plain.empty() && ll == 0) ll = 1;
            const int have = (int)b.plain.size() + ll;
            const double kind = r.unit();
            const int reach = kind < 0.25 ? 8 : (kind < 0.55 ? 64 : (kind < 0.8 ? 2000 : 65535));
            put_seq(r, b, ll, ml, r.range(1, (have < reach ? have : reach) + 1));
        }
        if ((int)b.plain.size() >= target && !endsLong) break;
        const double k = r.unit();
        const int offs[] = {1, 2, 7, 4000, 65535};
        if (k < 0.4) put_seq(r, b, r.range(60000, 400000), 8, 3);
        else if (k < 0.8) put_seq(r, b, 2, r.range(60000, 700000), offs[r.below(5)]);
        else put_seq(r, b, 65536 + 15, 65536, 1);
        if ((int)b.plain.size() >= target) break;
    }
    const int tail = r.range(12, 40);
    b.comp.push_back((uint8_t)((tail < 15 ? tail : 15) << 4));
    if (tail >= 15) put_len(b.comp, tail - 15);
    for (int i = 0; i < tail; ++i) { const uint8_t v = (uint8_t)r.next(); b.comp.push_back(v); b.plain.push_back(v); }
    return b;
}

long nRun = 0, nTaken = 0, nRuns = 0;

[[noreturn]] void wrong(const char* what, int caseNo, int n, int cap, int got, int want)
{
    fprintf(stderr, "WRONG ANSWER: %s, case %d: n %d cap %d: %d, the oracle says %d\n", what, caseNo, n, cap, got, want);
    exit(1);
}

// one block of a call whose strides are maxIn / maxOut
void run(const std::vector<uint8_t>& comp, int n, int cap, int64_t maxIn, int64_t maxOut, int G, int thr, int caseNo)
{
    DxEmuHeap<uint8_t> src((size_t)n), dst((size_t)cap), ref((size_t)cap);
    if (n) memcpy(src.p, comp.data(), (size_t)n);
    DxbEmuStats st;
    const int r = dxb_emu_block(src.p, n, dst.p, cap, maxIn, maxOut, G, thr, &st);
    ++nRun;
    if (memcmp(src.p, comp.data(), (size_t)n)) wrong("source changed", caseNo, n, cap, r, 0);
    if (r == kDxEmuUnitsDisagree) wrong("units do not meet", caseNo, n, cap, r, 0);
    if (r == kDxEmuListOverrun || st.runs > st.room) wrong("run list beyond its reserved count", caseNo, n, cap, st.runs, st.room);
    if (r == kDxEmuLeft) return;
    const int want = orc_decompress_safe(src.p, n, ref.p, cap);
    if (r != want) wrong("dx big", caseNo, n, cap, r, want);
    if (want > 0 && memcmp(dst.p, ref.p, (size_t)want)) wrong("dx big: bytes", caseNo, n, cap, r, want);
    ++nTaken; nRuns += st.runs;
}

}  // namespace

int main()
{
    Rng r{20260412u};
    int caseNo = 0;
    const int kG[] = {0, 2, 4}, kThr[] = {0, 4096};
    for (int blk = 0; blk < 2; ++blk) {
        const Block b = make_block(r, (5 << 20) + r.below(1 << 19), blk == 1);
        const int n = (int)b.comp.size(), p = (int)b.plain.size();
        if (p < (5 << 20) || p > (6 << 20) + (3 << 19)) { fprintf(stderr, "generator: %d plaintext bytes\n", p); return 2; }
        const int64_t maxIn = n + 1000, maxOut = p + 8;
        // the block as it is, over the end-of-output margins; as the smaller block of a call with larger strides; with too little room
        const int caps[] = {p + 8, p, p - 1, p - 5, p - 12, p - 64, p / 2};
        for (int k = 0; k < 7; ++k, ++caseNo) run(b.comp, n, caps[k], maxIn, maxOut, kG[k % 3], kThr[k % 2], caseNo);
        run(b.comp, n, p + 8, 3 * (int64_t)n, 2 * (int64_t)p, 0, 0, caseNo++);
        run(b.comp, n, p + 8, n / 2, p + 8, 0, 0, caseNo++);                         // (longer than the call's tables: left)
        run(b.comp, n, p + 8, maxIn, p / 2, 2, 0, caseNo++);                         // (a capacity above the call's pointers: left)
        // damaged copies
        const int at[] = {n / 7, n / 2, n - 70000, n - 20};
        for (int k = 0; k < 16; ++k, ++caseNo) {
            std::vector<uint8_t> d = b.comp;
            const int i = at[k / 4] + r.below(64) < n - 2 ? at[k / 4] + r.below(64) : n - 3;
            switch (k % 4) {
            case 0: d[(size_t)i] ^= (uint8_t)(1u << r.below(8)); break;
            case 1: d[(size_t)i] = 0xFF; break;
            case 2: d[(size_t)i] = 0; d[(size_t)i + 1] = 0; break;
            default: d.resize((size_t)i); break;
            }
            run(d, (int)d.size(), k % 3 == 2 ? p : p + 8, maxIn, maxOut, kG[k % 3], kThr[(k / 2) % 2], caseNo);
        }
        // a run of 0xFF laid over the length bytes of the first long sequence: a length that has no end inside the block
        {
            std::vector<uint8_t> d = b.comp;
            size_t i = 0; while (i + 300 < d.size() && !(d[i] == 255 && d[i + 1] == 255 && d[i + 40] == 255)) ++i;
            for (size_t k = i; k < d.size(); ++k) d[k] = 0xFF;
            run(d, (int)d.size(), p + 8, maxIn, maxOut, 2, 4096, caseNo++);
        }
    }
    if (nTaken < 10 || nRuns < 10) { fprintf(stderr, "too little was answered: %ld of %ld, %ld runs\n", nTaken, nRun, nRuns); return 1; }
    printf("dx big path: %ld trains, %ld answered, %ld listed runs: no access outside a buffer, every answer the oracle's\n", nRun, nTaken, nRuns);
    return 0;
}
