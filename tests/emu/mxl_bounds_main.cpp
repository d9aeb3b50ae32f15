// The rounds of the few-block level-2 parse behind an external segment (MxlFlavour) with every workspace array an allocation of
// exactly the planned size (piece_rounds.h), as a program of its own for the address and undefined-behaviour sanitizers
// (tests/test_mxl_bounds.py).  The plaintext is one allocation of exactly segment + block (the walk documents no slack behind a
// block), the block's record array one of exactly the staged call's size; the block's records must be the unbroken
// hc_mid_parse<true>'s.  One line per segment length; a wrong answer exits non-zero, a bad access ends the program with the
// sanitizer's report.  Inputs are generated here: text-like data, zeros, random bytes, a mix, and a block that starts with a copy of
// its segment's tail.
// Host code only, test infrastructure only.
#define PLZ4_EMU 1
#include "piece_rounds.h"
#include <stdio.h>

int plz4_emu_descending = 0;

using namespace plz4;

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 16); }

// words out of a small vocabulary (matches every dozen bytes), zeros, random bytes, or a quarter each
void fill(uint8_t* b, int n, int kind)
{
    static std::vector<std::vector<uint8_t>> vocab;
    if (vocab.empty()) for (int i = 0; i < 300; ++i) { std::vector<uint8_t> w(2 + rnd() % 11); for (auto& c : w) c = (uint8_t)('a' + rnd() % 26); w.push_back(' '); vocab.push_back(w); }
    for (int at = 0; at < n; ) {
        const int k = kind == 3 ? (at * 4 / (n > 0 ? n : 1)) % 3 : kind;
        if (k == 0) { const auto& w = vocab[rnd() % vocab.size()]; for (size_t i = 0; i < w.size() && at < n; ++i) b[at++] = w[i]; }
        else if (k == 1) b[at++] = 0;
        else b[at++] = (uint8_t)rnd();
    }
}

// kind 4: text whose block starts with a copy of the segment's tail (matches into the segment in the first pieces)
int one(int segLen, int n, int kind, int pb, int warm, int order, int maxLen)
{
    const size_t total = (size_t)segLen + (size_t)n;
    uint8_t* const buf = (uint8_t*)malloc(total ? total : 1);
    fill(buf, segLen + n, kind == 4 ? 0 : kind);
    if (kind == 4) { const int c = segLen < n ? segLen : n; if (c > 0) memcpy(buf + segLen, buf + segLen - c + c / 16, (size_t)(c - c / 16)); }
    const uint8_t* const blk = buf + segLen;
    const size_t room = (size_t)seq_capacity(n) + 1;
    uint64_t* whole = (uint64_t*)malloc((room + 64) * 8);
    uint32_t* tabs = (uint32_t*)malloc(kMxTab * 4);
    int la = 0;
    const int nw = hc_mid_parse<true>(blk, n, tabs, tabs + 16384, whole, &la, segLen);
    int bad = 0;
    {
        PieceEmuBlock<MxlFlavour> B(n, pb, maxLen);
        uint64_t* seq = (uint64_t*)malloc(room * 8);
        B.run(MxlFlavour(segLen), blk, warm, order);
        SeqInfo info; info.nseq = -1; info.lastAnchor = 0;
        int chained = 0;
        if (!B.gather(seq, (int)room - 1, &info, order, &chained)) bad = 1;
        else if (info.nseq != nw || info.lastAnchor != la || memcmp(seq, whole, (size_t)nw * 8) != 0) bad = 2;
        free(seq);
    }
    if (bad) printf("WRONG (%d): segment %d n %d kind %d piece %d warm %d order %d\n", bad, segLen, n, kind, pb, warm, order);
    free(whole); free(tabs); free(buf);
    return bad;
}

}  // namespace

int main()
{
    int wrong = 0;
    const int pb = 4096;
    const int segs[] = {0, 3, 7, 8, 9, 100, 4096, 65535, 65536};
    const int lens[] = {0, 12, 13, pb, pb + 1, 5 * pb + 7, 40001};
    for (int segLen : segs) {
        int bad = 0, cases = 0;
        for (int kind = 0; kind < 5; ++kind)
            for (int n : lens)
                for (int warm : {0, 2 * pb})
                    for (int order = 0; order < 2; ++order) {
                        if ((kind == 1 || kind == 2) && (warm || order)) continue;          // (zeros and random bytes: one pass each)
                        bad += one(segLen, n, kind, pb, warm, order, -1) != 0; ++cases;
                    }
        // a short block in a call sized for a longer one; lanes in descending order; one larger block at 16 KiB pieces
        bad += one(segLen, 100, 0, pb, pb, 0, 70001) != 0; ++cases;
        plz4_emu_descending = 1;
        bad += one(segLen, 70001, 4, pb, 0, 1, -1) != 0; ++cases;
        plz4_emu_descending = 0;
        bad += one(segLen, 150007, 4, 16384, 16384, 0, -1) != 0; ++cases;
        printf("segment %d: %d cases, %d wrong%s\n", segLen, cases, bad, bad ? "" : ": no access outside a buffer, every block the unbroken walk's");
        wrong += bad;
    }
    return wrong ? 1 : 0;
}
