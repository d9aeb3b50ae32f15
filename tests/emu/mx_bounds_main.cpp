// The rounds of the few-block level-2 path with every workspace array an allocation of exactly the planned size (mx_rounds.h), as a
// program of its own for the address and undefined-behaviour sanitizers (tests/test_mx_bounds.py).  The block's records must be the
// unbroken hc_mid_parse's; a wrong answer exits non-zero, a bad access ends the program with the sanitizer's report.  Inputs are
// generated here: text-like data, zeros, random bytes, a mix; lengths around the pieces and around kMinLength.  The input and the block's
// record array are allocations of exactly their size as well.
// Host code only, test infrastructure only.
#define PLZ4_EMU 1
#include "mx_rounds.h"
#include <stdio.h>

int plz4_emu_descending = 0;

using namespace plz4;

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 16); }

// words out of a small vocabulary (matches every dozen bytes), zeros, random bytes, or a quarter each
void fill(std::vector<uint8_t>& b, int n, int kind)
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

int one(int n, int kind, int pb, int warm, int order, int maxLen)
{
    std::vector<uint8_t> src((size_t)n, 0);
    fill(src, n, kind);
    const size_t room = (size_t)seq_capacity(n) + 1;                        // the staged call's record array of one block
    uint64_t* whole = (uint64_t*)malloc((room + 64) * 8);
    uint64_t* seq = (uint64_t*)malloc(room * 8);
    uint32_t* tabs = (uint32_t*)malloc(kMxTab * 4);
    int la = 0;
    const int nw = hc_mid_parse(src.data(), n, tabs, tabs + 16384, whole, &la);
    int bad = 0;
    {
        MxEmuBlock B(n, pb, maxLen);
        B.run(src.data(), warm, order);
        SeqInfo info; info.nseq = -1; info.lastAnchor = 0;
        int chained = 0;
        if (!B.gather(seq, (int)room - 1, &info, order, &chained)) bad = 1;
        else if (info.nseq != nw || info.lastAnchor != la || memcmp(seq, whole, (size_t)nw * 8) != 0) bad = 2;
    }
    if (bad) printf("WRONG (%d): n %d kind %d piece %d warm %d order %d\n", bad, n, kind, pb, warm, order);
    free(whole); free(seq); free(tabs);
    return bad;
}

}  // namespace

int main()
{
    int bad = 0, cases = 0;
    const int pb = 4096;
    const int lens[] = {0, 1, 12, 13, 14, pb - 1, pb, pb + 1, 6 * pb, 5 * pb + 7, 5 * pb + 12, 70001};
    for (int kind = 0; kind < 4; ++kind)
        for (int n : lens)
            for (int warm : {0, pb, 3 * pb})
                for (int order = 0; order < 2; ++order) { bad += one(n, kind, pb, warm, order, -1) != 0; ++cases; }
    // a short block in a call sized for a longer one; lanes in descending order; one larger block at 16 KiB pieces
    bad += one(100, 0, pb, pb, 0, 70001) != 0; ++cases;
    plz4_emu_descending = 1;
    bad += one(70001, 3, pb, 0, 1, -1) != 0; ++cases;
    plz4_emu_descending = 0;
    bad += one(300007, 3, 16384, 32768, 0, -1) != 0; ++cases;
    printf("%d cases, %d wrong\n", cases, bad);
    if (!bad) printf("no access outside a buffer, every block the unbroken walk's\n");
    return bad ? 1 : 0;
}
