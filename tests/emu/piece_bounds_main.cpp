// The rounds of the few-block parses with every workspace array an allocation of exactly the planned size (piece_rounds.h), as a
// program of its own for the address and undefined-behaviour sanitizers (tests/test_piece_bounds.py), one flavour after the other:
//   level 2            the block's records must be the unbroken hc_mid_parse's;
//   level 1            ... one unbroken wave_parse_l1's (a block below kFxMinLen is not the path's: the kernel's rule, that very parse);
//   level 1, linked    ... l1x_block's one exact run, behind a 64 KiB segment under kDictLoad and with none under kDictFreshPrefix.
// A wrong answer exits non-zero, a bad access ends the program with the sanitizer's report.  Inputs are generated here: text-like
// data, zeros, random bytes, a mix; lengths around the pieces, around kMinLength and around kFxMinLen.  The input and the block's
// record array are allocations of exactly their size as well.
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

uint32_t lds[kHashBytes / 4];

// the rounds and the gather of one block against the unbroken parse's records (whole, nw, la).  0: the same
template <class F> int rounds_match(PieceEmuBlock<F>& B, const F& f, const uint8_t* src, int warm, int order, const uint64_t* whole, int nw, int la)
{
    const size_t room = (size_t)seq_capacity(B.n) + 1;                      // the staged call's record array of one block
    uint64_t* seq = (uint64_t*)malloc(room * 8);
    B.run(f, src, warm, order);
    SeqInfo info; info.nseq = -1; info.lastAnchor = 0;
    int chained = 0, bad = 0;
    if (!B.gather(seq, (int)room - 1, &info, order, &chained)) bad = 1;
    else if (info.nseq != nw || info.lastAnchor != la || memcmp(seq, whole, (size_t)nw * 8) != 0) bad = 2;
    free(seq);
    return bad;
}

int one_mx(int n, int kind, int pb, int warm, int order, int maxLen)
{
    std::vector<uint8_t> src((size_t)n, 0);
    fill(src.data(), n, kind);
    uint64_t* whole = (uint64_t*)malloc(((size_t)seq_capacity(n) + 1 + 64) * 8);
    uint32_t* tabs = (uint32_t*)malloc(kMxTab * 4);
    int la = 0;
    const int nw = hc_mid_parse(src.data(), n, tabs, tabs + 16384, whole, &la);
    int bad;
    {
        PieceEmuBlock<MxFlavour> B(n, pb, maxLen);
        bad = rounds_match(B, MxFlavour{}, src.data(), warm, order, whole, nw, la);
    }
    if (bad) printf("WRONG level 2 (%d): n %d kind %d piece %d warm %d order %d\n", bad, n, kind, pb, warm, order);
    free(whole); free(tabs);
    return bad;
}

int one_fx(int n, int kind, int pb, int warm, int order)
{
    std::vector<uint8_t> src((size_t)n, 0);
    fill(src.data(), n, kind);
    uint64_t* whole = (uint64_t*)malloc(((size_t)seq_capacity(n) + 1) * 8);
    int la = 0;
    const int nw = wave_parse_l1<2>(src.data(), n, lds, whole, &la);
    int bad = -1;                                                           // -1: below kFxMinLen, k_piece's out-of-scope rule -- the parse above
    if (n >= kFxMinLen) {
        PieceEmuBlock<FxFlavour<false>> B(n, pb);
        bad = rounds_match(B, FxFlavour<false>{lds, 0}, src.data(), warm, order, whole, nw, la);
    }
    if (bad > 0) printf("WRONG level 1 (%d): n %d kind %d piece %d warm %d order %d\n", bad, n, kind, pb, warm, order);
    free(whole);
    return bad;
}

// mode: kDictLoad behind a 64 KiB segment, kDictFreshPrefix without one.  Two copies of segment room + block: the rounds' and the exact run's.
int one_fxl(int n, int kind, int mode, int pb, int warm, int order)
{
    const int segLen = mode == kDictLoad ? 65536 : 0;
    std::vector<uint8_t> seg((size_t)segLen, 0);
    fill(seg.data(), segLen, kind);
    uint8_t* bufA = (uint8_t*)malloc((size_t)65536 + n);
    uint8_t* bufB = (uint8_t*)malloc((size_t)65536 + n);
    memset(bufA, 0xA7, 65536); memset(bufB, 0xA7, 65536);
    fill(bufA + 65536, n, kind);
    if (n) memcpy(bufB + 65536, bufA + 65536, (size_t)n);
    const size_t room = (size_t)seq_capacity(n) + 1;
    uint64_t* whole = (uint64_t*)malloc(room * 8);
    int la = 0;
    FxlBlk xw;
    const int nw = l1x_block(bufB + 65536, n, mode, seg.data(), segLen, nullptr, whole, (int)room - 1, &la, &xw, lds);
    int bad = nw < 0 ? 3 : 0;
    if (!bad) {
        PieceEmuBlock<FxFlavour<true>> B(n, pb, -1, true);
        const FxlBlk xb = *B.xb = fxl_prep(bufA + 65536, n, mode, seg.data(), segLen, nullptr, B.tabIn, lds);   // k_fxl_prep
        if (xb.pfx != xw.pfx || xb.bs != xw.bs || xb.pfx < 0) bad = 4;
        else bad = rounds_match(B, FxFlavour<true>{lds, xb.bs}, bufA + 65536, warm, order, whole, nw, la);
    }
    if (bad) printf("WRONG level 1 linked (%d): n %d kind %d mode %d piece %d warm %d order %d\n", bad, n, kind, mode, pb, warm, order);
    free(bufA); free(bufB); free(whole);
    return bad;
}

}  // namespace

int main()
{
    int wrong = 0;
    const int pb = 4096;
    {   // level 2
        int bad = 0, cases = 0;
        const int lens[] = {0, 1, 12, 13, 14, pb - 1, pb, pb + 1, 6 * pb, 5 * pb + 7, 5 * pb + 12, 70001};
        for (int kind = 0; kind < 4; ++kind)
            for (int n : lens)
                for (int warm : {0, pb, 3 * pb})
                    for (int order = 0; order < 2; ++order) { bad += one_mx(n, kind, pb, warm, order, -1) != 0; ++cases; }
        // a short block in a call sized for a longer one; lanes in descending order; one larger block at 16 KiB pieces
        bad += one_mx(100, 0, pb, pb, 0, 70001) != 0; ++cases;
        plz4_emu_descending = 1;
        bad += one_mx(70001, 3, pb, 0, 1, -1) != 0; ++cases;
        plz4_emu_descending = 0;
        bad += one_mx(300007, 3, 16384, 32768, 0, -1) != 0; ++cases;
        printf("level 2: %d cases, %d wrong\n", cases, bad);
        if (!bad) printf("level 2: no access outside a buffer, every block the unbroken parse's\n");
        wrong += bad;
    }
    {   // level 1, independent blocks: around kFxMinLen, more than one piece, a last piece of 7 bytes
        int bad = 0, cases = 0, outside = 0;
        const int lens[] = {65536, 65537, kFxMinLen, kFxMinLen + 1, 70001, 65536 + 6 * pb + 7};
        for (int kind = 0; kind < 4; ++kind)
            for (int n : lens)
                for (int warm : {0, pb, 3 * pb})
                    for (int order = 0; order < 2; ++order) {
                        const int r = one_fx(n, kind, pb, warm, order);
                        if (r < 0) ++outside; else { bad += r != 0; ++cases; }
                    }
        printf("level 1: %d cases, %d wrong (%d more below kFxMinLen: not the path's, parsed whole, compared with nothing)\n", cases, bad, outside);
        if (!bad) printf("level 1: no access outside a buffer, every block the unbroken parse's\n");
        wrong += bad;
    }
    {   // level 1, history outside the block: below kMinLength, a piece-0-only block, more than one piece
        int bad = 0, cases = 0;
        const int lens[] = {0, 12, 13, pb, pb + 1, 70001};
        for (int kind = 0; kind < 4; ++kind)
            for (int n : lens)
                for (int mode : {(int)kDictLoad, (int)kDictFreshPrefix})
                    for (int warm : {0, pb, 3 * pb})
                        for (int order = 0; order < 2; ++order) { bad += one_fxl(n, kind, mode, pb, warm, order) != 0; ++cases; }
        printf("level 1 linked: %d cases, %d wrong\n", cases, bad);
        if (!bad) printf("level 1 linked: no access outside a buffer, every block the unbroken parse's\n");
        wrong += bad;
    }
    return wrong ? 1 : 0;
}
