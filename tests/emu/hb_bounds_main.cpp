// The builder that cuts a block's chain and lists into pieces (plz4_amd/csrc/lz4hc_lists_device.inl) with every array an allocation
// of exactly the size the kernels' layouts give (hb_staged.h: chain nPad x 2, rank nPad x 4, list (nPad + 8) x 4, offsets 32768 x 4,
// counts and slots HbLayout's total, the two LDS tables 64 KiB each) and a source of exactly n bytes, as a program of its own for the
// address and undefined-behaviour sanitizers (tests/test_hb_bounds.py).  Lengths around the pieces, the positions that are never
// inserted around them, both lane orders, pieces of 256 and 1024 positions.  A wrong array exits non-zero, a bad access ends the
// program with the sanitizer's report.  Host code only, test infrastructure only.
#define PLZ4_EMU 1
#include "hb_staged.h"
#include <stdio.h>

int plz4_emu_descending = 0;

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 16); }

// words out of a small vocabulary, zeros, random bytes, or a third each
void fill(uint8_t* b, int n, int kind)
{
    static std::vector<std::vector<uint8_t>> vocab;
    if (vocab.empty()) for (int i = 0; i < 300; ++i) { std::vector<uint8_t> w(2 + rnd() % 11); for (auto& c : w) c = (uint8_t)('a' + rnd() % 26); w.push_back(' '); vocab.push_back(w); }
    for (int at = 0; at < n; ) {
        const int k = kind == 3 ? (int)((int64_t)at * 3 / (n > 0 ? n : 1)) % 3 : kind;
        if (k == 0) { const auto& w = vocab[rnd() % vocab.size()]; for (size_t i = 0; i < w.size() && at < n; ++i) b[at++] = w[i]; }
        else if (k == 1) b[at++] = 0;
        else b[at++] = (uint8_t)rnd();
    }
}

}  // namespace

int main()
{
    long runs = 0;
    for (int desc = 0; desc < 2; ++desc) {
        plz4_emu_descending = desc;
        for (int piece : {256, 1024}) {
            const int lengths[] = {0, 1, 3, 4, 5, 63, 64, 65, piece - 1, piece, piece + 1, piece + 3, piece + 4, 3 * piece + 17, 200 * 1024 + 13};
            const int segs[] = {0, 2, 3, 4, piece - 1, piece + 2, 65536};
            for (int n : lengths) {
                for (int kind = 0; kind < 4; ++kind) {
                    if (n > 4096 * 4 && (kind != 3 || (desc && piece == 256))) continue;   // (the long one: the mix)
                    std::vector<uint8_t> b((size_t)n + 1);
                    fill(b.data(), n, kind);
                    const int r = hbt::compare(b.data(), n, piece, 0, 0);
                    if (r) { printf("FAIL: length %d kind %d piece %d lanes %d: %d\n", n, kind, piece, desc, r); return 1; }
                    ++runs;
                }
            }
            for (int seg : segs) {
                for (int n : lengths) {
                    if (n > 4096 * 4) continue;
                    if (seg > piece + 2 && n != 5 && n != 65 && n != piece + 1 && n != 3 * piece + 17) continue;   // (the long segment: four lengths)
                    std::vector<uint8_t> b((size_t)seg + n + 1);
                    fill(b.data(), seg + n, 3);
                    const int r = hbt::compare(b.data(), seg + n, piece, seg > 3 ? seg - 3 : 0, seg);
                    if (r) { printf("FAIL: segment %d length %d piece %d lanes %d: %d\n", seg, n, piece, desc, r); return 1; }
                    ++runs;
                }
            }
        }
    }
    printf("lists in pieces: no access outside a buffer, every array hc12_build_lists's and the definition's (%ld inputs)\n", runs);
    return 0;
}
