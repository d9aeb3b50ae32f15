// wave_finish_record (plz4_amd/csrc/lz4_block_io.inl) touches no byte outside the block and its record: a program of its own for the
// address and undefined-behaviour sanitizers (tests/test_block_io_bounds.py builds and runs it; never loaded into Python, never run on
// a GPU).  The block is a heap allocation of exactly n bytes, the record one of exactly 4 + max(c, n) + (checksum ? 4 : 0) bytes, so a
// load or store past either end is a heap-buffer-overflow.  Every record is checked byte for byte against one put together here from
// the encoder's bytes, the plaintext and a plain xxh32; a wrong byte exits non-zero.
#define PLZ4_EMU 1
#include "../../plz4_amd/csrc/lz4_block_io.inl"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

int plz4_emu_descending = 0;

using namespace plz4;

static uint32_t plain_xxh32(const uint8_t* p, size_t n)
{
    auto rol = [](uint32_t x, int r) { return (x << r) | (x >> (32 - r)); };
    auto rd = [](const uint8_t* q) { return (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24); };
    const uint32_t P1 = 2654435761u, P2 = 2246822519u, P3 = 3266489917u, P4 = 668265263u, P5 = 374761393u;
    const uint8_t* const end = p + n;
    uint32_t h;
    if (n >= 16) {
        uint32_t v[4] = {P1 + P2, P2, 0u, 0u - P1};
        for (; p + 16 <= end; p += 16)
            for (int k = 0; k < 4; ++k) v[k] = rol(v[k] + rd(p + 4 * k) * P2, 13) * P1;
        h = rol(v[0], 1) + rol(v[1], 7) + rol(v[2], 12) + rol(v[3], 18);
    } else {
        h = P5;
    }
    h += (uint32_t)n;
    for (; p + 4 <= end; p += 4) h = rol(h + rd(p) * P3, 17) * P4;
    for (; p < end; ++p) h = rol(h + (uint32_t)*p * P5, 11) * P1;
    h ^= h >> 15; h *= P2; h ^= h >> 13; h *= P3; h ^= h >> 16;
    return h;
}
static void put32(std::vector<uint8_t>& v, uint32_t x) { for (int k = 0; k < 4; ++k) v.push_back((uint8_t)(x >> (8 * k))); }

int main()
{
    static const int kLens[] = {0, 1, 13, 4097, 65536};
    static uint32_t lds[kHashBytes / 4];
    const int bsz = 65536;
    unsigned seed = 12345u;
    long checked = 0, stored = 0;
    for (int desc = 0; desc < 2; ++desc) for (int kind = 0; kind < 3; ++kind) for (int n : kLens) for (int checksum = 0; checksum < 2; ++checksum) {
        plz4_emu_descending = desc;
        // the plaintext (kind 0: text-like, 1: zeros, 2: random -- it does not compress) and the encoder's bytes, in buffers with room to spare
        std::vector<uint8_t> plain((size_t)n + 64, 0), comp((size_t)bsz + 64, 0);
        for (int k = 0; k < n; ++k) {
            seed = seed * 1664525u + 1013904223u;
            plain[k] = kind == 0 ? (uint8_t)("the quick brown fox "[(k + (k >> 9)) % 20]) : kind == 1 ? 0 : (uint8_t)(seed >> 24);
        }
        const int c = wave_encode_block(plain.data(), n, comp.data(), bsz, lds);
        if (c < 0 || c > bsz) { fprintf(stderr, "encoder: %d\n", c); return 1; }
        if (kind == 2 && n == bsz && c != 0) { fprintf(stderr, "random bytes were expected not to fit\n"); return 1; }
        // exact allocations (malloc(0) may be null: then n == 0 and nothing of it is read)
        uint8_t* const s = (uint8_t*)malloc((size_t)n);
        if (n) memcpy(s, plain.data(), (size_t)n);
        const size_t recBytes = 4 + (size_t)(c > n ? c : n) + (checksum ? 4 : 0);
        uint8_t* const rec = (uint8_t*)malloc(recBytes);
        memset(rec, 0xA5, recBytes);
        memcpy(rec + 4, comp.data(), (size_t)c);
        const int len = wave_finish_record(rec, s, n, c, checksum != 0);
        std::vector<uint8_t> want;
        put32(want, c ? (uint32_t)c : (0x80000000u | (uint32_t)n));
        want.insert(want.end(), c ? comp.data() : plain.data(), (c ? comp.data() : plain.data()) + (c ? c : n));
        if (checksum) put32(want, plain_xxh32(want.data() + 4, want.size() - 4));
        if (len != (int)want.size() || (size_t)len > recBytes || memcmp(rec, want.data(), want.size()) != 0) {
            fprintf(stderr, "wrong record: kind %d n %d checksum %d descending %d: encoder %d, length %d, expected %zu\n", kind, n, checksum, desc, c, len, want.size());
            return 1;
        }
        for (size_t k = (size_t)len; k < recBytes; ++k) if (rec[k] != 0xA5) { fprintf(stderr, "byte %zu behind the record written (kind %d n %d)\n", k, kind, n); return 1; }
        ++checked; stored += c == 0;
        free(s); free(rec);
    }
    if (!stored) { fprintf(stderr, "no block was stored\n"); return 1; }
    printf("block io bounds: %ld records (%ld stored), no access outside a buffer, every byte as expected\n", checked, stored);
    return 0;
}
