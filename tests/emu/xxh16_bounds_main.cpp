// wave_xxh32_x16 reads no byte outside [p, p + n): a program of its own for the address sanitizer (never loaded into Python, never
// run on a GPU; the build + run line is in scripts/README.md).  Every buffer is a heap allocation of exactly its length, at every
// start offset modulo 16 the allocator's alignment allows by over-allocating in FRONT only (the end of the buffer is the end of the
// allocation), so a load past p + n -- a prefetch included -- is a heap-buffer-overflow.  Digests are checked against a plain xxh32.
#define PLZ4_EMU 1
#include "../../plz4_amd/csrc/lz4_device.inl"
#include <stdio.h>
#include <stdlib.h>
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

int main()
{
    // (2047 .. 2064: around twice the ring's depth, where its refill loop first runs)
    static const int kLens[] = {0, 1, 15, 16, 17, 31, 32, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 2063, 2064, 100003};
    const int nLens = (int)(sizeof(kLens) / sizeof(kLens[0]));
    static const int kCounts[] = {1, 15, 16, 17, 33};
    unsigned seed = 12345u;
    long checked = 0;
    for (int desc = 0; desc < 2; ++desc) {
        plz4_emu_descending = desc;
        for (int count : kCounts) {
            for (int shift = 0; shift < 16; ++shift) {
                // buffer i: length kLens[(shift + 5 i) mod nLens], start offset (shift + 3 i) mod 16; the last wave is short
                std::vector<uint8_t*> alloc(count);
                std::vector<const uint8_t*> ptr(count);
                std::vector<int> len(count);
                for (int i = 0; i < count; ++i) {
                    const int n = kLens[(shift + 5 * i) % nLens], front = (shift + 3 * i) % 16;
                    alloc[i] = (uint8_t*)malloc((size_t)front + (size_t)n);       // (malloc(0) may be null: then n == 0 and nothing is read)
                    ptr[i] = alloc[i] ? alloc[i] + front : nullptr; len[i] = n;
                    for (int k = 0; k < n; ++k) { seed = seed * 1664525u + 1013904223u; alloc[i][front + k] = (uint8_t)(seed >> 24); }
                }
                for (int w0 = 0; w0 < count; w0 += 16) {
                    const uint8_t* p[64]; int n[64]; uint32_t h[64];
                    for (int lane = 0; lane < 64; ++lane) {
                        const int i = w0 + (lane >> 2);
                        p[lane] = i < count ? ptr[i] : nullptr;
                        n[lane] = i < count ? len[i] : -1;
                    }
                    wave_xxh32_x16(p, n, h);
                    for (int g = 0; g < 16 && w0 + g < count; ++g, ++checked) {
                        const uint32_t want = plain_xxh32(ptr[w0 + g], (size_t)len[w0 + g]);
                        if (h[4 * g] != want) {
                            fprintf(stderr, "digest mismatch: count %d shift %d buffer %d length %d: %08x != %08x\n", count, shift, w0 + g, len[w0 + g], h[4 * g], want);
                            return 1;
                        }
                    }
                }
                for (int i = 0; i < count; ++i) free(alloc[i]);
            }
        }
    }
    printf("xxh16 bounds: %ld digests, no read outside a buffer\n", checked);
    return 0;
}
