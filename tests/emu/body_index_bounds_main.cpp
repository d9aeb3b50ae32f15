// The frame-body index (wave_index_body, plz4_amd/csrc/lz4_body_index_device.inl) on hostile bodies reads no byte outside
// [body, body + bodyBytes) and writes no byte outside recOff[0 .. maxBlocks] and info: a program of its own for the address and
// undefined-behaviour sanitizers (never loaded into Python, never run on a GPU; tests/test_body_index_bounds.py builds and runs it).
// The body is a heap allocation that ends where the body ends, at every start offset modulo 8 by padding in FRONT only; recOff is an
// allocation of exactly (maxBlocks + 1) * 8 bytes and info one of exactly 16.  Every answer is checked against a walk written here,
// byte by byte, from the table of rules in include/plz4hip.h.  Inputs:
//   1  bodies of 0 .. 3 bytes;
//   2  a well-formed body, with and without an end mark, cut at each of its last 12 byte positions;
//   3  the size words 0x7FFFFFFF, 0xFFFFFFFF, bsz + 1 (with and without the stored bit) and 0 as the first, a middle and the last word;
//   4  a few thousand random streams of size words: records of random sizes around bsz, some stored, some of size 0, an end mark
//      somewhere or nowhere, random trailing bytes, a random cut -- over maxBlocks from 0 to beyond the records + two store groups;
//   5  a sparse mapping of 5 GiB that holds five size words: offsets beyond 2^32 (left out where the mapping is refused).
// Prints one line of counts; exit status 1 on a wrong answer, the sanitizer's on a bad access.
#define PLZ4_EMU 1
#include "../../plz4_amd/csrc/lz4_body_index_device.inl"
#include <stdio.h>
#include <stdlib.h>
#include <sys/mman.h>
#include <vector>

int plz4_emu_descending = 0;

using namespace plz4;

namespace {

struct Rng {
    uint32_t s;
    uint32_t next() { s = s * 1664525u + 1013904223u; return s >> 8; }
    int below(int n) { return n > 0 ? (int)(next() % (uint32_t)n) : 0; }
};

struct Want { std::vector<int64_t> off; int64_t end; int n; int status; };

// the rules of include/plz4hip.h, one byte at a time
Want walk(const uint8_t* body, int64_t bodyBytes, int bsz, bool checksum, int maxBlocks)
{
    Want w; int64_t off = 0; int i = 0;
    for (;;) {
        w.end = off;
        if (off == bodyBytes) { w.status = 1; break; }
        if (bodyBytes - off < 4) { w.status = 4; break; }
        const uint32_t word = (uint32_t)body[off] | (uint32_t)body[off + 1] << 8 | (uint32_t)body[off + 2] << 16 | (uint32_t)body[off + 3] << 24;
        if (word == 0) { w.status = 0; w.end = off + 4; break; }
        if (i == maxBlocks) { w.status = 2; break; }
        const int64_t size = (int64_t)(word & 0x7FFFFFFFu);
        if (size > (int64_t)bsz) { w.status = 3; break; }
        const int64_t need = 4 + size + (checksum ? 4 : 0);
        if (need > bodyBytes - off) { w.status = 5; break; }
        w.off.push_back(off); off += need; ++i;
    }
    w.n = i;
    while ((int64_t)w.off.size() < (int64_t)maxBlocks + 1) w.off.push_back(off);
    return w;
}

long g_checked = 0;

// the walk on exactly sized buffers against `want`
void run(const uint8_t* body, int64_t bodyBytes, int bsz, bool checksum, int maxBlocks, const Want& want, const char* what)
{
    const size_t nOff = (size_t)maxBlocks + 1;
    int64_t*   recOff = (int64_t*)malloc(nOff * sizeof(int64_t));
    BodyIndex* info   = (BodyIndex*)malloc(sizeof(BodyIndex));
    if (!recOff || !info) { fprintf(stderr, "out of memory\n"); exit(2); }
    for (size_t k = 0; k < nOff; ++k) recOff[k] = -99;
    info->end = -99; info->nBlocks = -99; info->status = -99;
    wave_index_body(body, bodyBytes, bsz, checksum, maxBlocks, recOff, info);
    bool ok = info->end == want.end && info->nBlocks == want.n && info->status == want.status;
    for (size_t k = 0; ok && k < nOff; ++k) ok = recOff[k] == want.off[k];
    if (!ok) {
        fprintf(stderr, "wrong answer: %s, bodyBytes %lld bsz %d checksum %d maxBlocks %d: end %lld n %d status %d, wanted %lld %d %d\n", what,
                (long long)bodyBytes, bsz, (int)checksum, maxBlocks, (long long)info->end, info->nBlocks, info->status, (long long)want.end, want.n, want.status);
        exit(1);
    }
    free(recOff); free(info);
    ++g_checked;
}

// `bytes` copied to the end of an allocation (front: bytes of padding before them), both lane orders, a set of maxBlocks
void check(const std::vector<uint8_t>& bytes, int64_t bodyBytes, int bsz, bool checksum, const std::vector<int>& maxBlocks, int front, const char* what)
{
    uint8_t* base = (uint8_t*)malloc((size_t)bodyBytes + (size_t)front + (bodyBytes + front == 0 ? 16 : 0));
    if (!base) { fprintf(stderr, "out of memory\n"); exit(2); }
    uint8_t* body = base + front + (bodyBytes + front == 0 ? 16 : 0);             // (an empty body: a pointer whose every byte is out of bounds)
    for (int64_t k = 0; k < bodyBytes; ++k) body[k] = bytes[(size_t)k];
    for (int mb : maxBlocks) {
        const Want want = walk(bytes.data(), bodyBytes, bsz, checksum, mb);
        for (int desc = 0; desc < 2; ++desc) { plz4_emu_descending = desc; run(body, bodyBytes, bsz, checksum, mb, want, what); }
    }
    plz4_emu_descending = 0;
    free(base);
}

void put32(std::vector<uint8_t>& b, uint32_t v) { for (int k = 0; k < 4; ++k) b.push_back((uint8_t)(v >> (8 * k))); }

// records of the given sizes (bit 31 of a size: stored), noise of 0x01..0xFF as payload and checksum; recStart: where each starts
std::vector<uint8_t> body_of(const std::vector<uint32_t>& words, bool checksum, Rng& rng, std::vector<size_t>* recStart)
{
    std::vector<uint8_t> b;
    for (uint32_t w : words) {
        if (recStart) recStart->push_back(b.size());
        put32(b, w);
        const uint32_t n = (w & 0x7FFFFFFFu) + (checksum ? 4u : 0u);
        for (uint32_t k = 0; k < n; ++k) b.push_back((uint8_t)(1 + rng.below(255)));
    }
    return b;
}

}  // namespace

int main()
{
    Rng rng{20240607u};
    const std::vector<int> few = {0, 1, 3, 4, 5, 6, 64, 80};
    for (int cks = 0; cks < 2; ++cks) for (int bsz : {1024, 65536}) {
        const bool checksum = cks != 0;
        // 1. bodies of 0 .. 3 bytes
        for (int n = 0; n < 4; ++n) for (int fill : {0x41, 0x00}) {
            const std::vector<uint8_t> b((size_t)n, (uint8_t)fill);
            for (int front = 0; front < 8; ++front) check(b, n, bsz, checksum, few, front, "short body");
        }
        // 2. the last 12 cuts of a well-formed body
        const std::vector<uint32_t> words = {17u, 0x80000000u | 40u, 0x80000000u, (uint32_t)bsz, 9u};
        for (int mark = 0; mark < 2; ++mark) {
            std::vector<size_t> at;
            std::vector<uint8_t> b = body_of(words, checksum, rng, &at);
            if (mark) put32(b, 0);
            for (int cut = 0; cut <= 12; ++cut) check(b, (int64_t)b.size() - cut, bsz, checksum, few, cut & 7, "cut body");
            // 3. hostile size words
            for (uint32_t w : {0x7FFFFFFFu, 0xFFFFFFFFu, (uint32_t)bsz + 1u, 0x80000000u | ((uint32_t)bsz + 1u), 0u}) for (size_t k : {(size_t)0, (size_t)2, (size_t)4}) {
                std::vector<uint8_t> h = b;
                for (int j = 0; j < 4; ++j) h[at[k] + (size_t)j] = (uint8_t)(w >> (8 * j));
                check(h, (int64_t)h.size(), bsz, checksum, few, (int)k + 1, "hostile word");
            }
        }
    }
    // 4. random streams of size words (bsz small, so that sizes around it are cheap)
    for (int it = 0; it < 4000; ++it) {
        const bool checksum = rng.below(2) != 0;
        const int bsz = 1 + rng.below(48);
        const int n = rng.below(4) == 0 ? rng.below(140) : rng.below(12);
        std::vector<uint32_t> words;
        for (int k = 0; k < n; ++k) {
            uint32_t size = (uint32_t)rng.below(bsz + 1);
            const int how = rng.below(40);
            if (how == 0) size = (uint32_t)bsz + 1u + (uint32_t)rng.below(3);
            if (how == 1) size = 0;
            if (how == 2) size = 0x7FFFFFFFu - (uint32_t)rng.below(12);
            words.push_back(size | (rng.below(4) == 0 ? 0x80000000u : 0u));
        }
        std::vector<uint8_t> b;
        {   // (a word above bsz has no payload behind it here: the walk must stop at it, so nothing behind it matters)
            for (uint32_t w : words) {
                put32(b, w);
                const uint32_t sz = w & 0x7FFFFFFFu;
                if (sz > (uint32_t)bsz) break;
                for (uint32_t k = 0; k < sz + (checksum ? 4u : 0u); ++k) b.push_back((uint8_t)(1 + rng.below(255)));
            }
        }
        if (rng.below(2)) { put32(b, 0); for (int k = rng.below(9); k > 0; --k) b.push_back((uint8_t)rng.below(256)); }
        int64_t bodyBytes = (int64_t)b.size();
        if (rng.below(3) == 0) bodyBytes -= rng.below((int)(bodyBytes < 14 ? bodyBytes + 1 : 14));
        const std::vector<int> mbs = {0, rng.below(n + 2), n, n + 1 + rng.below(140)};
        check(b, bodyBytes, bsz, checksum, mbs, rng.below(8), "random stream");
    }
    // 5. offsets beyond 2^32: five records of 0x46000000 + 13 k bytes in a sparse mapping that holds only their size words
    bool sparse = false;
    {
        const int bsz = 0x7FFFFFFF;
        int64_t total = 0, at[6];
        for (int k = 0; k < 5; ++k) { at[k] = total; total += 4 + (int64_t)0x46000000 + 13 * k; }
        at[5] = total;
        void* m = mmap(nullptr, (size_t)total, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
        if (m != MAP_FAILED) {
            sparse = true;
            uint8_t* body = (uint8_t*)m;
            for (int k = 0; k < 5; ++k) { const uint32_t w = (uint32_t)(0x46000000 + 13 * k) | (k == 2 ? 0x80000000u : 0u); for (int j = 0; j < 4; ++j) body[at[k] + j] = (uint8_t)(w >> (8 * j)); }
            for (int mb : {4, 5, 70}) {
                Want want; want.n = mb < 5 ? mb : 5; want.status = mb < 5 ? 2 : 1; want.end = at[want.n];
                for (int k = 0; k <= mb; ++k) want.off.push_back(at[k < want.n ? k : want.n]);
                run(body, total, bsz, false, mb, want, "sparse body");
            }
            Want cut; cut.n = 4; cut.status = 5; cut.end = at[4];
            for (int k = 0; k <= 8; ++k) cut.off.push_back(at[k < 4 ? k : 4]);
            run(body, total - 1, bsz, false, 8, cut, "sparse body, one byte short");
            munmap(m, (size_t)total);
        }
    }
    printf("body index bounds: %ld walks%s, no access outside a buffer\n", g_checked, sparse ? "" : " (the sparse 5 GiB mapping was refused: left out)");
    return 0;
}
