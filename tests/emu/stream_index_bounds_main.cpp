// The stream index (wave_index_stream, plz4_amd/csrc/lz4_stream_index_device.inl) on hostile streams reads no byte outside
// [bytes, bytes + nBytes) and writes no byte outside frames[0 .. maxFrames), recOff[0 .. maxRecs] and info: a program of its own for
// the address and undefined-behaviour sanitizers (never loaded into Python, never run on a GPU; tests/test_stream_index_bounds.py
// builds and runs it).  The stream is a heap allocation that ends where the stream ends, at every start offset modulo 8 by padding in
// FRONT only; frames is an allocation of exactly maxFrames * 64 bytes, recOff one of exactly (maxRecs + 1) * 8 and info one of
// exactly 32.  Every answer -- info, every listed entry, the canary in the entries behind them, recOff with its padding -- is checked
// against a walk written here, byte by byte, from the table of steps in include/plz4hip.h.  Inputs:
//   1  streams of 0 .. 7 bytes: zeros, noise, the start of a frame, the start of a skippable frame;
//   2  every header of 7, 11, 15 and 19 bytes cut at each byte, alone and behind a complete frame;
//   3  each bad header in turn: magics, versions, the reserved bit, block descriptors, every wrong hash byte;
//   4  skippable frames: all nibbles, sizes 0, up to the last byte, one more, 0xFFFFFFFF, the eighth byte missing;
//   5  a stream of frames with 0 .. 129 records, cut at each of its last 16 byte positions, over table sizes around what it holds;
//   6  a few thousand random streams: frames with random options and records, skippable frames, then random damage -- a flipped
//      byte, a cut, a magic followed by noise -- over random table sizes;
//   7  a sparse mapping of 5.5 GiB: a frame, two skippable frames of 3 and 2.5 GiB, a frame (left out where the mapping is refused).
// Prints one line of counts; exit status 1 on a wrong answer, the sanitizer's on a bad access.
#define PLZ4_EMU 1
#include "../../plz4_amd/csrc/lz4_stream_index_device.inl"
#include <stdio.h>
#include <stdlib.h>
#include <sys/mman.h>
#include <vector>

int plz4_emu_descending = 0;

using namespace plz4;

namespace {

typedef std::vector<uint8_t> Bytes;

struct Rng {
    uint32_t s;
    uint32_t next() { s = s * 1664525u + 1013904223u; return s >> 8; }
    int below(int n) { return n > 0 ? (int)(next() % (uint32_t)n) : 0; }
};

// xxh32 with seed 0, any length (the walk needs only the short form; this is the whole of it, from the algorithm's description)
uint32_t rotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
uint32_t xxh32(const uint8_t* p, size_t n)
{
    const uint32_t P1 = 2654435761u, P2 = 2246822519u, P3 = 3266489917u, P4 = 668265263u, P5 = 374761393u;
    const uint8_t* const e = p + n;
    uint32_t h;
    if (n >= 16) {
        uint32_t v1 = P1 + P2, v2 = P2, v3 = 0, v4 = 0u - P1;
        for (; e - p >= 16; p += 16) {
            v1 = rotl(v1 + le32(p) * P2, 13) * P1;      v2 = rotl(v2 + le32(p + 4) * P2, 13) * P1;
            v3 = rotl(v3 + le32(p + 8) * P2, 13) * P1;  v4 = rotl(v4 + le32(p + 12) * P2, 13) * P1;
        }
        h = rotl(v1, 1) + rotl(v2, 7) + rotl(v3, 12) + rotl(v4, 18);
    } else h = P5;
    h += (uint32_t)n;
    for (; e - p >= 4; p += 4) h = rotl(h + le32(p) * P3, 17) * P4;
    for (; p < e; ++p) h = rotl(h + *p * P5, 11) * P1;
    h ^= h >> 15; h *= P2; h ^= h >> 13; h *= P3; h ^= h >> 16;
    return h;
}

struct Want { std::vector<FrameIndex> frames; std::vector<int64_t> off; StreamIndex info; };

// the steps of include/plz4hip.h, one byte at a time; at(k): the stream's byte k
template <class At> Want walk(At at, int64_t nBytes, int maxFrames, int maxRecs)
{
    Want w; int64_t off = 0, end = 0, recEnd = 0; int status, nRecs = 0, nSkip = 0, maxBsz = 0; uint32_t fAnd = 0xFF, fOr = 0;
    const auto word = [&](int64_t o) { return (uint32_t)at(o) | (uint32_t)at(o + 1) << 8 | (uint32_t)at(o + 2) << 16 | (uint32_t)at(o + 3) << 24; };
    for (;;) {
        end = off;
        if (off == nBytes) { status = 0; break; }
        if ((int)w.frames.size() == maxFrames) { status = 1; break; }
        const int64_t left = nBytes - off;
        if (left < 7) { status = 3; break; }
        const uint32_t magic = word(off);
        FrameIndex f; memset(&f, 0, sizeof f);
        f.hdrOff = off; f.firstRec = nRecs;
        if (magic >= 0x184D2A50u && magic <= 0x184D2A5Fu) {
            if (left < 8) { status = 3; break; }
            const int64_t size = (int64_t)word(off + 4);
            if (size > left - 8) { status = 9; break; }
            f.bodyOff = off + 8; f.end = off + 8 + size; f.contentSz = (uint64_t)size; f.kind = 1; f.nibble = (uint8_t)(magic & 15u);
            w.frames.push_back(f); ++nSkip; off = f.end;
            continue;
        }
        if (magic != 0x184D2204u) { status = 4; break; }
        const uint32_t flg = at(off + 4), bd = at(off + 5);
        if ((flg >> 6) != 1) { status = 5; break; }
        if (flg & 2) { status = 6; break; }
        if (((bd >> 4) & 7) < 4 || (bd & 0x80) || (bd & 0x0F)) { status = 7; break; }
        const int len = 7 + ((flg & 8) ? 8 : 0) + ((flg & 1) ? 4 : 0);
        if ((int64_t)len > left) { status = 3; break; }
        uint8_t hdr[19];
        for (int k = 0; k < len; ++k) hdr[k] = at(off + k);
        if (hdr[len - 1] != ((xxh32(hdr + 4, (size_t)len - 5) >> 8) & 0xFF)) { status = 8; break; }
        f.bodyOff = off + len; f.flags = (uint8_t)flg; f.blockDesc = (uint8_t)bd; f.bsz = 65536 << 2 * (int)(((bd >> 4) & 7) - 4);
        if (flg & 8) for (int k = 7; k >= 0; --k) f.contentSz = f.contentSz << 8 | hdr[6 + k];
        if (flg & 1) f.dictId = le32(hdr + len - 5);
        fAnd &= flg; fOr |= flg; if (f.bsz > maxBsz) maxBsz = f.bsz;
        off += len;
        int body;
        for (;;) {
            end = off;
            if (nBytes - off < 4) { body = 4; break; }
            const uint32_t sw = word(off);
            if (sw == 0) { body = 0; end = off + 4; break; }
            if (nRecs == maxRecs) { body = 2; break; }
            const int64_t size = (int64_t)(sw & 0x7FFFFFFFu);
            if (size > (int64_t)f.bsz) { body = 3; break; }
            const int64_t need = 4 + size + ((flg & 16) ? 4 : 0);
            if (need > nBytes - off) { body = 5; break; }
            w.off.push_back(off); ++nRecs; off += need; recEnd = off;
        }
        f.nRecs = nRecs - f.firstRec; f.status = body; f.end = end;
        status = body == 0 ? -1 : body == 2 ? 2 : 10;
        if (body == 0 && (flg & 4)) {
            if (nBytes - end < 4) status = 11;
            else { f.contentSum = word(end); end += 4; f.end = end; }
        }
        w.frames.push_back(f);
        if (status >= 0) break;
        off = end;
    }
    memset(&w.info, 0, sizeof w.info);
    w.info.end = end; w.info.nFrames = (int)w.frames.size(); w.info.nRecs = nRecs; w.info.status = status; w.info.nSkippable = nSkip;
    w.info.maxBsz = maxBsz; w.info.flagsAnd = (uint8_t)((int)w.frames.size() > nSkip ? fAnd : 0); w.info.flagsOr = (uint8_t)fOr;
    while ((int64_t)w.off.size() < (int64_t)maxRecs + 1) w.off.push_back(recEnd);
    return w;
}

long g_checked = 0;
int  g_seen = 0;                                             // bit s: a stream that stopped with status s was among them

// the walk on exactly sized buffers against `want`
void run(const uint8_t* bytes, int64_t nBytes, int maxFrames, int maxRecs, const Want& want, const char* what)
{
    const size_t nOff = (size_t)maxRecs + 1;
    FrameIndex*  frames = maxFrames ? (FrameIndex*)malloc((size_t)maxFrames * sizeof(FrameIndex)) : nullptr;
    int64_t*     recOff = (int64_t*)malloc(nOff * sizeof(int64_t));
    StreamIndex* info   = (StreamIndex*)malloc(sizeof(StreamIndex));
    if ((maxFrames && !frames) || !recOff || !info) { fprintf(stderr, "out of memory\n"); exit(2); }
    if (maxFrames) memset(frames, 0xC7, (size_t)maxFrames * sizeof(FrameIndex));
    for (size_t k = 0; k < nOff; ++k) recOff[k] = -99;
    memset(info, 0xC7, sizeof *info);
    wave_index_stream(bytes, nBytes, maxFrames, maxRecs, frames, recOff, info);
    bool ok = memcmp(info, &want.info, sizeof *info) == 0;
    for (int k = 0; ok && k < maxFrames; ++k) {
        if (k < want.info.nFrames) ok = memcmp(frames + k, &want.frames[(size_t)k], sizeof(FrameIndex)) == 0;
        else for (size_t j = 0; ok && j < sizeof(FrameIndex); ++j) ok = ((const uint8_t*)(frames + k))[j] == 0xC7;
    }
    for (size_t k = 0; ok && k < nOff; ++k) ok = recOff[k] == want.off[k];
    if (!ok) {
        fprintf(stderr, "wrong answer: %s, nBytes %lld maxFrames %d maxRecs %d: end %lld frames %d recs %d status %d, wanted %lld %d %d %d\n", what,
                (long long)nBytes, maxFrames, maxRecs, (long long)info->end, info->nFrames, info->nRecs, info->status, (long long)want.info.end,
                want.info.nFrames, want.info.nRecs, want.info.status);
        exit(1);
    }
    free(frames); free(recOff); free(info);
    g_seen |= 1 << want.info.status;
    ++g_checked;
}

struct Sizes { int frames, recs; };

// the first nBytes of `s` copied to the end of an allocation (front: bytes of padding before them), both lane orders, a set of sizes
void check(const Bytes& s, int64_t nBytes, const std::vector<Sizes>& sizes, int front, const char* what)
{
    uint8_t* base = (uint8_t*)malloc((size_t)nBytes + (size_t)front + (nBytes + front == 0 ? 16 : 0));
    if (!base) { fprintf(stderr, "out of memory\n"); exit(2); }
    uint8_t* bytes = base + front + (nBytes + front == 0 ? 16 : 0);               // (an empty stream: a pointer whose every byte is out of bounds)
    for (int64_t k = 0; k < nBytes; ++k) bytes[k] = s[(size_t)k];
    for (const Sizes& z : sizes) {
        const Want want = walk([&](int64_t k) { return s[(size_t)k]; }, nBytes, z.frames, z.recs);
        for (int desc = 0; desc < 2; ++desc) { plz4_emu_descending = desc; run(bytes, nBytes, z.frames, z.recs, want, what); }
    }
    plz4_emu_descending = 0;
    free(base);
}
void check(const Bytes& s, const std::vector<Sizes>& sizes, int front, const char* what) { check(s, (int64_t)s.size(), sizes, front, what); }

void put32(Bytes& b, uint32_t v) { for (int k = 0; k < 4; ++k) b.push_back((uint8_t)(v >> (8 * k))); }
void noise(Bytes& b, size_t n, Rng& rng) { for (size_t k = 0; k < n; ++k) b.push_back((uint8_t)(1 + rng.below(255))); }
void append(Bytes& b, const Bytes& x) { b.insert(b.end(), x.begin(), x.end()); }

// a frame header: FLG with version 1 and the given option bits (0x20 independent, 0x10 block checksums, 0x08 content size,
// 0x04 content checksum, 0x01 dictionary id), BD id
Bytes header(uint32_t opts, int bdId, Rng& rng)
{
    Bytes h; put32(h, 0x184D2204u);
    h.push_back((uint8_t)(0x40u | (opts & 0x3Du))); h.push_back((uint8_t)(bdId << 4));
    if (opts & 8) noise(h, 8, rng);
    if (opts & 1) noise(h, 4, rng);
    h.push_back((uint8_t)(xxh32(h.data() + 4, h.size() - 4) >> 8));
    return h;
}

// a whole frame: header, records of the given size words over noise (bit 31: stored), end mark, a content checksum of noise
Bytes frame(uint32_t opts, int bdId, const std::vector<uint32_t>& words, Rng& rng, bool endMark = true)
{
    Bytes f = header(opts, bdId, rng);
    for (uint32_t w : words) { put32(f, w); noise(f, (w & 0x7FFFFFFFu) + ((opts & 16) ? 4u : 0u), rng); }
    if (endMark) { put32(f, 0); if (opts & 4) noise(f, 4, rng); }
    return f;
}

Bytes skippable(int nibble, uint32_t payload, uint32_t declared, Rng& rng)
{
    Bytes f; put32(f, 0x184D2A50u | (uint32_t)nibble); put32(f, declared); noise(f, payload, rng);
    return f;
}

std::vector<uint32_t> some_words(int n, Rng& rng)
{
    std::vector<uint32_t> w;
    for (int k = 0; k < n; ++k) w.push_back((uint32_t)rng.below(40) | (rng.below(4) == 0 ? 0x80000000u : 0u));
    return w;
}

}  // namespace

int main()
{
    Rng rng{20240911u};
    const std::vector<Sizes> few = {{0, 0}, {1, 0}, {1, 1}, {2, 3}, {3, 5}, {4, 64}, {8, 80}};
    const Bytes lead = frame(0x34, 4, {5u, 0x80000003u}, rng);
    // 1. streams of 0 .. 7 bytes
    {
        const Bytes f = frame(0x20, 4, {3u}, rng), sk = skippable(5, 0, 0, rng);
        for (int n = 0; n <= 7; ++n) for (int front = 0; front < 8; ++front) {
            check(Bytes((size_t)n, 0), few, front, "zeros");
            check(Bytes((size_t)n, 0x41), few, front, "noise");
            check(f, n, few, front, "the start of a frame");
            check(sk, n, few, front, "the start of a skippable frame");
        }
    }
    // 2. every header cut at each byte; 3. bad headers
    for (uint32_t opts = 0; opts < 64; ++opts) {
        if (opts & 2) continue;
        for (int bdId = 4; bdId <= 7; ++bdId) {
            const Bytes f = frame(opts, bdId, {7u, 0x80000000u}, rng);
            const size_t hlen = 7 + ((opts & 8) ? 8 : 0) + ((opts & 1) ? 4 : 0);
            Bytes both = lead; append(both, f);
            check(both, few, (int)opts & 7, "a complete frame");
            if (bdId != 4 + (int)(opts & 3)) continue;
            for (size_t cut = 0; cut <= hlen + 4; ++cut) {
                check(f, (int64_t)cut, few, (int)cut & 7, "cut header");
                check(both, (int64_t)(lead.size() + cut), few, (int)cut & 7, "cut header behind a frame");
            }
        }
    }
    for (uint32_t opts : {0x20u, 0x3Du}) {
        const Bytes good = frame(opts, 6, {7u, 9u}, rng);
        const size_t hlen = opts == 0x20u ? 7 : 19;
        const auto with = [&](size_t at, uint32_t v, bool fix, const char* what) {
            Bytes f = good; f[at] = (uint8_t)v;
            if (fix) f[hlen - 1] = (uint8_t)(xxh32(f.data() + 4, hlen - 5) >> 8);
            Bytes s = lead; append(s, f);
            check(s, few, (int)(at + v) & 7, what);
        };
        for (uint32_t m : {0x184D2203u, 0x184D2205u, 0x184D2A60u, 0x184D2A4Fu, 0x04224D18u, 0u}) {
            Bytes f = good; for (int j = 0; j < 4; ++j) f[(size_t)j] = (uint8_t)(m >> (8 * j));
            Bytes s = lead; append(s, f);
            check(s, few, 3, "bad magic");
        }
        for (uint32_t v : {0u, 2u, 3u}) { with(4, (good[4] & 0x3Fu) | v << 6, true, "version"); with(4, (good[4] & 0x3Fu) | v << 6, false, "version, stale hash"); }
        with(4, good[4] | 2u, true, "reserved bit");
        for (uint32_t id = 0; id < 4; ++id) with(5, id << 4, true, "BD id");
        with(5, good[5] | 0x80u, true, "BD bit 7");
        for (int bit = 0; bit < 4; ++bit) with(5, good[5] | 1u << bit, true, "BD low nibble");
        for (uint32_t v = 0; v < 256; ++v) if (v != good[hlen - 1]) with(hlen - 1, v, false, "hash byte");
    }
    // 4. skippable frames
    for (int nib = 0; nib < 16; ++nib) {
        Bytes s = skippable(nib, (uint32_t)nib, (uint32_t)nib, rng); append(s, lead); append(s, skippable(15 - nib, 0, 0, rng));
        check(s, few, nib & 7, "skippable in front and last");
    }
    for (uint32_t more : {0u, 1u, 2u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFF6u}) {
        Bytes s = lead; append(s, skippable(3, 9, 9 + more, rng));
        check(s, few, 5, "skippable up to the last byte and beyond");
        for (int cut = 1; cut <= 10; ++cut) check(s, (int64_t)s.size() - cut, few, cut & 7, "skippable, cut");
        append(s, lead);
        check(s, few, 2, "skippable whose size reaches into the next frame");
    }
    // 5. frames of 0 .. 129 records, cut at each of the last 16 positions
    {
        Bytes s; int nRecs = 0, nFrames = 0;
        for (int n : {63, 1, 64, 0, 65, 129}) { append(s, frame(n & 1 ? 0x34u : 0x20u, 4 + (n & 3), some_words(n, rng), rng)); nRecs += n; ++nFrames; }
        std::vector<Sizes> around;
        for (int mf : {nFrames - 1, nFrames, nFrames + 1, 0}) for (int mr : {nRecs - 1, nRecs, nRecs + 1, nRecs + 70, 0, 63, 64, 128}) around.push_back({mf, mr});
        check(s, around, 1, "frames of 63, 1, 64, 0, 65, 129 records");
        for (int cut = 1; cut <= 16; ++cut) check(s, (int64_t)s.size() - cut, {{nFrames, nRecs}, {nFrames + 1, nRecs + 70}}, cut & 7, "cut in the last frame");
        Bytes open = lead; append(open, frame(0x34, 5, some_words(5, rng), rng, false));
        check(open, few, 0, "unterminated last frame");
        put32(open, 65536u * 4u + 1u); noise(open, 9, rng);
        check(open, few, 0, "a size word above bsz");
    }
    // 6. random streams, then random damage
    for (int it = 0; it < 4000; ++it) {
        Bytes s; int nRecs = 0, nFrames = 0;
        for (int k = rng.below(6); k >= 0; --k) {
            const int how = rng.below(8);
            if (how < 2) {
                const uint32_t pay = (uint32_t)rng.below(30);
                append(s, skippable(rng.below(16), pay, pay, rng));
            } else {
                const int n = rng.below(5) == 0 ? rng.below(140) : rng.below(6);
                append(s, frame((uint32_t)rng.below(64) & 0x3Du, 4 + rng.below(4), some_words(n, rng), rng, k != 0 || rng.below(4) != 0));
                nRecs += n;
            }
            ++nFrames;
        }
        int64_t nBytes = (int64_t)s.size();
        switch (rng.below(6)) {
        case 0: s[(size_t)rng.below((int)s.size())] ^= (uint8_t)(1 << rng.below(8)); break;
        case 1: nBytes -= rng.below((int)(nBytes < 24 ? nBytes + 1 : 24)); break;
        case 2: put32(s, rng.below(2) ? 0x184D2204u : 0x184D2A50u + (uint32_t)rng.below(16)); for (int k = rng.below(20); k > 0; --k) s.push_back((uint8_t)rng.below(256)); nBytes = (int64_t)s.size(); break;
        case 3: { const size_t at = (size_t)rng.below((int)s.size()); s[at] = (uint8_t)rng.below(256); break; }
        default: break;
        }
        const std::vector<Sizes> zs = {{nFrames + 2, nRecs + 1 + rng.below(140)}, {rng.below(nFrames + 2), rng.below(nRecs + 2)}, {nFrames, nRecs}, {0, 0}};
        check(s, nBytes, zs, rng.below(8), "random stream");
    }
    // 7. offsets beyond 2^32: a frame, skippable frames of 3 GiB and 2.5 GiB + 13 in a sparse mapping, a frame
    bool sparse = false;
    {
        const Bytes a = frame(0x34, 4, {5u, 0x80000007u, 1u}, rng), b = frame(0x24, 7, {9u, 2u}, rng);
        const int64_t s1 = (int64_t)3 << 30, s2 = ((int64_t)5 << 29) + 13;
        const int64_t at1 = (int64_t)a.size(), at2 = at1 + 8 + s1, atB = at2 + 8 + s2, total = atB + (int64_t)b.size();
        void* m = mmap(nullptr, (size_t)total, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
        if (m != MAP_FAILED) {
            sparse = true;
            uint8_t* p = (uint8_t*)m;
            for (size_t k = 0; k < a.size(); ++k) p[k] = a[k];
            for (size_t k = 0; k < b.size(); ++k) p[atB + (int64_t)k] = b[k];
            for (int j = 0; j < 4; ++j) {
                p[at1 + j] = (uint8_t)(0x184D2A5Cu >> (8 * j)); p[at1 + 4 + j] = (uint8_t)((uint64_t)s1 >> (8 * j));
                p[at2 + j] = (uint8_t)(0x184D2A51u >> (8 * j)); p[at2 + 4 + j] = (uint8_t)((uint64_t)s2 >> (8 * j));
            }
            // the walk written here reads the same mapping, but only header bytes, size words and trailers: it is the table's walk
            const auto at = [&](int64_t k) { return p[k]; };
            for (const Sizes z : {Sizes{4, 5}, Sizes{6, 80}, Sizes{3, 5}, Sizes{4, 4}})
                run(p, total, z.frames, z.recs, walk(at, total, z.frames, z.recs), "sparse stream");
            const Want whole = walk(at, total, 4, 5);
            if (whole.info.status != 0 || whole.info.end != total || whole.frames[3].hdrOff != atB || whole.off[3] != atB + 7) { fprintf(stderr, "sparse stream: the walk itself is off\n"); return 1; }
            run(p, atB - 1, 4, 5, walk(at, atB - 1, 4, 5), "sparse stream, one byte short of the second skippable frame");
            run(p, total - 5, 4, 5, walk(at, total - 5, 4, 5), "sparse stream, cut in the end mark");
            munmap(m, (size_t)total);
        }
    }
    if ((g_seen & 0xFFF) != 0xFFF) { fprintf(stderr, "the inputs never reached every status: seen mask %03x\n", g_seen); return 1; }
    printf("stream index bounds: %ld walks%s, no access outside a buffer\n", g_checked, sparse ? "" : " (the sparse 5.5 GiB mapping was refused: left out)");
    return 0;
}
