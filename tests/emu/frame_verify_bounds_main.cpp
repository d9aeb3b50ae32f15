// plz4hip_dev_verify_frames' walk (wave_verify_frames, wave_verify_summary) reads nothing but what the header says it reads: a program
// of its own for the address and undefined-behaviour sanitizers (never loaded into Python, never run on a GPU; the build + run line is
// in scripts/README.md).  status / result are heap allocations of exactly maxRecs entries, frames and verdicts of exactly maxFrames,
// info and sv of exactly 32 bytes.  dst ends with the last byte a walk by the rules may read, and inside it EVERY byte is poisoned
// except the first result[i] bytes of the records that walk hashes: a load of a record behind a bad one, of a frame that is not
// hashed, or of a byte at or beyond dst + i * dstStride + result[i] -- a prefetch included -- ends the program with the sanitizer's
// report.  Every answer is checked against a walk written here.
#define PLZ4_EMU 1
#include "../../plz4_amd/csrc/lz4_frame_verify_device.inl"
#include <sanitizer/asan_interface.h>
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

static unsigned g_seed = 2463534242u;
static unsigned rnd() { g_seed ^= g_seed << 13; g_seed ^= g_seed >> 17; g_seed ^= g_seed << 5; return g_seed; }
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (unsigned)(hi - lo + 1)); }

struct Table {
    std::vector<FrameIndex> frames;                          // the entries the table really has
    int infoFrames = 0, maxFrames = 0, maxRecs = 0, cap = 0;
    int64_t stride = 0;                                      // a multiple of 8: the poison's granule
    std::vector<int32_t> result, status;                     // maxRecs entries
};

static FrameIndex entry(int firstRec, int nRecs, uint32_t flg, int status, int kind = 0)
{
    FrameIndex e;
    memset(&e, 0, sizeof e);
    e.firstRec = firstRec; e.nRecs = nRecs; e.flags = (uint8_t)flg; e.status = status; e.kind = (uint8_t)kind; e.bsz = 65536; e.blockDesc = 0x40;
    return e;
}

// the walk by the header's table over `plain` (maxRecs * stride bytes nobody poisons); read[i]: record i's bytes are hashed
static void expect(const Table& t, const std::vector<uint8_t>& plain, std::vector<FrameVerdict>& want, StreamVerdict& sv, std::vector<char>& read)
{
    const int nf = t.infoFrames < 0 ? 0 : t.infoFrames > t.maxFrames ? t.maxFrames : t.infoFrames;
    want.assign((size_t)nf, FrameVerdict());
    read.assign((size_t)t.maxRecs, 0);
    memset(&sv, 0, sizeof sv);
    sv.firstBadFrame = -1; sv.nFrames = nf;
    for (int f = 0; f < nf; ++f) {
        const FrameIndex& e = t.frames[(size_t)f];
        FrameVerdict& v = want[(size_t)f];
        memset(&v, 0, sizeof v);
        v.firstBad = -1; v.status = -1;
        if (e.kind == 1) v.status = kFrameSkippable;
        else {
            const bool complete = e.status == kBodyEndMark, hashed = complete && (e.flags & 4);
            std::vector<uint8_t> bytes;
            if (e.firstRec < 0 || e.nRecs < 0 || (int64_t)e.firstRec + e.nRecs > t.maxRecs) v.status = kFrameRange;
            else
                for (int i = e.firstRec; i < e.firstRec + e.nRecs; ++i) {
                    if (t.status[(size_t)i] != 0) { v.status = kFrameBlock; v.firstBad = i; v.blockStatus = t.status[(size_t)i]; break; }
                    const int r = t.result[(size_t)i];
                    if (r < 0 || r > t.cap) { v.status = kFrameRange; v.firstBad = i; break; }
                    v.contentSz += (uint64_t)r;
                    if (hashed) { read[(size_t)i] = 1; bytes.insert(bytes.end(), plain.begin() + i * t.stride, plain.begin() + i * t.stride + r); }
                }
            if (hashed) v.contentSum = plain_xxh32(bytes.data(), bytes.size());
            if (v.status < 0) {
                if (!complete) v.status = kFrameIncomplete;
                else if ((e.flags & 4) && v.contentSum != e.contentSum) v.status = kFrameContentHash;
                else if ((e.flags & 8) && v.contentSz != e.contentSz) v.status = kFrameContentSize;
                else v.status = kFrameOk;
            }
        }
        if (v.status == kFrameOk) ++sv.nOk;
        if (v.status == kFrameSkippable) ++sv.nSkippable;
        if (sv.firstBadFrame < 0) {
            sv.contentBytes += (int64_t)v.contentSz;
            if (v.status > kFrameSkippable) { sv.firstBadFrame = f; sv.status = v.status; }
        }
    }
}

static long g_checked = 0, g_frames = 0;

// stored: give the complete checksummed frames of the table their right checksum / size first (where `fix` says so)
static int run(Table t, const char* what, int nWaves, unsigned fixMask = ~0u)
{
    std::vector<uint8_t> plain((size_t)(t.maxRecs * t.stride));
    for (auto& b : plain) b = (uint8_t)(rnd() >> 24);
    std::vector<FrameVerdict> want; StreamVerdict wsv; std::vector<char> read;
    expect(t, plain, want, wsv, read);
    for (size_t f = 0; f < want.size(); ++f)                  // entry f stores what the walk finds, unless it is to lie
        if ((fixMask >> (f & 31)) & 1u) {
            if (t.frames[f].flags & 4) t.frames[f].contentSum = want[f].contentSum;
            if (t.frames[f].flags & 8) t.frames[f].contentSz = want[f].contentSz;
        }
    expect(t, plain, want, wsv, read);
    // dst: up to the end of the last record that is read, everything else poisoned
    int64_t need = 0;
    for (int i = 0; i < t.maxRecs; ++i) if (read[(size_t)i]) need = i * t.stride + t.result[(size_t)i];
    uint8_t* const dst = (uint8_t*)malloc((size_t)need + 1);     // (+ 1: malloc(0) may be null, and the byte is poisoned like the rest)
    if (need) memcpy(dst, plain.data(), (size_t)need);
    ASAN_POISON_MEMORY_REGION(dst, (size_t)need + 1);
    for (int i = 0; i < t.maxRecs; ++i) if (read[(size_t)i]) ASAN_UNPOISON_MEMORY_REGION(dst + i * t.stride, (size_t)t.result[(size_t)i]);
    FrameIndex* const frames = (FrameIndex*)malloc(sizeof(FrameIndex) * (size_t)t.maxFrames + 1);
    for (int f = 0; f < t.maxFrames; ++f) {
        if (f < (int)t.frames.size()) frames[f] = t.frames[(size_t)f]; else memset((void*)(frames + f), 0xC7, sizeof(FrameIndex));
    }
    ASAN_POISON_MEMORY_REGION((uint8_t*)frames + sizeof(FrameIndex) * (size_t)t.maxFrames, 1);
    int32_t* const result = (int32_t*)malloc(4 * (size_t)t.maxRecs + 4);
    int32_t* const status = (int32_t*)malloc(4 * (size_t)t.maxRecs + 4);
    for (int i = 0; i < t.maxRecs; ++i) { result[i] = t.result[(size_t)i]; status[i] = t.status[(size_t)i]; }
    ASAN_POISON_MEMORY_REGION(result + t.maxRecs, 4);
    ASAN_POISON_MEMORY_REGION(status + t.maxRecs, 4);
    FrameVerdict* const verdicts = (FrameVerdict*)malloc(sizeof(FrameVerdict) * (size_t)t.maxFrames + 1);
    memset((void*)verdicts, 0xC7, sizeof(FrameVerdict) * (size_t)t.maxFrames);
    ASAN_POISON_MEMORY_REGION((uint8_t*)verdicts + sizeof(FrameVerdict) * (size_t)t.maxFrames, 1);
    StreamIndex* const info = (StreamIndex*)malloc(sizeof(StreamIndex));
    memset((void*)info, 0, sizeof *info);
    info->nFrames = t.infoFrames;
    StreamVerdict* const sv = (StreamVerdict*)malloc(sizeof(StreamVerdict));
    memset((void*)sv, 0xC7, sizeof *sv);

    const int groups = (t.maxFrames + 15) / 16, grid = groups < nWaves ? groups : nWaves;
    for (int w = 0; w < grid; ++w)
        wave_verify_frames(frames, info, t.maxFrames, dst, t.stride, t.cap, result, status, t.maxRecs, verdicts, w, grid);
    wave_verify_summary(info, t.maxFrames, verdicts, sv);

    int bad = 0;
    if (memcmp(sv, &wsv, sizeof wsv)) {
        fprintf(stderr, "%s: sv {%lld %d %d %d %d %d %d} != {%lld %d %d %d %d %d %d}\n", what, (long long)sv->contentBytes, sv->firstBadFrame, sv->status,
                sv->nFrames, sv->nOk, sv->nSkippable, sv->reserved, (long long)wsv.contentBytes, wsv.firstBadFrame, wsv.status, wsv.nFrames, wsv.nOk,
                wsv.nSkippable, wsv.reserved);
        bad = 1;
    }
    for (size_t f = 0; f < want.size() && !bad; ++f)
        if (memcmp(verdicts + f, &want[f], sizeof(FrameVerdict))) {
            fprintf(stderr, "%s: frame %zu {%llu %08x %d %d %d} != {%llu %08x %d %d %d}\n", what, f, (unsigned long long)verdicts[f].contentSz,
                    verdicts[f].contentSum, verdicts[f].status, verdicts[f].firstBad, verdicts[f].blockStatus, (unsigned long long)want[f].contentSz,
                    want[f].contentSum, want[f].status, want[f].firstBad, want[f].blockStatus);
            bad = 1;
        }
    for (size_t k = sizeof(FrameVerdict) * want.size(); k < sizeof(FrameVerdict) * (size_t)t.maxFrames && !bad; ++k)
        if (((const uint8_t*)verdicts)[k] != 0xC7) { fprintf(stderr, "%s: a store behind verdicts[nFrames)\n", what); bad = 1; }
    ++g_checked; g_frames += (long)want.size();
    ASAN_UNPOISON_MEMORY_REGION(dst, (size_t)need + 1);
    free(dst); free(frames); free(result); free(status); free(verdicts); free(info); free(sv);
    return bad;
}

// a frame of the given pieces behind the records the table already has
static void add_frame(Table& t, const std::vector<int>& pieces, uint32_t flg = 0x64, int entryStatus = kBodyEndMark)
{
    t.frames.push_back(entry((int)t.result.size(), (int)pieces.size(), flg, entryStatus));
    for (int n : pieces) { t.result.push_back(n); t.status.push_back(0); }
}
static void close_table(Table& t, int cap)
{
    t.cap = cap; t.stride = (cap + 7) / 8 * 8; t.maxRecs = (int)t.result.size(); t.maxFrames = t.infoFrames = (int)t.frames.size();
}

int main()
{
    static const int kLens[] = {0, 1, 3, 4, 15, 16, 17, 31, 32, 127, 128, 1023, 1024, 1025, 2047, 2048, 2049, 2048 + 16 * 3 + 5, 2048 + 16 * 64 + 7,
                                2048 + 16 * 129 + 1};
    const int kCap = 2048 + 16 * 129 + 1;
    int bad = 0;
    for (int desc = 0; desc < 2 && !bad; ++desc) {
        plz4_emu_descending = desc;
        // 1. the piece cases: every length behind every fill; and with the block under test the LAST one read, each block of a frame in
        //    turn (the next one is marked bad: the walk stops in front of it, dst ends with the block under test)
        {
            Table t;
            for (int n : kLens) for (int fill = 0; fill < 16; ++fill) { std::vector<int> p; if (fill) p.push_back(fill); p.push_back(n); p.push_back(7); add_frame(t, p); }
            close_table(t, kCap);
            bad |= run(t, "every length behind every fill", 1 << 20);
            bad |= run(t, "every length behind every fill, 3 waves", 3);
        }
        for (int n : kLens)
            for (int fill = 0; fill < 16 && !bad; fill += 5)
                for (int last = 0; last < 4 && !bad; ++last) {
                    Table t;
                    add_frame(t, {fill, n, n, 7, 9});
                    close_table(t, kCap);
                    t.status[(size_t)last + 1] = 3;             // records 0 .. last are read, dst ends behind record `last`
                    bad |= run(t, "each block in turn", 1);
                }
        {
            Table t;
            add_frame(t, std::vector<int>(40, 1)); add_frame(t, std::vector<int>(20, 0)); add_frame(t, {}); add_frame(t, {15}); add_frame(t, {16});
            add_frame(t, {7, 8}); add_frame(t, {8, 8}); add_frame(t, {0, 0, 15}); add_frame(t, {5, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 3, 33, 1});
            for (int k = 0; k < 33; ++k) add_frame(t, {(k * 37) % 300, (k * 101) % 600, k % 19}, k % 3 ? 0x64u : 0x6Cu);
            close_table(t, 600);
            bad |= run(t, "tiny pieces and 42 frames", 1 << 20);
            bad |= run(t, "tiny pieces and 42 frames, 2 waves", 2);
            bad |= run(t, "tiny pieces and 42 frames, wrong sums", 1, 0x55555555u);
        }
        // 2. hostile tables: lying firstRec / nRecs / result, frames that are not hashed, tables shorter than info says
        {
            Table t;
            add_frame(t, {100, 200, 50}); add_frame(t, {10, 20, 30}); add_frame(t, {10, 20, 30}, 0x60u); add_frame(t, {10, 20, 30}, 0x64u, kBodyTruncatedBlock);
            add_frame(t, {40, 50});
            close_table(t, 300);
            t.frames.push_back(entry(-1, 2, 0x64u, 0)); t.frames.push_back(entry(2, -1, 0x64u, 0)); t.frames.push_back(entry(0x7FFFFFFF, 0x7FFFFFFF, 0x64u, 0));
            t.frames.push_back(entry(t.maxRecs - 1, 2, 0x64u, 0)); t.frames.push_back(entry(t.maxRecs, 0, 0x6Cu, 0)); t.frames.push_back(entry(t.maxRecs + 1, 0, 0x64u, 0));
            t.frames.push_back(entry(0, t.maxRecs, 0x64u, 0)); t.frames.push_back(entry(-7, -7, 0, 0, 1)); t.frames.push_back(entry(3, 5, 0x6Cu, 0));
            t.maxFrames = t.infoFrames = (int)t.frames.size();
            bad |= run(t, "lying table entries", 1 << 20);
            Table u = t;
            u.result[1] = -1; u.result[4] = 301; u.result[7] = 0x7FFFFFFF; u.result[10] = (int32_t)0x80000000u; u.status[12] = 1; u.status[13] = -5;
            bad |= run(u, "lying results", 1 << 20);
            u = t; u.infoFrames = 0x7FFFFFFF; u.maxFrames = 9;
            bad |= run(u, "info->nFrames above maxFrames", 1 << 20);
            u = t; u.infoFrames = -3;
            bad |= run(u, "info->nFrames negative", 1 << 20);
            u = t; u.maxFrames = 0;
            bad |= run(u, "maxFrames 0", 1 << 20);
            u = t; u.maxRecs = 0; u.result.clear(); u.status.clear();
            bad |= run(u, "maxRecs 0", 1 << 20);
            u = t; u.maxRecs -= 1; u.result.pop_back(); u.status.pop_back();
            bad |= run(u, "one record short", 1 << 20);
        }
        // 3. random tables
        for (int round = 0; round < 2500 && !bad; ++round) {
            Table t;
            t.cap = rnd_in(0, 3) ? rnd_in(0, 200) : rnd_in(900, 2300);
            t.stride = (t.cap + 7) / 8 * 8 + 8 * rnd_in(0, 2);
            t.maxRecs = rnd_in(0, 40);
            for (int i = 0; i < t.maxRecs; ++i) {
                const int k = rnd_in(0, 23);
                t.result.push_back(k == 0 ? -rnd_in(1, 9) : k == 1 ? t.cap + rnd_in(1, 70000) : k == 2 ? t.cap : k == 3 ? 0 : rnd_in(0, t.cap));
                t.status.push_back(rnd_in(0, 15) ? 0 : rnd_in(-1, 3));
            }
            const int nf = rnd_in(0, 40);
            int at = 0;
            for (int f = 0; f < nf; ++f) {
                const int k = rnd_in(0, 19);
                int n = rnd_in(0, 4);
                int first = at;
                if (k == 0) first = rnd_in(-3, t.maxRecs + 3);               // overlapping, out of order, outside
                if (k == 1) n = rnd_in(-2, t.maxRecs + 2);
                if (k == 2) { first = 0x7FFFFFFF - rnd_in(0, 3); n = rnd_in(0, 0x7FFFFFFE); }
                const uint32_t flg = 0x60u | (rnd_in(0, 3) ? 4u : 0u) | (rnd_in(0, 2) ? 0u : 8u);
                t.frames.push_back(entry(first, n, flg, rnd_in(0, 7) ? 0 : rnd_in(1, 5), rnd_in(0, 9) ? 0 : 1));
                if (first >= 0 && n >= 0 && (int64_t)first + n <= t.maxRecs) at = first + n;
            }
            t.maxFrames = rnd_in(0, 9) ? nf : rnd_in(0, nf);
            t.infoFrames = rnd_in(0, 9) ? (nf < t.maxFrames ? nf : t.maxFrames) : rnd_in(-2, nf + 5);
            if (t.infoFrames > nf && t.maxFrames > nf) t.maxFrames = nf;     // (the table has nf entries)
            bad |= run(t, "random table", rnd_in(0, 2) ? 1 << 20 : rnd_in(1, 3), rnd_in(0, 3) ? ~0u : rnd());
        }
    }
    if (bad) return 1;
    printf("frame verify bounds: %ld tables, %ld frames, no access outside a buffer\n", g_checked, g_frames);
    return 0;
}
