// plz4hip_dev_write_frames' kernels (wave_frame_edges, wave_frame_move, wave_frame_summary) read and write nothing but what the header
// says: a program of its own for the address and undefined-behaviour sanitizers (never loaded into Python, never run on a GPU; the
// build + run line is in scripts/README.md).  recOff, frames, outRecOff, info and out are heap allocations of exactly their sizes; the
// plaintext and the body each end on the last byte of their allocation.  Poisoned: recOff where there is no block; the plaintext's
// gaps, all of it without a content checksum or without room, and every block behind a frame's first bad record; of the body all but
// the size words of records that pass the range tests and the bytes of records that are moved.  A load of anything else -- a prefetch
// included -- or a store outside an output ends the program with the sanitizer's report.  info is checked against a walk written
// here, and a stream that is written is taken apart again.
#define PLZ4_EMU 1
#include "../../plz4_amd/csrc/lz4_frame_write_device.inl"
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

constexpr int kBsz = 65536;

struct Call {
    bool bck = false, linked = false, cck = false, csize = false, hasDict = false;
    uint32_t dictId = 0;
    int64_t srcBytes = 0, stride = kBsz, bodyBytes = 0, outCap = 0;
    int k = 0, waves = 1 << 20, slices = 1;
    std::vector<uint8_t> body;                               // what lies at body: body.size() bytes (bodyBytes may say otherwise)
    std::vector<int64_t> recOff;                             // nBlocks + 1
};

// a copy of `bytes` that ends on the last byte of its allocation; allowed[j]: byte j may be read.  Poison is kept per 8 bytes as
// "the first k are addressable": of every granule the bytes up to its last allowed one stay readable.
static uint8_t* guarded_copy(const std::vector<uint8_t>& bytes, const std::vector<char>& allowed)
{
    const size_t n = bytes.size();
    uint8_t* const p = (uint8_t*)malloc(n + 1);              // (+ 1: malloc(0) may be null; the byte is poisoned like the rest)
    if (n) memcpy(p, bytes.data(), n);
    ASAN_POISON_MEMORY_REGION(p, n + 1);
    for (size_t g = 0; g < n; g += 8) {
        size_t k = 0;
        for (size_t j = g; j < g + 8 && j < n; ++j) if (allowed[j]) k = j - g + 1;
        if (k) ASAN_UNPOISON_MEMORY_REGION(p + g, k);
    }
    return p;
}

static long g_checked = 0, g_written = 0, g_status[3] = {0, 0, 0};

static int fail(const char* what, const char* why) { fprintf(stderr, "%s: %s\n", what, why); return 1; }

static int run(const Call& c, const char* what)
{
    const FrameWriteGeom g = frame_write_geom(kBsz, c.bck, c.linked, c.cck, c.csize, c.hasDict, c.dictId, c.srcBytes, c.stride, c.bodyBytes, c.k, c.outCap);
    const int n = g.nBlocks, nf = g.nFrames;
    const int64_t edge = 4 + 4 * g.bck;
    // the walk by the header's table
    const int64_t tail = n ? c.recOff[(size_t)n] : 0;
    const bool known = tail >= 0 && tail <= c.bodyBytes;
    const int64_t E = known ? (int64_t)nf * (g.H + g.T) + tail : -1;
    const bool noRoom = known && E > c.outCap;
    std::vector<char> goodRec((size_t)n, 0), wordRead((size_t)n, 0);
    int firstBad = -1;
    if (!noRoom)
        for (int i = 0; i < n; ++i) {
            const int64_t a = c.recOff[(size_t)i], b = c.recOff[(size_t)i + 1];
            bool ok = !(a < 0 || b < a || b > c.bodyBytes) && b - a >= edge;
            if (ok) {
                wordRead[(size_t)i] = 1;
                const int64_t size = (int64_t)(ld32u(c.body.data() + a) & 0x7FFFFFFFu);
                ok = size <= kBsz && size + edge == b - a;
            }
            goodRec[(size_t)i] = ok;
            if (!ok && firstBad < 0) firstBad = i;
        }
    const int status = noRoom ? kWriteNoRoom : (firstBad >= 0 || !known) ? kWriteRecord : kWriteOk;
    if (!known && firstBad < 0) return fail(what, "an unknown end without a bad record");
    // what may be read
    std::vector<char> bodyOk(c.body.size(), 0);
    for (int i = 0; i < n; ++i) {
        const int64_t a = c.recOff[(size_t)i];
        if (wordRead[(size_t)i]) for (int j = 0; j < 4; ++j) bodyOk[(size_t)a + j] = 1;
        if (goodRec[(size_t)i] && known) for (int64_t j = a; j < c.recOff[(size_t)i + 1]; ++j) bodyOk[(size_t)j] = 1;
    }
    const int64_t lastLen = n ? c.srcBytes - (int64_t)(n - 1) * kBsz : 0;
    std::vector<uint8_t> plain((size_t)(n ? (n - 1) * c.stride + lastLen : 0));
    for (auto& b : plain) b = (uint8_t)(rnd() >> 24);
    std::vector<char> plainOk(plain.size(), 0);
    if (c.cck && !noRoom)
        for (int f = 0; f < nf; ++f)
            for (int64_t i = f * g.k; i < (f + 1) * g.k && i < n && goodRec[(size_t)i]; ++i)
                for (int64_t j = 0; j < (i == n - 1 ? lastLen : kBsz); ++j) plainOk[(size_t)(i * c.stride + j)] = 1;
    uint8_t* const src = guarded_copy(plain, plainOk);
    uint8_t* const body = guarded_copy(c.body, bodyOk);
    int64_t* const recOff = (int64_t*)malloc(8 * ((size_t)n + 1));
    memcpy(recOff, c.recOff.data(), 8 * ((size_t)n + 1));
    if (!n) ASAN_POISON_MEMORY_REGION(recOff, 8);
    uint8_t* const out = (uint8_t*)malloc((size_t)c.outCap + 1);
    memset(out, 0xC7, (size_t)c.outCap + 1);
    ASAN_POISON_MEMORY_REGION(out + c.outCap, 1);
    FrameIndex* const frames = (FrameIndex*)malloc(sizeof(FrameIndex) * (size_t)nf);
    memset((void*)frames, 0xC7, sizeof(FrameIndex) * (size_t)nf);
    int64_t* const outRecOff = (int64_t*)malloc(8 * ((size_t)n + 1));
    memset(outRecOff, 0xC7, 8 * ((size_t)n + 1));
    WriteInfo* const info = (WriteInfo*)malloc(sizeof(WriteInfo));
    memset((void*)info, 0xC7, sizeof *info);

    const int64_t groups = ((int64_t)nf + 15) / 16;
    const int grid = (int)(groups < c.waves ? groups : c.waves);
    for (int w = 0; w < grid; ++w) wave_frame_edges(g, src, body, recOff, out, frames, outRecOff, w, grid);
    for (int i = 0; i < n; ++i)
        for (int wv = 0; wv < 4 * c.slices; ++wv) wave_frame_move(g, body, recOff, out, i, wv, 4 * c.slices);
    wave_frame_summary(g, recOff, frames, info);

    int bad = 0;
    if (info->end != E || info->nFrames != nf || info->nRecs != n || info->status != status || info->firstBadRec != (noRoom ? -1 : firstBad) ||
        info->reserved[0] || info->reserved[1]) {
        fprintf(stderr, "%s: info {%lld %d %d %d %d} != {%lld %d %d %d %d}\n", what, (long long)info->end, info->nFrames, info->nRecs, info->status,
                info->firstBadRec, (long long)E, nf, n, status, noRoom ? -1 : firstBad);
        bad = 1;
    }
    if (noRoom && !bad) {
        for (int64_t j = 0; j < c.outCap; ++j) if (out[j] != 0xC7) { bad = fail(what, "no room, and a byte of out was written"); break; }
        for (size_t j = 0; j < sizeof(FrameIndex) * (size_t)nf; ++j) if (((const uint8_t*)frames)[j] != 0xC7) { bad = fail(what, "no room, and the table was written"); break; }
    }
    if (status == kWriteOk && !bad) {                        // the stream, taken apart again
        int64_t at = n ? c.recOff[0] : 0;
        for (int64_t j = 0; j < at; ++j) if (out[j] != 0xC7) { bad = fail(what, "a store in front of the stream"); break; }
        for (int f = 0; f < nf && !bad; ++f) {
            const int64_t first = f * g.k, last = first + g.k < n ? first + g.k : n;
            const FrameIndex& e = frames[f];
            std::vector<uint8_t> text;
            for (int64_t i = first; i < last; ++i) text.insert(text.end(), plain.begin() + i * c.stride, plain.begin() + i * c.stride + (i == n - 1 ? lastLen : kBsz));
            const uint8_t* const h = out + at;
            if (e.hdrOff != at || e.bodyOff != at + g.H || ld32u(h) != 0x184D2204u || h[4] != g.flg || h[5] != g.bd ||
                h[g.H - 1] != (uint8_t)(plain_xxh32(h + 4, (size_t)g.H - 5) >> 8)) { bad = fail(what, "a header"); break; }
            if (c.csize && (ld64u(h + 6) != text.size() || e.contentSz != text.size())) { bad = fail(what, "a content size"); break; }
            if (c.hasDict && (ld32u(h + g.H - 5) != c.dictId || e.dictId != c.dictId)) { bad = fail(what, "a dictionary id"); break; }
            at += g.H;
            for (int64_t i = first; i < last && !bad; ++i) {
                const int64_t len = c.recOff[(size_t)i + 1] - c.recOff[(size_t)i];
                if (outRecOff[i] != at || memcmp(out + at, c.body.data() + c.recOff[(size_t)i], (size_t)len)) bad = fail(what, "a record");
                at += len;
            }
            if (bad) break;
            if (ld32u(out + at) != 0) { bad = fail(what, "an end mark"); break; }
            at += 4;
            if (c.cck) {
                const uint32_t sum = plain_xxh32(text.data(), text.size());
                if (ld32u(out + at) != sum || e.contentSum != sum) { bad = fail(what, "a content checksum"); break; }
                at += 4;
            }
            if (e.end != at || e.firstRec != first || e.nRecs != last - first || e.status != kBodyEndMark || e.bsz != kBsz || e.flags != g.flg ||
                e.blockDesc != g.bd || e.kind || e.nibble || e.reserved) { bad = fail(what, "a table entry"); break; }
        }
        if (!bad && at != E) bad = fail(what, "the stream's end");
        if (!bad && outRecOff[n] != (n ? E - g.T : 0)) bad = fail(what, "outRecOff[nBlocks]");
        for (int64_t j = E; j < c.outCap && !bad; ++j) if (out[j] != 0xC7) bad = fail(what, "a store behind the stream");
        ++g_written;
    }
    ++g_checked; ++g_status[status];
    ASAN_UNPOISON_MEMORY_REGION(src, plain.size() + 1);
    ASAN_UNPOISON_MEMORY_REGION(body, c.body.size() + 1);
    ASAN_UNPOISON_MEMORY_REGION(recOff, 8);
    ASAN_UNPOISON_MEMORY_REGION(out + c.outCap, 1);
    free(src); free(body); free(recOff); free(out); free(frames); free(outRecOff); free(info);
    return bad;
}

// n records by the rules behind `base` bytes of noise: compressed or stored size words over noise, now and then a stored one of bsz
static Call made(int n, int lastLen, bool bck, int base = 0)
{
    Call c;
    c.bck = bck;
    c.srcBytes = n ? (int64_t)(n - 1) * kBsz + lastLen : 0;
    c.body.assign((size_t)base, 0xB7);
    c.recOff.push_back(base);
    for (int i = 0; i < n; ++i) {
        const int size = rnd_in(0, 40) ? rnd_in(1, 700) : kBsz;
        const uint32_t w = (uint32_t)size | (rnd_in(0, 2) ? 0u : 0x80000000u);
        for (int j = 0; j < 4; ++j) c.body.push_back((uint8_t)(w >> 8 * j));
        for (int j = 0; j < size + (bck ? 4 : 0); ++j) c.body.push_back((uint8_t)(rnd() >> 24));
        c.recOff.push_back((int64_t)c.body.size());
    }
    c.bodyBytes = (int64_t)c.body.size();
    return c;
}
static int64_t end_of(const Call& c)
{
    const FrameWriteGeom g = frame_write_geom(kBsz, c.bck, c.linked, c.cck, c.csize, c.hasDict, c.dictId, c.srcBytes, c.stride, c.bodyBytes, c.k, 0);
    return (int64_t)((uint64_t)((int64_t)g.nFrames * (g.H + g.T)) + (uint64_t)(g.nBlocks ? c.recOff[(size_t)g.nBlocks] : 0));   // (it may hold anything)
}

int main()
{
    static const int64_t kHostile[] = {-1, -5, INT64_MIN, INT64_MAX, INT64_MAX - 3, (int64_t)1 << 62, (int64_t)1 << 32, 0, 3, -((int64_t)1 << 40)};
    int bad = 0;
    for (int desc = 0; desc < 2 && !bad; ++desc) {
        plz4_emu_descending = desc;
        // 1. by the rules: every option, frame sizes, last blocks, both strides, exactly enough room
        for (int o = 0; o < 32 && !bad; ++o)
            for (int k = 0; k < 4 && !bad; ++k) {
                if ((o & 16) && k) continue;
                static const int kLast[] = {1, 15, 16, 17, 4096 + 5, kBsz};
                const int n = (o + k) % 6;
                Call c = made(n, kLast[(o + 3 * k) % 6], o & 1, (o & 2) ? 5 : 0);
                c.cck = o & 2; c.csize = o & 4; c.hasDict = o & 8; c.linked = o & 16; c.dictId = 0xA1B2C3D4u + (uint32_t)o; c.k = k;
                if (k & 1) c.stride = kBsz + 65536 + 8 * (o % 3);
                c.slices = 1 + o % 3;
                c.outCap = end_of(c);
                bad |= run(c, "by the rules");
            }
        // 2. hostile tables on one body: every entry in turn set to every hostile value and to its neighbours' values +- 1
        for (int k = 0; k < 3 && !bad; ++k)
            for (int at = 0; at <= 5 && !bad; ++at) {
                Call base = made(5, 777, true);
                base.cck = true; base.csize = true; base.k = k;
                base.outCap = end_of(base) + 64;
                for (int64_t v : kHostile) { Call c = base; c.recOff[(size_t)at] = v; bad |= run(c, "a hostile offset"); }
                for (int d = -9; d <= 9 && !bad; d += 3) {
                    Call c = base; c.recOff[(size_t)at] = base.recOff[(size_t)(at ? at - 1 : 1)] + d; bad |= run(c, "an offset beside its neighbour");
                    c = base; c.recOff[(size_t)at] += d; bad |= run(c, "an offset moved");
                }
                Call c = base; c.bodyBytes = base.recOff[(size_t)at]; c.body.resize((size_t)c.bodyBytes); bad |= run(c, "a body that ends early");
                c = base; c.bodyBytes = base.recOff[(size_t)at] + 3; c.body.resize((size_t)c.bodyBytes); bad |= run(c, "a body that ends inside a size word");
                c = base; c.outCap = base.recOff[(size_t)at]; bad |= run(c, "no room");
            }
        // 3. random tables
        for (int round = 0; round < 1500 && !bad; ++round) {
            Call c = made(rnd_in(0, 6), rnd_in(0, 3) ? rnd_in(1, 600) : rnd_in(1, kBsz), rnd_in(0, 1), rnd_in(0, 3) ? 0 : rnd_in(1, 40));
            c.cck = rnd_in(0, 2); c.csize = rnd_in(0, 1); c.hasDict = rnd_in(0, 1); c.dictId = rnd();
            c.k = rnd_in(0, 3); c.linked = !c.k && rnd_in(0, 1);
            if (rnd_in(0, 1)) c.stride = kBsz + 65536 + 8 * rnd_in(0, 4);
            c.waves = rnd_in(0, 1) ? 1 << 20 : 1; c.slices = rnd_in(1, 3);
            const int n = (int)c.recOff.size() - 1;
            for (int m = rnd_in(0, 3) ? 0 : rnd_in(1, 3); m > 0 && n; --m) {
                const int i = rnd_in(0, n), how = rnd_in(0, 5);
                if (how == 0) c.recOff[(size_t)i] = kHostile[rnd_in(0, 9)];
                if (how == 1) c.recOff[(size_t)i] = (int64_t)((uint64_t)c.recOff[(size_t)i] + (uint64_t)(int64_t)rnd_in(-9, 9));
                if (how == 2) c.recOff[(size_t)i] = c.recOff[(size_t)rnd_in(0, n)];
                if (how == 3 && i < n && c.recOff[(size_t)i] >= 0 && c.recOff[(size_t)i] + 4 <= (int64_t)c.body.size()) { const uint32_t w = rnd_in(0, 1) ? (uint32_t)kBsz + 1u + (rnd() & 0x80000000u) : rnd(); for (int j = 0; j < 4; ++j) c.body[(size_t)c.recOff[(size_t)i] + j] = (uint8_t)(w >> 8 * j); }
                if (how == 4) { c.bodyBytes = rnd_in(0, (int)c.body.size()); c.body.resize((size_t)c.bodyBytes); }
                if (how == 5) c.bck = !c.bck;
            }
            const int64_t e = end_of(c);
            const int room = rnd_in(0, 5);
            c.outCap = room == 0 ? 0 : room == 1 && e > 0 && e < (1 << 24) ? e - 1 : room == 2 ? rnd_in(0, 2000) : e >= 0 && e < (1 << 24) ? e + rnd_in(0, 1) * 50 : 4096;
            bad |= run(c, "random table");
        }
    }
    if (bad) return 1;
    printf("frame write bounds: %ld calls (%ld ok, %ld no room, %ld bad records), %ld streams taken apart, no access outside a buffer\n", g_checked,
           g_status[0], g_status[1], g_status[2], g_written);
    return 0;
}
