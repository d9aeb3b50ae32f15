// Lane-emulation harness of the few-block level-1 path (plz4_amd/csrc/lz4_fx_device.inl): the rounds of piece parses, the gather
// and the unchanged emit stage, as the kernels run them, over one block.  Also a plain restatement of liblz4's byU32 parse
// (lz4.c:1040-1300) that can be started from a saved state, to check the restart argument without the wave code.
// Test infrastructure only: built into tests/emu/_build/, never loaded by plz4_amd, not a CPU fallback.
#define PLZ4_EMU 1
#include "piece_rounds.h"
#include <stdlib.h>
#include <string.h>
#include <vector>

int plz4_emu_descending = 0;

using namespace plz4;

namespace {

// ---- the simulator: LZ4_compress_generic(noDict, byU32, accel 1) as sequences (probe position, forward length, offset) -------
uint32_t sim_hash(const uint8_t* p)
{
    uint64_t v; memcpy(&v, p, 8);
    return (uint32_t)(((v << 24) * 889523592379ull) >> (64 - 12));           // LZ4_hash5 (lz4.c:720-730), 12 bits
}
uint32_t rd32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
int common(const uint8_t* s, int a, int b, int lim) { int l = 0; while (a + l < lim && s[a + l] == s[b + l]) ++l; return l; }

struct SimState { int anchor; uint32_t tab[4096]; };

// from the block's start (st == null) or from a post-match state; stops at the first post-match state with anchor >= stopAt
// (written to out; returns 1) or at the end of the block (returns 0, *lastAnchor).  Sequences go to seq (probe position, forward
// length beyond MINMATCH, offset).
int sim_parse(const uint8_t* s, int n, const SimState* st, int stopAt, SimState* out, std::vector<uint64_t>& seq, int* lastAnchor)
{
    const int lastProbe = n - 11, matchLimit = n - 5;
    uint32_t tab[4096];
    int anchor, ip;
    bool post;
    if (!st) { for (int i = 0; i < 4096; ++i) tab[i] = 0; tab[sim_hash(s)] = 0; anchor = 0; ip = 1; post = false; }
    else { memcpy(tab, st->tab, sizeof tab); anchor = st->anchor; ip = anchor; post = true; }
    for (;;) {
        if (post) {                                                          // lz4.c:1230-1294
            if (anchor >= stopAt) { out->anchor = anchor; memcpy(out->tab, tab, sizeof tab); return 1; }
            if (ip >= lastProbe) break;
            tab[sim_hash(s + ip - 2)] = (uint32_t)(ip - 2);
            const uint32_t h = sim_hash(s + ip), m = tab[h];
            tab[h] = (uint32_t)ip;
            if (m + 65535u >= (uint32_t)ip && rd32(s + m) == rd32(s + ip)) {
                const int f = common(s, ip + 4, (int)m + 4, matchLimit);
                seq.push_back((uint64_t)ip | ((uint64_t)f << 22) | ((uint64_t)(ip - (int)m) << 44));
                ip += 4 + f; anchor = ip;
                continue;
            }
            ip++;
            post = false;
        }
        // search (lz4.c:1040-1101)
        int fwd = ip, step = 1, nb = 1 << 6, found = -1, cand = 0;
        for (;;) {
            const int cur = fwd;
            fwd += step; step = (nb++) >> 6;
            if (fwd > lastProbe) break;
            const uint32_t h = sim_hash(s + cur), m = tab[h];
            tab[h] = (uint32_t)cur;
            if (m + 65535u < (uint32_t)cur) continue;
            if (rd32(s + m) == rd32(s + cur)) { found = cur; cand = (int)m; break; }
        }
        if (found < 0) break;
        const int f = common(s, found + 4, cand + 4, matchLimit);
        seq.push_back((uint64_t)found | ((uint64_t)f << 22) | ((uint64_t)(found - cand) << 44));
        ip = found + 4 + f; anchor = ip; post = true;
    }
    *lastAnchor = anchor;
    return 0;
}

}  // namespace

extern "C" {

void emu_fx_set_descending(int d) { plz4_emu_descending = d; }

// the simulator over a whole block, unbroken (stops == 0) or chained through saved states every `stops` bytes; records to out
int emu_fx_sim(const uint8_t* src, int n, int stops, uint64_t* out, int cap, int* lastAnchor)
{
    std::vector<uint64_t> seq;
    SimState* a = (SimState*)malloc(sizeof(SimState));
    SimState* b = (SimState*)malloc(sizeof(SimState));
    int r = sim_parse(src, n, nullptr, stops > 0 ? stops : 0x7FFFFFFF, a, seq, lastAnchor);
    for (int k = 2; r == 1; ++k) { r = sim_parse(src, n, a, stops * k, b, seq, lastAnchor); SimState* t = a; a = b; b = t; }
    free(a); free(b);
    if ((int)seq.size() > cap) return -1;
    memcpy(out, seq.data(), seq.size() * 8);
    return (int)seq.size();
}

// The few-block path over one block of n (kFxMinLen <= n <= 4 MiB): the rounds over the pieces (in descending piece order when
// `order` is 1) and the gather (piece_rounds.h), then the emit stage of lz4_seq_device.inl.  Returns the block's compressed size (0: does not fit
// cap), stats[0] = rounds that parsed, [1] = pieces parsed more than once, [2] = pieces, [3] = records; seqOut (optional) gets the
// records.
int emu_fx_encode(const uint8_t* src, int n, uint8_t* dst, int cap, int pieceBytes, int warmBytes, int order, long long* stats, uint64_t* seqOut)
{
    if (n < kFxMinLen || n > kSeqMaxBlock || pieceBytes < 1024) return -1;
    static thread_local uint32_t lds[kHashBytes / 4];
    PieceEmuBlock<FxFlavour<false>> B(n, pieceBytes);
    const int rounds = B.run(FxFlavour<false>{lds, 0}, src, warmBytes, order);
    const int seqStride = seq_capacity(n) + 1;
    std::vector<uint64_t> seq((size_t)seqStride);
    SeqInfo info; info.nseq = -1; info.lastAnchor = 0;
    int chained = 0;
    if (!B.gather(seq.data(), seqStride - 1, &info, order, &chained) || info.nseq < 0) return -3;
    const int nseq = info.nseq;
    if (stats) { stats[0] = rounds; stats[1] = B.again(); stats[2] = B.P; stats[3] = nseq; }
    if (seqOut) memcpy(seqOut, seq.data(), (size_t)nseq * 8);
    const int nChunks = (nseq + kSeqChunk - 1) / kSeqChunk;
    std::vector<uint32_t> cb(nChunks + 1), co(nChunks + 1);
    std::vector<uint8_t> bk((size_t)seqStride);
    co[0] = 0;
    for (int c = 0; c < nChunks; ++c) cb[c] = seq_emit_sizes(src, seq.data(), bk.data(), nseq, c);
    const int total = seq_emit_scan(cb.data(), co.data(), nseq, info.lastAnchor, n, cap);
    if (total > 0) for (int c = 0; c < (nChunks ? nChunks : 1); ++c) seq_emit_write(src, n, seq.data(), bk.data(), nseq, info.lastAnchor, c, co[c], dst);
    return total;
}

}  // extern "C"
