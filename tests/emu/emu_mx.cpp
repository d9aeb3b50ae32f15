// Lane-emulation harness of the few-block level-2 path (plz4_amd/csrc/lz4_mx_device.inl): the rounds of piece walks, the gather and
// the unchanged emit stage, as the kernels run them, over one block; the unbroken hc_mid_parse beside it; the walk restarted from
// every saved boundary state; the path's layout and route functions.
// Test infrastructure only: built into tests/emu/_build/, never loaded by plz4_amd, not a CPU fallback.
#define PLZ4_EMU 1
#include "piece_rounds.h"
#include "../../plz4_amd/csrc/route.h"
#include <string.h>
#include <string>

int plz4_emu_descending = 0;

using namespace plz4;

extern "C" {

void emu_mx_set_descending(int d) { plz4_emu_descending = d; }

// the unbroken walk: records to out (room for n / 4 + 64), returns their number
int emu_mx_whole(const uint8_t* src, int n, uint64_t* out, int* lastAnchor)
{
    std::vector<uint8_t> padded((size_t)n + 64, 0);
    if (n > 0) memcpy(padded.data(), src, (size_t)n);
    std::vector<uint32_t> tabs(kMxTab);
    return hc_mid_parse(padded.data(), n, tabs.data(), tabs.data() + 16384, out, lastAnchor);
}

// The few-block path over one block of 0 <= n <= 4 MiB (piece_rounds.h), then the emit stage of lz4_seq_device.inl.  Returns the
// block's compressed size (0: does not fit cap), stats[0] = rounds that walked, [1] = pieces walked more than once, [2] = pieces,
// [3] = records, [4] = pieces in the chain, [5] = bytes walked in all rounds; seqOut (optional) gets the records.
int emu_mx_encode(const uint8_t* src, int n, uint8_t* dst, int cap, int pieceBytes, int warmBytes, int order, long long* stats, uint64_t* seqOut)
{
    if (n < 0 || n > kSeqMaxBlock || pieceBytes < 1024) return -1;
    std::vector<uint8_t> padded((size_t)n + 64, 0);
    if (n > 0) memcpy(padded.data(), src, (size_t)n);
    PieceEmuBlock<MxFlavour> B(n, pieceBytes);
    const int rounds = B.run(MxFlavour{}, padded.data(), warmBytes, order);
    const int seqStride = seq_capacity(n) + 1;
    std::vector<uint64_t> seq((size_t)seqStride);
    SeqInfo info; info.nseq = -1; info.lastAnchor = 0;
    int chained = 0;
    if (!B.gather(seq.data(), seqStride - 1, &info, order, &chained) || info.nseq < 0) return -3;
    if (stats) { stats[0] = rounds; stats[1] = B.again(); stats[2] = B.P; stats[3] = info.nseq; stats[4] = chained; stats[5] = B.walked; }
    if (seqOut) memcpy(seqOut, seq.data(), (size_t)info.nseq * 8);
    const int nseq = info.nseq, nChunks = (nseq + kSeqChunk - 1) / kSeqChunk;
    std::vector<uint32_t> cb(nChunks + 1), co(nChunks + 1);
    co[0] = 0;
    for (int c = 0; c < nChunks; ++c) cb[c] = seq_emit_sizes<false>(padded.data(), seq.data(), nullptr, nseq, c);
    const int total = seq_emit_scan(cb.data(), co.data(), nseq, info.lastAnchor, n, cap);
    if (total > 0) for (int c = 0; c < (nChunks ? nChunks : 1); ++c) seq_emit_write<false>(padded.data(), n, seq.data(), nullptr, nseq, info.lastAnchor, c, co[c], dst);
    return total;
}

// Restart exactness: the block is walked once, stopping at the first post-match state at or beyond every multiple of `stops`; from
// every state saved that way a fresh walk to the block's end must give the records the unbroken walk gives from that anchor on.
// Returns the states tried (< 0: the first one that failed, counted from -1).
int emu_mx_restart(const uint8_t* src, int n, int stops)
{
    std::vector<uint8_t> padded((size_t)n + 64, 0);
    if (n > 0) memcpy(padded.data(), src, (size_t)n);
    const size_t room = (size_t)n / 4 + 64;
    std::vector<uint64_t> whole(room), part(room);
    int la = 0;
    std::vector<uint32_t> tabs(kMxTab), saved(kMxTab);
    const int nw = hc_mid_parse(padded.data(), n, tabs.data(), tabs.data() + 16384, whole.data(), &la);
    int tried = 0, anchor = -1;
    for (int stop = stops; stop < n; stop += stops) {
        if (anchor >= stop) continue;                                       // (the state saved last lies behind this boundary too)
        // the chain so far: from the state saved last (or the block's start) to the next boundary
        MidRun run;
        run.entryAnchor = anchor; run.primed = anchor >= 0; run.cp = -1; run.cpTab = nullptr; run.cpAnchor = -1;
        run.end = stop; run.outAnchor = -1; run.seqCap = (int)room - 1; run.fin = 0; run.over = 0;
        if (anchor >= 0) memcpy(tabs.data(), saved.data(), kMxTab * 4);
        int la2 = 0;
        hc_mid_parse<false, uint32_t*, MidNoCtx, true>(padded.data(), n, tabs.data(), tabs.data() + 16384, part.data(), &la2, 0, MidNoCtx(), &run);
        if (run.fin || run.over) break;
        anchor = run.outAnchor;
        memcpy(saved.data(), tabs.data(), kMxTab * 4);
        // a fresh walk from it to the block's end
        MidRun rest = run;
        rest.entryAnchor = anchor; rest.primed = 1; rest.end = n; rest.outAnchor = -1; rest.fin = 0;
        int la3 = 0;
        const int nr = hc_mid_parse<false, uint32_t*, MidNoCtx, true>(padded.data(), n, tabs.data(), tabs.data() + 16384, part.data(), &la3, 0, MidNoCtx(), &rest);
        ++tried;
        int first = 0;
        while (first < nw && (int)seq_pos(whole[first]) < anchor) ++first;
        if (!rest.fin || la3 != la || nr != nw - first || memcmp(part.data(), whole.data() + first, (size_t)nr * 8) != 0) return -tried;
    }
    return tried;
}

// piece_layout of the level-2 flavour: out = offMeta, offIn, offOut, offRec, total, then per take (off, bytes); returns the takes
int emu_mx_layout(int per, int P, int recStride, long long* out, int cap)
{
    std::vector<WsTake> log;
    const PieceLayout L = piece_layout(per, P, recStride, kMxTab, false, &log);
    long long v[5] = {(long long)L.offMeta, (long long)L.offIn, (long long)L.offOut, (long long)L.offRec, (long long)L.total};
    int at = 0;
    for (int i = 0; i < 5 && at < cap; ++i) out[at++] = v[i];
    for (const WsTake& t : log) { if (at + 2 > cap) break; out[at++] = (long long)t.off; out[at++] = (long long)(t.count * t.size); }
    return (int)log.size();
}

// mx_want + mx_route under an environment given as "NAME=value\n" lines: out = mx, piece, warm, P, route(staged, mx granted),
// route(staged refused), route(mx refused)
void emu_mx_route(const char* env, int level, int nb, int maxLen, int hcEx, int rider, int* out)
{
    const std::string e(env ? env : "");
    static thread_local std::string val;
    const auto get = [&](const char* name) -> const char* {
        const std::string key = std::string(name) + "=";
        size_t at = 0;
        while (at < e.size()) {
            size_t nl = e.find('\n', at); if (nl == std::string::npos) nl = e.size();
            if (e.compare(at, key.size(), key) == 0) { val = e.substr(at + key.size(), nl - at - key.size()); return val.c_str(); }
            at = nl + 1;
        }
        return nullptr;
    };
    const MxSwitches sw = parse_mx_switches(get);
    const MxWant w = mx_want(MxShape{level, nb, maxLen, hcEx != 0, rider != 0}, sw);
    out[0] = w.mx; out[1] = w.piece; out[2] = w.warm; out[3] = w.P;
    out[4] = mx_route(w, true, true); out[5] = mx_route(w, false, true); out[6] = mx_route(w, true, false);
}

}  // extern "C"
