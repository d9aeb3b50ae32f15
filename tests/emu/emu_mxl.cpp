// Lane-emulation harness of the few-block level-2 path on a block with history outside the block (MxlFlavour,
// plz4_amd/csrc/lz4_mx_device.inl): the rounds of piece walks behind an external segment, the gather and the unchanged emit stage, as
// the kernels run them, over one block; the unbroken hc_mid_parse<true> beside it; the walk restarted from every saved boundary
// state; the path's route function.
// Test infrastructure only: built into tests/emu/_build/, never loaded by plz4_amd, not a CPU fallback.
#define PLZ4_EMU 1
#include "piece_rounds.h"
#include "../../plz4_amd/csrc/route.h"
#include <string.h>
#include <string>

int plz4_emu_descending = 0;

using namespace plz4;

namespace {

// segment + block + 64 bytes of slack, as one buffer; the block starts at segLen
std::vector<uint8_t> laid_out(const uint8_t* seg, int segLen, const uint8_t* src, int n)
{
    std::vector<uint8_t> cat((size_t)segLen + (size_t)n + 64, 0);
    if (segLen > 0) memcpy(cat.data(), seg, (size_t)segLen);
    if (n > 0) memcpy(cat.data() + segLen, src, (size_t)n);
    return cat;
}

}  // namespace

extern "C" {

void emu_mxl_set_descending(int d) { plz4_emu_descending = d; }

// the unbroken walk behind the segment: records (block-relative) to out (room for n / 4 + 64), returns their number
int emu_mxl_whole(const uint8_t* seg, int segLen, const uint8_t* src, int n, uint64_t* out, int* lastAnchor)
{
    std::vector<uint8_t> cat = laid_out(seg, segLen, src, n);
    std::vector<uint32_t> tabs(kMxTab);
    return hc_mid_parse<true>(cat.data() + segLen, n, tabs.data(), tabs.data() + 16384, out, lastAnchor, segLen);
}

// The few-block path over one block of 0 <= n <= 4 MiB behind a segment of 0 <= segLen <= 64 KiB (piece_rounds.h), then the emit
// stage of lz4_seq_device.inl.  Returns the block's compressed size (0: does not fit cap), stats[0] = rounds that walked, [1] =
// pieces walked more than once, [2] = pieces, [3] = records, [4] = pieces in the chain, [5] = bytes walked in all rounds; seqOut
// (optional) gets the records.
int emu_mxl_encode(const uint8_t* seg, int segLen, const uint8_t* src, int n, uint8_t* dst, int cap, int pieceBytes, int warmBytes, int order,
                   long long* stats, uint64_t* seqOut)
{
    if (n < 0 || n > kSeqMaxBlock || segLen < 0 || segLen > 65536 || pieceBytes < 1024) return -1;
    std::vector<uint8_t> cat = laid_out(seg, segLen, src, n);
    const uint8_t* const blk = cat.data() + segLen;
    PieceEmuBlock<MxlFlavour> B(n, pieceBytes);
    const int rounds = B.run(MxlFlavour(segLen), blk, warmBytes, order);
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
    for (int c = 0; c < nChunks; ++c) cb[c] = seq_emit_sizes<false>(blk, seq.data(), nullptr, nseq, c);
    const int total = seq_emit_scan(cb.data(), co.data(), nseq, info.lastAnchor, n, cap);
    if (total > 0) for (int c = 0; c < (nChunks ? nChunks : 1); ++c) seq_emit_write<false>(blk, n, seq.data(), nullptr, nseq, info.lastAnchor, c, co[c], dst);
    return total;
}

// Restart exactness behind a segment: the block is walked once, stopping at the first post-match state at or beyond every multiple
// of `stops`; from every state saved that way a fresh walk to the block's end must give the records the unbroken hc_mid_parse<true>
// gives from that anchor on.  Returns the states tried (< 0: the first one that failed, counted from -1).
int emu_mxl_restart(const uint8_t* seg, int segLen, const uint8_t* src, int n, int stops)
{
    std::vector<uint8_t> cat = laid_out(seg, segLen, src, n);
    const uint8_t* const blk = cat.data() + segLen;
    const size_t room = (size_t)n / 4 + 64;
    std::vector<uint64_t> whole(room), part(room);
    int la = 0;
    std::vector<uint32_t> tabs(kMxTab), saved(kMxTab);
    const int nw = hc_mid_parse<true>(blk, n, tabs.data(), tabs.data() + 16384, whole.data(), &la, segLen);
    int tried = 0, anchor = -1;                                             // (the parser's coordinates: the block starts at segLen)
    for (int stop = stops; stop < n; stop += stops) {
        if (anchor >= segLen + stop) continue;                              // (the state saved last lies behind this boundary too)
        MidRun run;
        run.entryAnchor = anchor; run.primed = anchor >= 0; run.cp = -1; run.cpTab = nullptr; run.cpAnchor = -1;
        run.end = segLen + stop; run.outAnchor = -1; run.seqCap = (int)room - 1; run.fin = 0; run.over = 0;
        if (anchor >= 0) memcpy(tabs.data(), saved.data(), kMxTab * 4);
        int la2 = 0;
        hc_mid_parse<true, uint32_t*, MidNoCtx, true>(blk, n, tabs.data(), tabs.data() + 16384, part.data(), &la2, segLen, MidNoCtx(), &run);
        if (run.fin || run.over) break;
        anchor = run.outAnchor;
        memcpy(saved.data(), tabs.data(), kMxTab * 4);
        MidRun rest = run;
        rest.entryAnchor = anchor; rest.primed = 1; rest.end = segLen + n; rest.outAnchor = -1; rest.fin = 0;
        int la3 = 0;
        const int nr = hc_mid_parse<true, uint32_t*, MidNoCtx, true>(blk, n, tabs.data(), tabs.data() + 16384, part.data(), &la3, segLen, MidNoCtx(), &rest);
        ++tried;
        int first = 0;
        while (first < nw && (int)seq_pos(whole[first]) < anchor - segLen) ++first;
        if (!rest.fin || la3 != la || nr != nw - first || memcmp(part.data(), whole.data() + first, (size_t)nr * 8) != 0) return -tried;
    }
    return tried;
}

// mxl_want + mx_route under an environment given as "NAME=value\n" lines: out = mxl, piece, warm, P, route(staged, pieces granted),
// route(staged refused), route(pieces refused), and what mx_want says to the same call
void emu_mxl_route(const char* env, int level, int nb, int maxLen, int hcEx, int rider, int* out)
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
    const MxShape shape{level, nb, maxLen, hcEx != 0, rider != 0};
    const MxWant w = mxl_want(shape, sw);
    out[0] = w.mx; out[1] = w.piece; out[2] = w.warm; out[3] = w.P;
    out[4] = mx_route(w, true, true); out[5] = mx_route(w, false, true); out[6] = mx_route(w, true, false);
    out[7] = mx_want(shape, sw).mx;
    out[8] = kMxlMaxBlocks;
}

}  // extern "C"
