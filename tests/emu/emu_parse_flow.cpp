// Lane-emulation harness of the level-1 parser's control flow (plz4_amd/csrc/lz4_seq_device.inl, lz4_fx_device.inl): the parser of a
// whole block in its three window forms and the parser of pieces (kPiece), each followed by the unchanged emit stage, with all of
// the parser's counters -- among them how the grid batches left the steady state.
// Test infrastructure only: built into tests/emu/_build/, never loaded by plz4_amd, not a CPU fallback.
#define PLZ4_EMU 1
#include "piece_rounds.h"
#include <stdlib.h>
#include <string.h>
#include <vector>

int plz4_emu_descending = 0;

using namespace plz4;

namespace {

int emit(const uint8_t* src, int n, const uint64_t* seq, int nseq, int lastAnchor, uint8_t* dst, int cap)
{
    const int nChunks = (nseq + kSeqChunk - 1) / kSeqChunk;
    std::vector<uint32_t> cb(nChunks + 1), co(nChunks + 1);
    std::vector<uint8_t> bk((size_t)seq_capacity(n) + 1);
    co[0] = 0;
    for (int c = 0; c < nChunks; ++c) cb[c] = seq_emit_sizes(src, seq, bk.data(), nseq, c);
    const int total = seq_emit_scan(cb.data(), co.data(), nseq, lastAnchor, n, cap);
    if (total > 0) for (int c = 0; c < (nChunks ? nChunks : 1); ++c) seq_emit_write(src, n, seq, bk.data(), nseq, lastAnchor, c, co[c], dst);
    return total;
}

}  // namespace

extern "C" {

void emu_pf_set_descending(int d) { plz4_emu_descending = d; }
void emu_pf_set_poison(int p) { plz4_emu_poison = p; }
int  emu_pf_slots() { return (int)(sizeof(plz4_emu_cnt) / sizeof(plz4_emu_cnt[0])); }

// the parser's counters (plz4_emu_cnt in lz4_seq_device.inl); reset on read
void emu_pf_counters(unsigned long long* out)
{
    for (int i = 0; i < emu_pf_slots(); ++i) { out[i] = plz4_emu_cnt[i]; plz4_emu_cnt[i] = 0; }
}

// one block of at most 4 MiB: parse (win: 0 per-lane windows, 1 LDS scratch, 2 lane exchange) -> emit.  Returns the compressed size
// (0: does not fit cap).
int emu_pf_encode(const uint8_t* src, int n, uint8_t* dst, int cap, int win)
{
    static thread_local uint32_t lds[kHashBytes / 4];
    static thread_local uint8_t scr[256 + 64];
    if (n < 0 || n > kSeqMaxBlock || win < 0 || win > 2) return -1;
    std::vector<uint64_t> seq((size_t)seq_capacity(n) + 1);                     // + the dump entry
    int lastAnchor = 0;
    const int nseq = win == 0 ? wave_parse_l1<0>(src, n, lds, seq.data(), &lastAnchor)
                   : win == 1 ? wave_parse_l1<1>(src, n, lds, seq.data(), &lastAnchor, scr)
                              : wave_parse_l1<2>(src, n, lds, seq.data(), &lastAnchor, nullptr);
    return emit(src, n, seq.data(), nseq, lastAnchor, dst, cap);
}

// one block of kFxMinLen..4 MiB through the pieces' parser: the rounds and the gather (piece_rounds.h), emit.  *rounds <- rounds that parsed.
int emu_pf_fx_encode(const uint8_t* src, int n, uint8_t* dst, int cap, int pieceBytes, int warmBytes, int* rounds)
{
    if (n < kFxMinLen || n > kSeqMaxBlock || pieceBytes < 1024) return -1;
    static thread_local uint32_t lds[kHashBytes / 4];
    PieceEmuBlock<FxFlavour<false>> B(n, pieceBytes);
    const int last = B.run(FxFlavour<false>{lds, 0}, src, warmBytes, 0);
    if (rounds) *rounds = last;
    const int seqStride = seq_capacity(n) + 1;
    std::vector<uint64_t> seq((size_t)seqStride);
    SeqInfo info; info.nseq = -1; info.lastAnchor = 0;
    int chained = 0;
    if (!B.gather(seq.data(), seqStride - 1, &info, 0, &chained) || info.nseq < 0) return -3;
    return emit(src, n, seq.data(), info.nseq, info.lastAnchor, dst, cap);
}

}  // extern "C"
