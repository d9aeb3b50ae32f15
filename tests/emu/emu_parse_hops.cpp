// Lane-emulation harness of the grid batch's scalar hop (plz4_amd/csrc/lz4_seq_device.inl, PLZ4_HOP): one build of the parser at a time
// (windows per lane, through the LDS scratch, through the lane exchange), then the unchanged emit stage, with the parser's records,
// all of its counters and the number of batches by how many matches their first walk executed.
// Test infrastructure only: built into tests/emu/_build/, never loaded by plz4_amd, not a CPU fallback.
#define PLZ4_EMU 1
#include "../../plz4_amd/csrc/lz4_device.inl"
#include "../../plz4_amd/csrc/lz4_seq_device.inl"
#include <stdlib.h>
#include <string.h>
#include <vector>

int plz4_emu_descending = 0;

using namespace plz4;

extern "C" {

void emu_ph_set_descending(int d) { plz4_emu_descending = d; }
void emu_ph_set_poison(int p) { plz4_emu_poison = p; }
int  emu_ph_variant() { return PLZ4_HOP; }
int  emu_ph_hops() { return kHopN; }                 // unconditional hops of a batch's first walk

// the parser's counters (plz4_emu_cnt, 32) and the batches by executed matches (plz4_emu_hops, 18); reset on read
void emu_ph_counters(unsigned long long* cnt32, unsigned long long* hops18)
{
    for (int i = 0; i < 32; ++i) { cnt32[i] = plz4_emu_cnt[i]; plz4_emu_cnt[i] = 0; }
    for (int i = 0; i < 18; ++i) { hops18[i] = plz4_emu_hops[i]; plz4_emu_hops[i] = 0; }
}

// parse (build `win`: 0 per-lane windows, 1 LDS scratch, 2 lane exchange) -> sizes -> scan -> write over one block of at most 4 MiB.
// Returns the block's compressed size (0: does not fit cap); seqOut (optional, seq_capacity(n) + 1 entries) gets the records,
// *nseqOut their number.
int emu_ph_encode(const uint8_t* src, int n, uint8_t* dst, int cap, int win, uint64_t* seqOut, int* nseqOut)
{
    static thread_local uint32_t lds[kHashBytes / 4];
    static thread_local uint8_t scr[256 + 64];
    if (n < 0 || n > kSeqMaxBlock || win < 0 || win > 2) return -1;
    std::vector<uint64_t> seq((size_t)seq_capacity(n) + 1);                     // + the dump entry
    int lastAnchor = 0;
    const int nseq = win == 0 ? wave_parse_l1<0>(src, n, lds, seq.data(), &lastAnchor)
                   : win == 1 ? wave_parse_l1<1>(src, n, lds, seq.data(), &lastAnchor, scr)
                              : wave_parse_l1<2>(src, n, lds, seq.data(), &lastAnchor, nullptr);
    if (nseqOut) *nseqOut = nseq;
    if (seqOut) memcpy(seqOut, seq.data(), (size_t)nseq * 8);
    const int nChunks = (nseq + kSeqChunk - 1) / kSeqChunk;
    std::vector<uint32_t> cb(nChunks + 1), co(nChunks + 1);
    std::vector<uint8_t> bk((size_t)seq_capacity(n) + 1);
    co[0] = 0;
    for (int c = 0; c < nChunks; ++c) cb[c] = seq_emit_sizes(src, seq.data(), bk.data(), nseq, c);
    const int total = seq_emit_scan(cb.data(), co.data(), nseq, lastAnchor, n, cap);
    if (total > 0) for (int c = 0; c < (nChunks ? nChunks : 1); ++c) seq_emit_write(src, n, seq.data(), bk.data(), nseq, lastAnchor, c, co[c], dst);
    return total;
}

}  // extern "C"
