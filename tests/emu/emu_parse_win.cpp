// Lane-emulation harness of the level-1 parser's candidate windows (plz4_amd/csrc/lz4_seq_device.inl): one build of the parser at a
// time (windows per lane, through the LDS scratch, through the lane exchange), then the unchanged emit stage, with the switch for
// what a lane without a candidate gets in place of a candidate window (poison / zeros) and the parser's counters.
// Test infrastructure only: built into tests/emu/_build/, never loaded by plz4_amd, not a CPU fallback.
#define PLZ4_EMU 1
#include "../../plz4_amd/csrc/lz4_device.inl"
#include "../../plz4_amd/csrc/lz4_seq_device.inl"
#include <stdlib.h>
#include <string.h>

int plz4_emu_descending = 0;

using namespace plz4;

extern "C" {

void emu_pw_set_descending(int d) { plz4_emu_descending = d; }
void emu_pw_set_poison(int p) { plz4_emu_poison = p; }
int  emu_pw_variant() { return PLZ4_PW; }

// the parser's counters (plz4_emu_cnt in lz4_seq_device.inl); reset on read
void emu_pw_counters(unsigned long long* out16)
{
    for (int i = 0; i < 16; ++i) { out16[i] = plz4_emu_cnt[i]; plz4_emu_cnt[i] = 0; }
}

// parse (build `win`: 0 per-lane windows, 1 LDS scratch, 2 lane exchange) -> sizes -> scan -> write over one block of at most 4 MiB.
// Returns the block's compressed size (0: does not fit cap); seqOut (optional, seq_capacity(n) + 1 entries) gets the records,
// *nseqOut their number.
int emu_pw_encode(const uint8_t* src, int n, uint8_t* dst, int cap, int win, uint64_t* seqOut, int* nseqOut)
{
    static thread_local uint32_t lds[kHashBytes / 4];
    static thread_local uint8_t scr[256 + 64];
    if (n < 0 || n > kSeqMaxBlock || win < 0 || win > 2) return -1;
    uint64_t* seq = (uint64_t*)malloc(((size_t)seq_capacity(n) + 1) * 8);       // + the dump entry
    int lastAnchor = 0;
    const int nseq = win == 0 ? wave_parse_l1<0>(src, n, lds, seq, &lastAnchor)
                   : win == 1 ? wave_parse_l1<1>(src, n, lds, seq, &lastAnchor, scr)
                              : wave_parse_l1<2>(src, n, lds, seq, &lastAnchor, nullptr);
    if (nseqOut) *nseqOut = nseq;
    if (seqOut) memcpy(seqOut, seq, (size_t)nseq * 8);
    const int nChunks = (nseq + kSeqChunk - 1) / kSeqChunk;
    uint32_t* cb = (uint32_t*)malloc((size_t)(nChunks + 1) * 4);
    uint32_t* co = (uint32_t*)malloc((size_t)(nChunks + 1) * 4);
    uint8_t* bk = (uint8_t*)malloc((size_t)seq_capacity(n) + 1);
    co[0] = 0;
    for (int c = 0; c < nChunks; ++c) cb[c] = seq_emit_sizes(src, seq, bk, nseq, c);
    const int total = seq_emit_scan(cb, co, nseq, lastAnchor, n, cap);
    if (total > 0) for (int c = 0; c < (nChunks ? nChunks : 1); ++c) seq_emit_write(src, n, seq, bk, nseq, lastAnchor, c, co[c], dst);
    free(seq); free(cb); free(co); free(bk);
    return total;
}

}  // extern "C"
