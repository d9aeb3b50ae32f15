// Lane-emulation harness of the few-block level-1 path for blocks with history outside the block (the kExt flavour of
// plz4_amd/csrc/lz4_fx_device.inl): fxl_prep, the rounds of piece parses and the gather (piece_rounds.h) and the emit stage with the
// segment's catch-up room, as the kernels run them, over one block; a block that is not the path's (<= 4 KiB under a dictionary context) gets the empty
// parse and then wave_encode_block_dict, as k_fxl_small does it.
// Test infrastructure only: built into tests/emu/_build/, never loaded by plz4_amd, not a CPU fallback.
#define PLZ4_EMU 1
#include "piece_rounds.h"
#include <stdlib.h>
#include <string.h>
#include <vector>

int plz4_emu_descending = 0;

using namespace plz4;

extern "C" {

void emu_fxl_set_descending(int d) { plz4_emu_descending = d; }

// One block of n bytes under `mode` (kDict*: 0 fresh prefix, 1 LZ4_loadDict(seg), 2 / 3 dictionary context, 4 a dropped dictionary);
// seg / segLen: the previous block's tail or the last <= 64 KiB of the dictionary, dictTable: the context's table (liblz4 indices).
// Returns the block's compressed size (0: does not fit cap); stats[0] = rounds that parsed, [1] = pieces parsed more than once,
// [2] = pieces, [3] = records, [4] = 1 when the block took the path.
int emu_fxl_encode(const uint8_t* src, int n, const uint8_t* seg, int segLen, int mode, const uint32_t* dictTable, uint8_t* dst, int cap,
                   int pieceBytes, int warmBytes, int order, long long* stats)
{
    if (n < 0 || n > kSeqMaxBlock || pieceBytes < 1024 || segLen < 0 || segLen > 65536) return -1;
    static thread_local uint32_t lds[kHashBytes / 4];
    // the staging layout: 64 KiB of room in front of the block (poisoned: nothing below the segment may matter)
    std::vector<uint8_t> buf((size_t)65536 + n + 256);
    memset(buf.data(), 0xA7, buf.size());
    uint8_t* const blk = buf.data() + 65536;
    if (n) memcpy(blk, src, (size_t)n);
    PieceEmuBlock<FxFlavour<true>> B(n, pieceBytes, -1, true);
    const FxlBlk xb = *B.xb = fxl_prep(blk, n, mode, seg, segLen, dictTable, B.tabIn, lds);
    const int seqStride = seq_capacity(n) + 1;
    std::vector<uint64_t> seq((size_t)seqStride);
    SeqInfo info; info.nseq = -1; info.lastAnchor = 0;
    int rounds = 0;
    long long again = 0;
    if (xb.pfx < 0) { info.nseq = 0; info.lastAnchor = 0; }
    else {
        rounds = B.run(FxFlavour<true>{lds, xb.bs}, blk, warmBytes, order);
        int chained = 0;
        if (!B.gather(seq.data(), seqStride - 1, &info, order, &chained) || info.nseq < 0) return -3;
        again = B.again();
    }
    const int nseq = info.nseq, pfx = xb.pfx < 0 ? 0 : xb.pfx;
    if (stats) { stats[0] = rounds; stats[1] = again; stats[2] = B.P; stats[3] = nseq; stats[4] = xb.pfx >= 0; }
    const int nChunks = (nseq + kSeqChunk - 1) / kSeqChunk;
    std::vector<uint32_t> cb(nChunks + 1), co(nChunks + 1);
    std::vector<uint8_t> bk((size_t)seqStride);
    co[0] = 0;
    for (int c = 0; c < nChunks; ++c) cb[c] = seq_emit_sizes<true, true>(blk, seq.data(), bk.data(), nseq, c, pfx);
    int total = seq_emit_scan(cb.data(), co.data(), nseq, info.lastAnchor, n, cap);
    if (total > 0) for (int c = 0; c < (nChunks ? nChunks : 1); ++c) seq_emit_write<true, true>(blk, n, seq.data(), bk.data(), nseq, info.lastAnchor, c, co[c], dst, pfx);
    if (xb.pfx < 0) {
        const DictEnc dc{seg, segLen, mode, dictTable};
        total = wave_encode_block_dict(blk, n, dst, cap, dc, lds);
    }
    return total;
}

}  // extern "C"
