// Lane-emulation harness of the bulk level-1 path for blocks with history outside the block (k_l1x_parse of plz4hip.hip: l1x_block
// of plz4_amd/csrc/lz4_fx_device.inl -- the segment in place or laid in front of the block, the starting table built in the wave's
// own table, one exact whole-block run of the kExt parse -- then the kSeg emit stage) over a linked call on CONTIGUOUS plaintext, as
// plz4hip_dev_encode_records_ex runs it; a block that is not the path's (<= 4 KiB under a dictionary context) gets
// wave_encode_block_dict, as k_fxl_small does it.
// Test infrastructure only: built into tests/emu/_build/, never loaded by plz4_amd, not a CPU fallback.
#define PLZ4_EMU 1
#include "../../plz4_amd/csrc/lz4_fx_device.inl"
#include "../../plz4_amd/csrc/lz4_block_io.inl"
#include <stdlib.h>
#include <string.h>
#include <vector>

int plz4_emu_descending = 0;

using namespace plz4;

extern "C" {

void emu_l1x_set_descending(int d) { plz4_emu_descending = d; }

// src: block 0 of srcBytes bytes of contiguous plaintext in blocks of bsz, 64 KiB of writable scratch in front of it.  How block i is
// primed is the kernels' own rule (hist_of + l1_prime, lz4_block_io.inl): after block i - 1's last <= 64 KiB, block 0 after prevTail
// (prevTailLen >= 0), else under the dictionary context (hasDict; dict / dictLen: its last <= 64 KiB, dictTable: its table), else
// a linked frame's first block.  Block i's compressed bytes go to dst + i * dstStride (capacity bsz), its size (0: does not fit)
// to result[i].  order: 0 first block first, 1 last block first.  Returns 0, or a negative number when a block's run failed.
int emu_l1x_encode(uint8_t* src, long long srcBytes, int bsz, const uint8_t* dict, int dictLen, const uint32_t* dictTable, int hasDict,
                   const uint8_t* prevTail, int prevTailLen, uint8_t* dst, long long dstStride, int* result, int order)
{
    if (bsz <= 0 || bsz > kSeqMaxBlock || srcBytes < 0 || prevTailLen > 65536) return -1;
    static thread_local uint32_t lds[kHashBytes / 4];
    const int nb = (int)((srcBytes + bsz - 1) / bsz);
    const int seqStride = seq_capacity(bsz) + 1;
    std::vector<uint64_t> seq((size_t)seqStride);
    std::vector<uint8_t> bk((size_t)seqStride);
    const HistView view{src, bsz, nullptr, srcBytes, bsz, 1, prevTail, prevTailLen, hasDict ? dict : nullptr, hasDict ? dictLen : -1};
    for (int j = 0; j < nb; ++j) {
        const int i = order ? nb - 1 - j : j;
        const long long rem = srcBytes - (long long)i * bsz;
        const int n = (int)(rem < bsz ? rem : bsz);
        uint8_t* const blk = src + (long long)i * bsz;
        const DictEnc dc = l1_prime(hist_of(view, i, n, false), false, dictTable);
        int lastAnchor = 0;
        FxlBlk xb;
        const int nseq = l1x_block(blk, n, dc.mode, dc.dict, dc.dictSize, dc.dictTable, seq.data(), seqStride - 1, &lastAnchor, &xb, lds);
        if (nseq < 0) return -2;
        uint8_t* const out = dst + (long long)i * dstStride;
        int total;
        if (xb.pfx < 0) total = wave_encode_block_dict(blk, n, out, bsz, dc, lds);
        else {
            const int nChunks = (nseq + kSeqChunk - 1) / kSeqChunk;
            std::vector<uint32_t> cb(nChunks + 1), co(nChunks + 1);
            co[0] = 0;
            for (int c = 0; c < nChunks; ++c) cb[c] = seq_emit_sizes<true, true>(blk, seq.data(), bk.data(), nseq, c, xb.pfx);
            total = seq_emit_scan(cb.data(), co.data(), nseq, lastAnchor, n, bsz);
            if (total > 0) for (int c = 0; c < (nChunks ? nChunks : 1); ++c) seq_emit_write<true, true>(blk, n, seq.data(), bk.data(), nseq, lastAnchor, c, co[c], out, xb.pfx);
        }
        result[i] = total;
    }
    return 0;
}

}  // extern "C"
