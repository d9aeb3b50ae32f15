// Lane-emulation harness of plz4_amd/csrc/lz4_block_io.inl: the priming rule (hist_of, l1_prime, hc_prime, hc_pfx) as a table
// function over stand-in addresses, the rule driving the emulated encoders over a list of blocks laid out as the kernels find them
// (64 KiB of scratch in front of every block), and the record writer.  tests/test_block_io.py.
// Test infrastructure only: built into tests/emu/_build/, never loaded by plz4_amd, not a CPU fallback.
#define PLZ4_EMU 1
#include "../../plz4_amd/csrc/lz4_block_io.inl"
#include <stdlib.h>
#include <vector>

int plz4_emu_descending = 0;

using namespace plz4;

namespace {
// the stand-in addresses of tests/golden/make_prime_golden.py
const uint8_t* const SRC = (const uint8_t*)0x10000000, * const DICT = (const uint8_t*)0x20000000, * const TAIL = (const uint8_t*)0x30000000;
const int64_t STRIDE = 1 << 20;
void where(const uint8_t* p, int i, long long* kind, long long* off)
{
    *off = -1;
    if (!p) *kind = 0;
    else if (p == TAIL) *kind = 1;
    else if (p == DICT) *kind = 2;
    else { *kind = 3; *off = (long long)(p - (SRC + (int64_t)(i - 1) * STRIDE)); }
}
HcWork hc_work(uint8_t* ws)
{
    HcWork w;
    w.hash = (uint32_t*)ws; w.chain = (uint16_t*)(ws + kHcHashEntries * 4);
    w.opt = (HcOpt*)(ws + kHcHashEntries * 4 + kHcChainEntries * 2); w.pre = nullptr; w.rank = nullptr; w.list = nullptr;
    return w;
}
}  // namespace

extern "C" {

void bio_set_descending(int d) { plz4_emu_descending = d; }
int bio_ctx_max_block(void) { return kCtxMaxBlock; }
int bio_tail_len(int pl) { return tail_len(pl); }

// One row of tests/golden/prime_parent.json (prevLen: the length of block i - 1, any value where the rule does not read it):
// out = l1Mode l1Size l1Bytes l1Off hcMode hcLen hcBytes hcOff isCtx hcPfx.  Returns 0, or -1 when a table pointer is set in a
// mode that has none.
int bio_prime_row(int raw, int linked, int i, int prevTailLen, int dictLen, int prevLen, int n, long long* out)
{
    static const uint32_t table[1] = {0}, hash[1] = {0}; static const uint16_t chain[1] = {0};
    int32_t lens[3] = {5, 5, 5};
    if (i > 0) lens[i - 1] = prevLen;
    lens[i] = n;
    const HistView v{SRC, STRIDE, lens, 0, 1 << 20, linked, prevTailLen >= 0 ? TAIL : nullptr, prevTailLen, dictLen >= 0 ? DICT : nullptr, dictLen};
    const Hist h = hist_of(v, i, n, raw != 0);
    const DictEnc dc = l1_prime(h, raw != 0, table);
    const HcDict d = hc_prime(h, hash, chain);
    if ((dc.dictTable != nullptr) != (dc.mode == kDictCtxCopy || dc.mode == kDictCtxLookup)) return -1;
    if ((d.hash != nullptr) != (d.mode == kHcCtx) || (d.chain != nullptr) != (d.mode == kHcCtx) || (d.bytes != nullptr && d.mode != kHcCtx)) return -1;
    out[0] = dc.mode; out[1] = dc.dictSize; where(dc.dict, i, &out[2], &out[3]);
    out[4] = d.mode; out[5] = d.len; where(d.mode == kHcExt ? h.bytes : d.bytes, i, &out[6], &out[7]);
    out[8] = ctx_small(v, i, n, raw != 0); out[9] = hc_pfx(d);
    return 0;
}

// A call's blocks through the rule and the emulated encoders.  Block i: lens[i] bytes at src + i * srcStride, at least 64 KiB of
// writable scratch in front of it.  level 1: encode_block_primed; 2..12: hc_compress (the context's tables built by hc_prime_dict).
// Block i's bytes go to dst + i * dstStride (capacity cap), its return value to result[i].  order 1: last block first.
int bio_encode(uint8_t* src, long long srcStride, const int32_t* lens, int nb, int level, int rawApi, int linked, const uint8_t* prevTail, int prevTailLen,
               const uint8_t* dict, int dictLen, const uint32_t* dictTable, uint8_t* dst, long long dstStride, int cap, int32_t* result, int order)
{
    static thread_local uint32_t lds[kHashBytes / 4];
    std::vector<uint8_t> ws(level > 1 ? kHcWorkBytes : 0), dws(level > 1 ? kHcWorkBytes : 0);
    HcWork dw{};
    if (level > 1 && dict) { dw = hc_work(dws.data()); hc_prime_dict(dict, dictLen > 0 ? dictLen : 0, level, dw); }
    const HistView v{src, srcStride, lens, 0, 0, linked, prevTail, prevTailLen, dict, dictLen};
    for (int j = 0; j < nb; ++j) {
        const int i = order ? nb - 1 - j : j;
        const int n = lens[i];
        const uint8_t* s = src + (long long)i * srcStride;
        uint8_t* out = dst + (long long)i * dstStride;
        const Hist h = hist_of(v, i, n, rawApi != 0);
        if (level == 1) result[i] = encode_block_primed(s, n, out, cap, l1_prime(h, rawApi != 0, dictTable), lds);
        else {
            const HcDict d = hc_prime(h, dw.hash, dw.chain);
            if (d.mode == kHcExt) lay_segment(s, h.bytes, d.len);
            result[i] = hc_compress(s, n, out, cap, level, hc_work(ws.data()), d);
        }
    }
    return 0;
}

// blk.CompressToBlk of s[0, n) with capacity bsz: the fused level-1 encoder, then the record writer.  rec: 4 + max(c, n) + 4 bytes
// at least.  *cOut: what the encoder returned.  Returns the record's length.
int bio_block_record(const uint8_t* s, int n, int bsz, int blockChecksum, uint8_t* rec, int* cOut)
{
    static thread_local uint32_t lds[kHashBytes / 4];
    const int c = wave_encode_block(s, n, rec + 4, bsz, lds);
    if (cOut) *cOut = c;
    return wave_finish_record(rec, s, n, c, blockChecksum != 0);
}
// the writer alone, behind an encoder that left c bytes at rec + 4
int bio_finish_record(uint8_t* rec, const uint8_t* s, int n, int c, int blockChecksum) { return wave_finish_record(rec, s, n, c, blockChecksum != 0); }

}  // extern "C"
