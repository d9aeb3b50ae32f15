// Lane-emulation harness of the wave-wide HC parser for blocks of at most 4 KiB under an attached dictionary context (k_hcx of
// plz4hip.hip: hcx_compress of plz4_amd/csrc/lz4hcx_device.inl -- the block's lists in the wave's LDS, the dictionary's lists as
// plz4hip_dict_create builds them, one candidate per lane, sequences written where they are decided).
// Test infrastructure only: built into tests/emu/_build/, never loaded by plz4_amd, not a CPU fallback.
#define PLZ4_EMU 1
#include "../../plz4_amd/csrc/lz4hcx_device.inl"
#include <stdlib.h>
#include <string.h>
#include <vector>

int plz4_emu_descending = 0;

using namespace plz4;

extern "C" {

void emu_hcx_set_descending(int d) { plz4_emu_descending = d; }
int  emu_hcx_min_level() { return kHcxMinLevel; }
int  emu_hcx_max_level() { return kHcxMaxLevel; }
int  emu_hcx_lds_bytes() { return (int)sizeof(HcxLds); }
int  emu_hcx_mid_lds_bytes() { return (int)sizeof(HcxMidLds); }

// LZ4_compress_HC_continue(src, n, cap) under the attached context of dict[0, dictLen) (its last <= 64 KiB, as the caller cut it).
// Returns the size, 0 when the block does not fit, -1 for a call the parser is not for.
int emu_hcx_compress(const uint8_t* src, int n, uint8_t* dst, int cap, int level, const uint8_t* dict, int dictLen)
{
    if (n < 0 || n > kHcxMaxBlock || level < kHcxMinLevel || level > kHcxMaxLevel || dictLen < 0 || dictLen > 65536) return -1;
    static thread_local HcxLds lds;
    std::vector<uint8_t> dcopy((size_t)dictLen + 64, 0);                    // (its own copy: reads past the end would show)
    if (dictLen) memcpy(dcopy.data(), dict, (size_t)dictLen);
    std::vector<uint32_t> start(kHcHashEntries + 1);
    std::vector<uint16_t> list(65536);
    hcx_dict_build(dcopy.data(), dictLen, start.data(), list.data());
    std::vector<uint8_t> scopy((size_t)n + 64, 0);
    if (n) memcpy(scopy.data(), src, (size_t)n);
    for (auto& v : lds.rank) v = 0xFFFF;                                    // (the lists are rebuilt for every block: nothing is left over)
    for (auto& v : lds.list) v = 0xFFFF;
    HcxDict d; d.bytes = dcopy.data(); d.len = dictLen; d.start = start.data(); d.list = list.data();
    static thread_local HcOpt opt[kHcOptNum + kHcTrailing + 1];
    if (level == 2) {                                                       // (the dictionary context's level-2 tables: k_hc_dict_prime's)
        static thread_local HcxMidLds mlds;
        memset(&mlds, 0xA5, sizeof mlds);
        std::vector<uint8_t> ws((size_t)kHcWorkBytes);
        HcWork dw; dw.hash = (uint32_t*)ws.data(); dw.chain = (uint16_t*)(ws.data() + kHcHashEntries * 4); dw.opt = nullptr; dw.pre = nullptr; dw.rank = nullptr; dw.list = nullptr;
        hc_prime_dict(dcopy.data(), dictLen, 2, dw);
        std::vector<uint64_t> seq((size_t)n / 4 + 128);
        return hcx_mid_block(scopy.data(), n, dst, cap, mlds, d, dw.hash, seq.data());
    }
    return hcx_compress(scopy.data(), n, dst, cap, level, lds, d, opt);
}

}  // extern "C"
