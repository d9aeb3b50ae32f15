// Lane-emulation harness of the sixteen-buffer checksum (wave_xxh32_x16) and of the one-wave scan of lengths (wave_scan_lengths),
// plz4_amd/csrc/lz4_device.inl: the emit stage's LDS-free kernels.
// Test infrastructure only: built into tests/emu/_build/, never loaded by plz4_amd, not a CPU fallback.
#define PLZ4_EMU 1
#include "../../plz4_amd/csrc/lz4_device.inl"

int plz4_emu_descending = 0;

using namespace plz4;

extern "C" {

void emu_x16_set_descending(int d) { plz4_emu_descending = d; }
int  emu_x16_depth() { return kX16Depth; }

// out[i] = xxh32(ptrs[i], lens[i]) for i < count, one emulated wave per sixteen buffers; the groups of the last wave beyond
// count have no buffer.  Returns the number of waves.
int emu_x16_hash(const uint8_t* const* ptrs, const int* lens, int count, uint32_t* out)
{
    int waves = 0;
    for (int w0 = 0; w0 < count; w0 += 16, ++waves) {
        const uint8_t* p[64]; int n[64]; uint32_t h[64];
        for (int lane = 0; lane < 64; ++lane) {
            const int i = w0 + (lane >> 2);
            p[lane] = i < count ? ptrs[i] : nullptr;
            n[lane] = i < count ? lens[i] : -1;
        }
        wave_xxh32_x16(p, n, h);
        for (int g = 0; g < 16 && w0 + g < count; ++g) out[w0 + g] = h[4 * g];
    }
    return waves;
}

// the scan body as k_scan (clamp = 0, first = 1) and k_scan_from (clamp = 1) call it; off: n + 1 entries
void emu_x16_scan(const int32_t* len, int64_t* off, int n, int first, int clamp)
{
    if (clamp) wave_scan_lengths<true>(len, off, n, first); else wave_scan_lengths<false>(len, off, n, first);
}

}  // extern "C"
