// Lane-emulation harness for the near steps of the decoder's LDS-staged batch (wave_decode_lds_batch, lz4_device.inl): one block
// through wave_decode_block<true> or <false>, the batch's counters and the step counters.  Test infrastructure only
// (tests/test_decode_steps.py).
#define PLZ4_EMU 1
#include "../../plz4_amd/csrc/lz4_device.inl"

int plz4_emu_descending = 0;

extern "C" {

void emu_ds_set_descending(int d) { plz4_emu_descending = d; }

// the batch's counters (plz4_emu_dec) and the step counters (plz4_emu_steps); reset on read
void emu_ds_counters(unsigned long long* out8, unsigned long long* steps4)
{
    for (int i = 0; i < 8; ++i) { out8[i] = plz4::plz4_emu_dec[i]; plz4::plz4_emu_dec[i] = 0; }
    for (int i = 0; i < 4; ++i) { steps4[i] = plz4::plz4_emu_steps[i]; plz4::plz4_emu_steps[i] = 0; }
}

// lds != 0: the LDS-staged build of the vector path (the record kernels); 0: the one that copies through memory
int emu_ds_decode(const uint8_t* src, int n, uint8_t* dst, int cap, int lds)
{
    static thread_local __attribute__((aligned(16))) uint8_t lb[plz4::kDecLdsBytes];
    if (lds) return plz4::wave_decode_block<true>(src, n, dst, cap, nullptr, 0, lb);
    return plz4::wave_decode_block<false>(src, n, dst, cap);
}

}
