// Lane-emulation harness of the few-block decoder's big path (raw blocks above 4 MiB + 8; dxb_* in
// plz4_amd/csrc/lz4_dx_device.inl): the stage train of dx_train.h behind a C entry for tests/dx_big_cases.py.  Test
// infrastructure only: built into tests/emu/_build/, never loaded by plz4_amd, not a CPU fallback.
#define PLZ4_EMU 1
#include "dx_train.h"

int plz4_emu_descending = 0;

using namespace plz4;

extern "C" void emu_dxb_set_descending(int d) { plz4_emu_descending = d; }

// out5: jump rounds launched, rounds taken (the one that saw nothing move included), runs listed, groups, the list's room
extern "C" int emu_dxb_decode(const uint8_t* src, int n, uint8_t* dst, int cap, int G, int thr, int* out5)
{
    DxbEmuStats st;
    // (the source as the product has it: n bytes, none behind them)
    DxEmuHeap<uint8_t> in((size_t)(n > 0 ? n : 0));
    if (n > 0) memcpy(in.p, src, (size_t)n);
    DxEmuHeap<uint8_t> out((size_t)(cap > 0 ? cap : 0));
    const int r = dxb_emu_block(in.p, n, out.p, cap, n > 16384 ? n : 16384, cap > 0 ? cap : 1, G, thr, &st);
    if (r > 0) memcpy(dst, out.p, (size_t)r);
    out5[0] = st.launched; out5[1] = st.taken; out5[2] = st.runs; out5[3] = st.groups; out5[4] = st.room;
    return r;
}
