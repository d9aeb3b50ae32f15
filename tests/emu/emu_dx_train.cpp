// Lane-emulation harness of the few-block decoders' stage train (tests/emu/dx_train.h) for a call of raw blocks whose workspace is
// laid out for sizes the test names -- not for the blocks' own, as the other entries do -- and the rounds rule beside the three
// rules it replaced (tests/test_dx_train.py).  Test infrastructure only: built into tests/emu/_build/, never loaded by plz4_amd,
// not a CPU fallback.
#define PLZ4_EMU 1
#include "dx_train.h"

int plz4_emu_descending = 0;

using namespace plz4;

// flavour 0: DxF, 1: DxbF, 2: DxlF under the dictionary dict.  Block b: len[b] bytes at src[b], cap[b] bytes at dst + b * dstStride.
// answer[b]: the block's size, or -999999: left to the one-wave decoder.  Returns 0, or -888888: units that do not meet.
extern "C" int emu_dxt_call(int flavour, int nb, const uint8_t* const* src, const int32_t* len, const int32_t* cap, int64_t maxIn, int64_t maxOut,
                            const uint8_t* dict, int dictLen, uint8_t* dst, int64_t dstStride, int32_t* answer)
{
    // (the blocks as the product has them: exactly len and cap bytes)
    std::vector<DxEmuHeap<uint8_t>*> in(nb);
    std::vector<const uint8_t*> sp(nb);
    int64_t stride = 1;
    for (int b = 0; b < nb; ++b) if (cap[b] > stride) stride = cap[b];
    DxEmuHeap<uint8_t> all((size_t)(stride * (nb - 1) + cap[nb - 1]));
    for (int b = 0; b < nb; ++b) { in[b] = new DxEmuHeap<uint8_t>((size_t)len[b]); memcpy(in[b]->p, src[b], (size_t)len[b]); sp[b] = in[b]->p; }
    const int rc = dx_emu_raw_call(flavour, DxEmuCall{nb, sp.data(), len, cap, all.p, stride}, maxIn, maxOut, dict, dictLen, 0, answer);
    for (int b = 0; b < nb; ++b) { if (answer[b] > 0) memcpy(dst + b * dstStride, all.p + b * stride, (size_t)answer[b]); delete in[b]; }
    return rc;
}

extern "C" int emu_dx_rounds_for(int64_t span) { return dx_rounds_for(span); }
extern "C" int emu_dxb_rounds(int64_t maxOut) { return dxb_rounds(maxOut); }
extern "C" int emu_dx_rounds(int flavour, int nb, int64_t maxOut)
{
    return flavour == 0 ? DxF::rounds(nb, maxOut) : flavour == 1 ? DxbF::rounds(nb, maxOut) : DxlF::rounds(nb, maxOut);
}
// the layouts' strides, for the tests' edges
extern "C" void emu_dxt_strides(int flavour, int64_t maxIn, int64_t maxOut, int64_t* out3)
{
    out3[0] = (int64_t)dx_t_stride(maxIn); out3[1] = (int64_t)(flavour == 1 ? dxb_ptr_stride(maxOut) : dx_ptr_stride(maxOut)); out3[2] = dx_max_seg(maxIn);
}
