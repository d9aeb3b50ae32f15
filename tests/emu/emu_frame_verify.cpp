// Lane-emulation harness of the frame verdicts (wave_verify_frames and wave_verify_summary, plz4_amd/csrc/lz4_frame_verify_device.inl):
// the walk behind plz4hip_dev_verify_frames, the same source the gfx950 kernels k_verify_frames and k_verify_summary are compiled
// from.  Test infrastructure only: built into tests/emu/_build/, never loaded by plz4_amd, not a CPU fallback.
#define PLZ4_EMU 1
#include "../../plz4_amd/csrc/lz4_frame_verify_device.inl"

int plz4_emu_descending = 0;

using namespace plz4;

static_assert(sizeof(FrameVerdict) == 32 && sizeof(StreamVerdict) == 32, "the layouts of include/plz4hip.h");

extern "C" {

void emu_frame_verify_set_descending(int d) { plz4_emu_descending = d; }

// the launch of plz4hip_dev_verify_frames with a grid of nWaves one-wave workgroups, then the summary behind it
void emu_verify_frames(const void* frames, const void* info, int maxFrames, const uint8_t* dst, int64_t dstStride, int dstCap,
                       const int32_t* result, const int32_t* status, int maxRecs, void* verdicts, void* sv, int nWaves)
{
    for (int w = 0; w < nWaves; ++w)
        wave_verify_frames((const FrameIndex*)frames, (const StreamIndex*)info, maxFrames, dst, dstStride, dstCap, result, status, maxRecs,
                           (FrameVerdict*)verdicts, w, nWaves);
    wave_verify_summary((const StreamIndex*)info, maxFrames, (const FrameVerdict*)verdicts, (StreamVerdict*)sv);
}

}  // extern "C"
