// Lane-emulation harness of the stream index (wave_index_stream, plz4_amd/csrc/lz4_stream_index_device.inl): the header-mode /
// body-mode walk behind plz4hip_dev_index_stream, the same source the gfx950 kernel k_index_stream is compiled from.
// Test infrastructure only: built into tests/emu/_build/, never loaded by plz4_amd, not a CPU fallback.
#define PLZ4_EMU 1
#include "../../plz4_amd/csrc/lz4_stream_index_device.inl"

int plz4_emu_descending = 0;

using namespace plz4;

static_assert(sizeof(FrameIndex) == 64 && sizeof(StreamIndex) == 32, "the layouts of include/plz4hip.h");

extern "C" {

void emu_stream_index_set_descending(int d) { plz4_emu_descending = d; }

// frames: maxFrames entries of 64 bytes; recOff: maxRecs + 1 entries; info: 32 bytes
void emu_index_stream(const uint8_t* bytes, int64_t nBytes, int maxFrames, int maxRecs, void* frames, int64_t* recOff, void* info)
{
    wave_index_stream(bytes, nBytes, maxFrames, maxRecs, (FrameIndex*)frames, recOff, (StreamIndex*)info);
}

}  // extern "C"
