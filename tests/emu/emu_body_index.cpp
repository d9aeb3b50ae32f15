// Lane-emulation harness of the frame-body index (wave_index_body, plz4_amd/csrc/lz4_body_index_device.inl): the size-word walk
// behind plz4hip_dev_index_body, the same source the gfx950 kernel k_index_body is compiled from.
// Test infrastructure only: built into tests/emu/_build/, never loaded by plz4_amd, not a CPU fallback.
#define PLZ4_EMU 1
#include "../../plz4_amd/csrc/lz4_body_index_device.inl"

int plz4_emu_descending = 0;

using namespace plz4;

extern "C" {

void emu_body_index_set_descending(int d) { plz4_emu_descending = d; }

// recOff: maxBlocks + 1 entries; info: {int64 end, int32 nBlocks, int32 status}
void emu_index_body(const uint8_t* body, int64_t bodyBytes, int bsz, int blockChecksum, int maxBlocks, int64_t* recOff, void* info)
{
    wave_index_body(body, bodyBytes, bsz, blockChecksum != 0, maxBlocks, recOff, (BodyIndex*)info);
}

}  // extern "C"
