// Lane-emulation harness of the frame writer (wave_frame_edges, wave_frame_move and wave_frame_summary,
// plz4_amd/csrc/lz4_frame_write_device.inl): the kernels behind plz4hip_dev_write_frames, the same source k_frame_edges, k_frame_move
// and k_frame_summary are compiled from, and the stream index over what they wrote (wave_index_stream).  Test infrastructure only:
// built into tests/emu/_build/, never loaded by plz4_amd, not a CPU fallback.
#define PLZ4_EMU 1
#include "../../plz4_amd/csrc/lz4_frame_write_device.inl"

int plz4_emu_descending = 0;

using namespace plz4;

static_assert(sizeof(WriteInfo) == 32 && sizeof(FrameIndex) == 64, "the layouts of include/plz4hip.h");

extern "C" {

void emu_frame_write_set_descending(int d) { plz4_emu_descending = d; }

// the launches of plz4hip_dev_write_frames: k_frame_edges on min(ceil(nFrames / 16), waves) one-wave workgroups, k_frame_move on
// (nBlocks, slices) workgroups of four waves, k_frame_summary
void emu_write_frames(const int32_t* opts, const uint8_t* src, int64_t srcBytes, int64_t srcStride, const uint8_t* body, int64_t bodyBytes,
                      const int64_t* recOff, int blocksPerFrame, uint8_t* out, int64_t outCap, void* frames, int64_t* outRecOff, void* info,
                      int waves, int slices)
{
    // (opts: the eight words of plz4hip_frame_opts)
    const FrameWriteGeom g = frame_write_geom(opts[0], opts[1] != 0, opts[2] != 0, opts[3] != 0, opts[4] != 0, opts[5] != 0, (uint32_t)opts[6], srcBytes,
                                              srcStride, bodyBytes, blocksPerFrame, outCap);
    const int64_t groups = ((int64_t)g.nFrames + 15) / 16;
    const int grid = (int)(groups < waves ? groups : waves);
    for (int w = 0; w < grid; ++w) wave_frame_edges(g, src, body, recOff, out, (FrameIndex*)frames, outRecOff, w, grid);
    for (int i = 0; i < g.nBlocks; ++i)
        for (int wv = 0; wv < 4 * slices; ++wv) wave_frame_move(g, body, recOff, out, i, wv, 4 * slices);
    wave_frame_summary(g, recOff, (const FrameIndex*)frames, (WriteInfo*)info);
}

void emu_frame_write_index_stream(const uint8_t* bytes, int64_t nBytes, int maxFrames, int maxRecs, void* frames, int64_t* recOff, void* info)
{
    wave_index_stream(bytes, nBytes, maxFrames, maxRecs, (FrameIndex*)frames, recOff, (StreamIndex*)info);
}

}  // extern "C"
