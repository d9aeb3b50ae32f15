// plz4hip.hip -- gfx950 kernels + the C ABI declared in include/plz4hip.h.
//
// Launch shape: ONE 64-lane wavefront per LZ4 block, persistent waves pulling block indices from a device-side
// counter (every wave exits when the counter passes nBlocks).  An encoder wave owns 16 KiB of LDS (liblz4's hash
// table, lz4.h:695-697): ten encoder waves per CU when a call fills the chip (one workgroup of ten independent waves
// per CU, see ENC_WAVE_TABLE), one-wave workgroups otherwise; the record decoder stages each batch of output in
// 1.1 KiB of LDS and is bounded by its registers (24 waves per CU).  Waves never communicate.
#include <hip/hip_runtime.h>

#include <array>
#include <atomic>
#include <mutex>
#include <thread>
#include <string>
#include <vector>
#include <cstdio>
#include <cstring>

#include "../../include/plz4hip.h"
#include "stream_ws.h"
#if defined(PLZ4_STATS)
__device__ unsigned long long plz4_stats[24];
#endif
#include "lz4_device.inl"
#include "lz4_seq_device.inl"
#include "lz4hc_device.inl"
#include "lz4hc12_device.inl"
#include "lz4hc_lists_device.inl"
#include "lz4hc_lazy_device.inl"
#include "lz4hcx_device.inl"
#include "lz4_dx_device.inl"
#include "lz4_fx_device.inl"
#include "lz4_mx_device.inl"
#include "lz4_block_io.inl"
#include "lz4_body_index_device.inl"
#include "lz4_stream_index_device.inl"
#include "lz4_frame_verify_device.inl"
#include "lz4_frame_write_device.inl"
#include "ws_layout.h"
#include "route.h"

namespace {

using namespace plz4;

// ------------------------------------------------------------------------------------------------ kernels
struct CodecArgs {
    const uint8_t* src;  int64_t srcStride;  const int32_t* srcLen;  int64_t srcBytes;  int bsz;
    uint8_t*       dst;  int64_t dstStride;  const int32_t* dstCap;  int dstCapAll;
    const int64_t* recOff;
    int32_t*       result;
    int32_t*       status;
    uint32_t*      queue;
    int            nBlocks;
    int            blockChecksum;
    // dictionary / linked blocks
    const uint8_t*  dict;       int dictLen;        // last <= 64 KiB of the user dictionary (device), or null
    const uint32_t* dictTable;                      // LZ4_loadDictSlow table of that dictionary
    int             linked;                         // encode: block i>0 is primed with the tail of block i-1
    const uint8_t*  prevTail;   int prevTailLen;    // linked: window of block 0 (-1: block 0 starts a frame)
    uint8_t*        window;     int* windowLen;     // linked decode: the 64 KiB sliding dictionary (2 x 64 KiB ping-pong) per chain, in/out
    int             nChains;    const int32_t* chainFirst;   // linked decode of several frames at once: chain c = records [chainFirst[c], chainFirst[c+1])
    // HC levels 2..12
    int             level;
    uint8_t*        hcWork;                         // gridDim.x x kHcWorkBytes
    const uint32_t* hcDictHash;                     // HC + dictionary: the dictionary context's tables for this level's strategy
    const uint16_t* hcDictChain;                    //   (clz4.NewDictCtxHC, clz4.go:122-147), built by k_hc_dict_prime
    int             hcEx;                           // HC call with a dictionary and/or linked blocks: inputs have 64 KiB of scratch in front
    // blocks <= 4 KiB under a dictionary context at levels 2..12 (lz4hcx_device.inl, k_hcx): the dictionary's lists (plz4hip_dict_create);
    // hcx: the call's blocks of that kind are k_hcx's (the one-thread kernels pass them over)
    const uint32_t* hcxStart;   const uint16_t* hcxList;   int hcx;
    int32_t*        hcPfx;                          // such a call on the list path (k_hc_ext_prep): per block, the bytes of the external segment that
                                                    // lies right in front of it (>= 0), or -1: a block <= 4 KiB under a dictionary context (k_encode_*_hc's)
    // level 12 in three phases (lz4hc12_device.inl): per-block chain and search results of the group [blk0, blk0 + nBlocks)
    int             blk0;
    uint16_t*       h12Chain;   int64_t h12ChainStride;      // entries per block (a multiple of 1024)
    uint32_t*       h12Rank;                                 // h12ChainStride entries per block
    uint32_t*       h12List;                                 // h12ChainStride + 8 entries per block (8 readable entries in front of index 0)
    uint32_t*       h12Offsets;                              // 32768 per block: where each hash's run starts in the list
    Hc12F*          h12F;       int64_t h12FStride;          // entries per block
    uint8_t*        h12Ws;                                   // gridDim.x x kHc12WsGlobalBytes: the price table's overflow
    int32_t*        h12Err;                                  // set when a kernel gives up (spin guard)
    int             rawMode;                                 // parse kernel: 1 = raw LZ4 blocks (dstCap per block), 0 = frame records
    int             h12Gather, h12Idle;                      // search kernel: lanes a phase / the queue waits for before its section runs
    // level 1 in stages (lz4_seq_device.inl): parse -> sizes -> scan -> write -> finish over the group [blk0, blk0 + nBlocks);
    // the workspace is indexed by the block's number inside the group
    SeqInfo*        l1Info;                                  // per block
    uint64_t*       l1Seq;      int64_t l1SeqStride;         // sequence records, entries per block
    uint32_t*       l1ChunkBytes; uint32_t* l1ChunkOff; int l1MaxChunks;   // per block: bytes of / before every chunk of 1024 sequences
    uint8_t*        l1Bk;                                    // per sequence: its catch-up length (l1SeqStride bytes per block)
    int             l1MaxLen;                                // what the workspace was sized for
    // levels 3..9 (lz4hc_lazy_device.inl): a block is walked in up to lzSegs segments of at least lzMinSeg bytes at once
    int             lzSegs, lzMinSeg;
    uint64_t*       lzRec;      uint64_t* lzBridge;  int64_t lzRecStride;     // records of the segments / of the walks into them, entries per block
    LzSegMeta*      lzMeta;     uint64_t* lzStarts;  LzPiece* lzPieces;       // per block: lzSegs, lzSegs * kLzStarts, 2 * lzSegs entries
    // a few blocks decoded by the whole chip (lz4_dx_device.inl): per block, the chain table of its input (one entry per byte), the
    // pointer table of its output (one per byte), the units of its segments, its state
    uint64_t*       dxT;        int64_t dxTStride;
    uint32_t*       dxPtr;      int64_t dxPtrStride;
    DxUnit*         dxUnits;    int dxMaxSeg;   int dxRound;
    DxInfo*         dxInfo;
    // the staged level-1 call writing its records back to back (plz4hip_dev_encode_body): dst = the frame body, bodyOff[i] = where
    // record i starts (made by the call: the scan over the records' lengths), bodyCap = the body's room
    int64_t*        bodyOff;    int64_t bodyCap;
    // the staged level-1 parse tells when its block queue has run dry (its last blocks are under way, workgroups begin to leave):
    // gate <- max(gate, gateSeq); the parse of the next call on ANOTHER stream waits for that behind k_parse_gate (launch_l1)
    uint32_t*       gate;       uint32_t gateSeq;
    const int64_t*  dxSrcOff;   const int32_t* dxLen;                       // records: where a block's payload starts in src and its size (-1: not this path's; -2, kDxRecBad: it fails the frame reader's checks)
    int32_t*        dxHashBad;                                              // records: the payload's xxh32 does not match (k_dx_rec_hash)
    // ... with history outside the block (dxl_*, lz4_dx_device.inl): per block the first block and the number of its chain, its row
    // of moved flags (kDxlMaxRounds + 1), whether the path has answered it; the jump rounds launched
    int32_t*        dxlFirst;   int32_t* dxlChain;   uint32_t* dxlMoved;   int32_t* dxlGood;   int dxlRounds;
    // a linked call cut into groups of consecutive blocks (launch_decode): every pointer above is the group's own view (block 0 = the
    // group's first block, chain 0 = the first chain with a block in it); chainFirst stays the call's, so the group's first block
    // dxlBlk0 comes off it.  dxlDead: per chain, an earlier group has met a bad block of it (null: the call is one group).
    // dxlGroup / dxlGroups: this group's number / how many the call has (0: not a grouped call).
    int32_t*        dxlDead;    int dxlBlk0;    int dxlGroup;   int dxlGroups;
    // raw blocks above kDxMaxOut (dxb_*, lz4_dx_device.inl): per block the composed rows of its groups of dxbG segments (one row of
    // kDxSeg entries per group), where the chain enters each group, the list of its long runs (dxbRunRoom entries), its state; the
    // run threshold and the jump rounds launched
    uint64_t*       dxbTG;      int64_t dxbTGStride;   DxbEntry* dxbEnt;   int dxbGroups;   int dxbG;
    DxRun*          dxbRuns;    int dxbRunRoom;   int dxbThr;   DxbInfo* dxbInfo;   int dxbRounds;
};

__device__ __forceinline__ int next_block(uint32_t* q)
{
    uint32_t v = 0;
    if ((threadIdx.x & 63u) == 0) v = atomicAdd(q, 1u);
    return (int)plz4_readfirstlane(v);
}

__device__ __forceinline__ int block_len(const CodecArgs& a, int i)
{
    if (a.srcLen) return a.srcLen[i];
    const int64_t rem = a.srcBytes - (int64_t)i * a.bsz;
    return (int)(rem < a.bsz ? rem : a.bsz);
}
// the room of raw block i's destination
__device__ __forceinline__ int cap_of(const CodecArgs& a, int i) { return a.dstCap ? a.dstCap[i] : a.dstCapAll; }

// ---- the two rules of lz4_block_io.inl on a call's arguments ----------------------------------------------------------------------
static_assert(kHcxMaxBlock == kCtxMaxBlock, "k_hcx serves the blocks a dictionary context serves by lookup");
// the call as the priming rule reads it
__device__ __forceinline__ HistView hist_view(const CodecArgs& a)
{
    return HistView{a.src, a.srcStride, a.srcLen, a.srcBytes, a.bsz, a.linked, a.prevTail, a.prevTailLen, a.dict, a.dictLen};
}
// how block i of a level-1 call is primed / of an HC call, its external segment laid in front of the block at s
__device__ __forceinline__ DictEnc l1_prime_of(const CodecArgs& a, int i, int n, bool rawApi) { return l1_prime(hist_of(hist_view(a), i, n, rawApi), rawApi, a.dictTable); }
__device__ __forceinline__ HcDict hc_prime_of(const CodecArgs& a, int i, int n, const uint8_t* s, bool rawApi)
{
    const Hist h = hist_of(hist_view(a), i, n, rawApi);
    const HcDict d = hc_prime(h, a.hcDictHash, a.hcDictChain);
    if (d.mode == kHcExt) lay_segment(s, h.bytes, d.len);
    return d;
}
// whether block i of an HC call is one its dictionary context serves by lookup (k_hcx's blocks), nothing read or laid out
__device__ __forceinline__ bool hc_is_ctx(const CodecArgs& a, int i, int n, bool rawApi) { return ctx_small(hist_view(a), i, n, rawApi); }
// Block i (s, n bytes) through enc(out, cap) -> bytes written or 0.  raw: an LZ4 block at dst + i * dstStride, result[i] = enc's
// answer.  Else blk.CompressToBlk: the payload at rec + 4 with capacity bsz (blk.go:73), the record around it, result[i] = its length.
template <class Enc> __device__ __forceinline__ void encode_out(const CodecArgs& a, int i, const uint8_t* s, int n, bool raw, Enc enc)
{
    uint8_t* const out = a.dst + (int64_t)i * a.dstStride;
    const int c = enc(raw ? out : out + 4, raw ? cap_of(a, i) : a.bsz);
    const int r = raw ? c : wave_finish_record(out, s, n, c, a.blockChecksum != 0);
    if ((threadIdx.x & 63u) == 0) a.result[i] = r;
}

// The level-1 encoder kernels run up to TEN independent waves per workgroup, each with its own 16 KiB table: one such
// workgroup owns all 160 KiB of a CU's LDS, i.e. ten tables per CU, where one-wave workgroups of 16 KiB only reach nine per CU
// (scripts/micro/residency.hip: "2560 16384 64" -> 9 per CU; two 80 KiB workgroups of five waves do not co-reside either --
// measured on k_encode_rec: the second one waits for the first).  The waves of a workgroup never synchronise; each pulls block
// ids from the queue until it is empty.  Only a call that fills the chip by itself is launched that way: a smaller one (the
// chunks of a host call, several of which share the GPU) keeps one-wave workgroups of 16 KiB, which leave the rest of a CU's
// LDS to other kernels -- hence the two instantiations of every encoder kernel (W = waves per workgroup).
constexpr int kEncWavesPerWg = 10;
#define ENC_WAVE_TABLE(name) \
    __shared__ uint32_t name##_all[W][kHashBytes / 4]; \
    uint32_t* const name = name##_all[W == 1 ? 0 : plz4_readfirstlane((int)(threadIdx.x >> 6))]

// LZ4 blocks only: dst[i] <- LZ4_compress_fast(src[i]), result[i] = bytes or 0.
template <int W> __global__ __launch_bounds__(64 * W) void k_encode_raw(CodecArgs a)
{
    ENC_WAVE_TABLE(lds);
    for (int i = next_block(a.queue); i < a.nBlocks; i = next_block(a.queue)) {
        const int      n = block_len(a, i);
        const uint8_t* s = a.src + (int64_t)i * a.srcStride;
        encode_out(a, i, s, n, true, [&](uint8_t* out, int cap) { return wave_encode_block(s, n, out, cap, lds); });
    }
}

// blk.CompressToBlk on the device: [LE32 size|stored][payload][LE32 xxh32?] at dst + i*dstStride.
template <int W> __global__ __launch_bounds__(64 * W) void k_encode_rec(CodecArgs a)
{
    ENC_WAVE_TABLE(lds);
    for (int i = next_block(a.queue); i < a.nBlocks; i = next_block(a.queue)) {
        const int      n = block_len(a, i);
        const uint8_t* s = a.src + (int64_t)i * a.srcStride;
        encode_out(a, i, s, n, false, [&](uint8_t* out, int cap) { return wave_encode_block(s, n, out, cap, lds); });
    }
}

// ---- level 1 in stages (independent blocks up to 4 MiB, no dictionary): lz4_seq_device.inl ------------------------------------
// k_l1_parse: persistent, one wave per block, the hash table in LDS -- the only serial stage; it writes one 8-byte record per
// sequence.  The others are plain data-parallel kernels, one lane per sequence, any number of waves per block, no LDS.
template <int kLdsWin = 0>
__device__ __forceinline__ void l1_parse_loop(const CodecArgs& a, uint32_t* lds, uint8_t* scr = nullptr)
{
    for (int i = next_block(a.queue); i < a.nBlocks; i = next_block(a.queue)) {
        const int gi = a.blk0 + i;
        const int n  = block_len(a, gi);
        int lastAnchor = 0, nseq = -1;                                       // -1: a block the workspace was not sized for
        if (n >= 0 && n <= a.l1MaxLen)
            nseq = wave_parse_l1<kLdsWin>(a.src + (int64_t)gi * a.srcStride, n, lds, a.l1Seq + (int64_t)i * a.l1SeqStride, &lastAnchor, scr);
        if ((threadIdx.x & 63u) == 0) { SeqInfo inf; inf.nseq = nseq; inf.lastAnchor = lastAnchor; inf.total = 0; inf.stored = 0; a.l1Info[i] = inf; }
    }
    if (a.gate && (threadIdx.x & 63u) == 0) atomicMax(a.gate, a.gateSeq);    // (sequence numbers: launch_l1 starts over before they wrap)
}
// One wave that holds its stream back until the parse launch `want` has run its queue dry (or ~1.5 s have passed: never a hang).
// Two parse launches started together share the CUs half and half and stay in step from then on -- nothing of one call then runs
// beside the other's parse; behind this gate the second one moves into the CUs as the first one's workgroups leave them.
__global__ __launch_bounds__(64) void k_parse_gate(const uint32_t* gate, uint32_t want)
{
    for (int it = 0; it < 400000; ++it) {
        if ((int32_t)(__hip_atomic_load(gate, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - want) >= 0) break;
        __builtin_amdgcn_s_sleep(127);
    }
}
template <int W> __global__ __launch_bounds__(64 * W) void k_l1_parse(CodecArgs a)
{
    ENC_WAVE_TABLE(lds);
    l1_parse_loop<2>(a, lds);                  // (ten tables fill the CU's LDS: the windows through the lane exchange, lz4_seq_device.inl)
}

// grid (waves per block / 4, blocks of the group): bytes of every chunk of 1024 sequences.  kBack: the level-1 parser's records
// (their catch-up is measured here); false: the HC parsers' records, which carry the final match.
// (kSeg / xb: blocks with an external segment in front of them, k_fxl_sizes / k_fxl_write below)
template <bool kBack, bool kSeg = false> __device__ __forceinline__ void l1_sizes_body(const CodecArgs a, const FxlBlk* xb = nullptr)
{
    const int i = blockIdx.y, wave = blockIdx.x * 4 + (int)(threadIdx.x >> 6), nW = gridDim.x * 4;
    const int nseq = a.l1Info[i].nseq;
    if (nseq <= 0) return;
    const int gi = a.blk0 + i;
    const uint8_t*  s   = a.src + (int64_t)gi * a.srcStride;
    const uint64_t* seq = a.l1Seq + (int64_t)i * a.l1SeqStride;
    const int nChunks = (nseq + kSeqChunk - 1) / kSeqChunk;
    for (int c = wave; c < nChunks; c += nW) {
        const uint32_t v = seq_emit_sizes<kBack, kSeg>(s, seq, kBack ? a.l1Bk + (int64_t)i * a.l1SeqStride : nullptr, nseq, c, kSeg ? max_(xb[i].pfx, 0) : 0);
        if ((threadIdx.x & 63u) == 0) a.l1ChunkBytes[(int64_t)i * a.l1MaxChunks + c] = v;
    }
}
template <bool kBack> __global__ __launch_bounds__(256) void k_l1_sizes(CodecArgs a) { l1_sizes_body<kBack>(a); }

// one wave per block: where every chunk goes, the block's size, liblz4's limitedOutput verdict; raw mode: result[i] = size or 0;
// records (blk.CompressToBlk, blk/blk.go:69-109): the size word (stored iff the encoder returned 0) and, without block
// checksums, the record length
__global__ __launch_bounds__(256) void k_l1_scan(CodecArgs a)
{
    const int i = blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (i >= a.nBlocks) return;
    const int gi = a.blk0 + i;
    const int n  = block_len(a, gi);
    SeqInfo inf = a.l1Info[i];
    const int cap = a.rawMode ? cap_of(a, gi) : a.bsz;     // records: capacity == bsz (blk/blk.go:73)
    int total = 0;
    const bool broken = inf.nseq == kSeqEngineFailed;                                 // (an HC search phase that gave up: no result)
    if (inf.nseq >= 0)
        total = seq_emit_scan(a.l1ChunkBytes + (int64_t)i * a.l1MaxChunks, a.l1ChunkOff + (int64_t)i * a.l1MaxChunks, inf.nseq, inf.lastAnchor, n, cap);
    if ((threadIdx.x & 63u) == 0) {
        inf.total = total; inf.stored = (total == 0);
        a.l1Info[i] = inf;
        if (broken) a.result[gi] = PLZ4HIP_E_DEVICE;
        else if (a.rawMode) a.result[gi] = total;
        else if (a.bodyOff) {
            // records back to back: every record's length now (the scan behind this kernel places them; the size word is written
            // with the payload, k_l1_write)
            a.result[gi] = (total ? total : n) + 4 + (a.blockChecksum ? 4 : 0);
        } else {
            const int c = total ? total : n;                                          // ErrCompress -> stored raw (blk.go:78-92)
            st32u(a.dst + (int64_t)gi * a.dstStride, total ? ((uint32_t)c & 0x7FFFFFFFu) : (0x80000000u | ((uint32_t)n & 0x7FFFFFFFu)));
            if (!a.blockChecksum) a.result[gi] = c + 4;
        }
    }
}

// grid as k_l1_sizes: every chunk written at its place; a record whose encoder returned 0 gets the plaintext instead
template <bool kBack, bool kSeg = false> __device__ __forceinline__ void l1_write_body(const CodecArgs a, const FxlBlk* xb = nullptr)
{
    const int i = blockIdx.y, wave = blockIdx.x * 4 + (int)(threadIdx.x >> 6), nW = gridDim.x * 4;
    const SeqInfo inf = a.l1Info[i];
    const int gi = a.blk0 + i;
    const int n  = block_len(a, gi);
    const uint8_t* s   = a.src + (int64_t)gi * a.srcStride;
    uint8_t*       out = a.dst + (int64_t)gi * a.dstStride + (a.rawMode ? 0 : 4);
    if (a.bodyOff) {
        // the record's place in the frame body; one that does not fit is not written (the caller sees bodyOff[n] > bodyCap)
        const int64_t off = a.bodyOff[gi];
        if (inf.nseq == kSeqEngineFailed || off + (int64_t)((inf.total ? inf.total : n) + 4 + (a.blockChecksum ? 4 : 0)) > a.bodyCap) return;
        out = a.dst + off + 4;
        if (wave == 0 && (threadIdx.x & 63u) == 0)                                    // the size word, stored iff the encoder returned 0 (blk.go:78-92)
            st32u(out - 4, inf.total ? ((uint32_t)inf.total & 0x7FFFFFFFu) : (0x80000000u | ((uint32_t)n & 0x7FFFFFFFu)));
    }
    if (kSeg && inf.nseq == kSeqElsewhere && inf.total > 0) {
        // (a frame body's block <= 4 KiB under a dictionary context: k_fxl_small has left its bytes where its records would lie)
        if (wave == 0) wave_copy(out, (const uint8_t*)(a.l1Seq + (int64_t)i * a.l1SeqStride), inf.total);
    } else if (inf.total > 0) {
        const uint64_t* seq = a.l1Seq + (int64_t)i * a.l1SeqStride;
        const int nChunks = (inf.nseq + kSeqChunk - 1) / kSeqChunk;
        for (int c = wave; c < (nChunks ? nChunks : 1); c += nW)
            seq_emit_write<kBack, kSeg>(s, n, seq, kBack ? a.l1Bk + (int64_t)i * a.l1SeqStride : nullptr, inf.nseq, inf.lastAnchor, c, nChunks ? a.l1ChunkOff[(int64_t)i * a.l1MaxChunks + c] : 0u, out,
                                        kSeg ? max_(xb[i].pfx, 0) : 0);
    } else if (!a.rawMode && n > 0) {
        const int slice = (((n + nW - 1) / nW) + 15) & ~15;
        const int off = wave * slice;
        if (off < n) wave_copy(out + off, s + off, min_(slice, n - off));
    }
}
template <bool kBack> __global__ __launch_bounds__(256) void k_l1_write(CodecArgs a) { l1_write_body<kBack>(a); }

// records with block checksums: xxh32 over the payload as stored (blk.go:98-102), one wave per 16 blocks (wave_xxh32_x16: four
// lanes per block); no LDS, so the kernel runs beside a parse launch that holds all of it
__global__ __launch_bounds__(64) void k_l1_finish(CodecArgs a)
{
    const int i = blockIdx.x * 16 + (int)((threadIdx.x & 63u) >> 2);
    const uint8_t* p[1] = {nullptr};
    int n[1] = {-1};
    uint32_t x[1];
    int gi = 0;
    bool failed = false;
    if (i < a.nBlocks) {
        gi = a.blk0 + i;
        const SeqInfo inf = a.l1Info[i];
        const int c = inf.total ? inf.total : block_len(a, gi);
        failed = inf.nseq == kSeqEngineFailed;
        const uint8_t* rec = a.dst + (int64_t)gi * a.dstStride;
        bool written = true;
        if (a.bodyOff) {
            const int64_t off = a.bodyOff[gi];
            written = !failed && off + (int64_t)c + 8 <= a.bodyCap;           // (not written: k_l1_write)
            rec = a.dst + off;
        }
        if (written) { p[0] = rec + 4; n[0] = c; }
    }
    wave_xxh32_x16(p, n, x);
    if ((threadIdx.x & 3u) == 0 && n[0] >= 0) {
        st32u(const_cast<uint8_t*>(p[0]) + n[0], x[0]);
        if (!a.bodyOff) a.result[gi] = failed ? PLZ4HIP_E_DEVICE : n[0] + 8;
    }
}

// blk.CompressToBlk with a dictionary and/or linked blocks (config 5).
template <int W> __global__ __launch_bounds__(64 * W) void k_encode_rec_dict(CodecArgs a)
{
    ENC_WAVE_TABLE(lds);
    for (int i = next_block(a.queue); i < a.nBlocks; i = next_block(a.queue)) {
        const int      n  = block_len(a, i);
        const uint8_t* s  = a.src + (int64_t)i * a.srcStride;
        const DictEnc  dc = l1_prime_of(a, i, n, false);
        encode_out(a, i, s, n, false, [&](uint8_t* out, int cap) { return encode_block_primed(s, n, out, cap, dc, lds); });
    }
}

// Raw LZ4 blocks with a dictionary context (StreamIndieCtx): the block API with WithBlockDictionary (plz4_block.go:48-53).
template <int W> __global__ __launch_bounds__(64 * W) void k_encode_raw_dict(CodecArgs a)
{
    ENC_WAVE_TABLE(lds);
    for (int i = next_block(a.queue); i < a.nBlocks; i = next_block(a.queue)) {
        const int      n  = block_len(a, i);
        const uint8_t* s  = a.src + (int64_t)i * a.srcStride;
        const DictEnc  dc = l1_prime_of(a, i, n, true);
        encode_out(a, i, s, n, true, [&](uint8_t* out, int cap) { return encode_block_primed(s, n, out, cap, dc, lds); });
    }
}

// ---- the parse of a few blocks cut across the chip (lz4_pieces_device.inl): grid (pieces, blocks of the group), one wave each,
// one launch per round, then the gather into the staged path's records (l1Seq / l1Info) -- the emit kernels run unchanged behind it.
// Workspace per piece: meta, entry state, two exit states, records (PieceLayout).  cnt: the ctx's counters (plz4hip_ctx_counters).
struct PieceArgs { PieceMeta* meta; uint32_t* tabIn; uint32_t* tabOut; uint64_t* rec; int P, pb, warm, recStride; unsigned long long* cnt; };

// A flavour at kernel level: the device flavour F, whether the wave needs the 16 KiB LDS table, whether the blocks have an FxlBlk
// (k_fxl_prep in front) or only a segment length (kPfx: a.hcPfx, k_hc_ext_prep in front), the counters it bumps (blocks, rounds of
// the last call, pieces parsed again; kBlocksToo: a second block counter or -1), which blocks are the path's and what a block that
// is not gets as its result (round 1, piece 0).
struct KFx {                   // level 1, independent blocks (lz4_fx_device.inl)
    typedef FxFlavour<false> F;
    enum : int { kLds = 1, kHist = 0, kPfx = 0, kBlocks = 0, kRounds = 1, kAgain = 2, kBlocksToo = -1 };
    static DEVM F flavour(const FxlBlk&, uint32_t* lds) { return F{lds, 0}; }
    static DEVM bool in_scope(const CodecArgs& a, int n, const FxlBlk&) { return n >= kFxMinLen && n <= a.l1MaxLen; }
    // byU16 blocks, lengths the workspace was not sized for: the block as k_l1_parse does it
    static DEVM int outside(const CodecArgs& a, int n, int i, int gi, const FxlBlk&, uint32_t* lds, int* lastAnchor)
    {
        if (n < 0 || n > a.l1MaxLen) return -1;
        return wave_parse_l1<2>(a.src + (int64_t)gi * a.srcStride, n, lds, a.l1Seq + (int64_t)i * a.l1SeqStride, lastAnchor);
    }
};
struct KFxl {                  // level 1, history outside the block (the kExt flavour)
    typedef FxFlavour<true> F;
    enum : int { kLds = 1, kHist = 1, kPfx = 0, kBlocks = 0, kRounds = 1, kAgain = 2, kBlocksToo = 7 };
    static DEVM F flavour(const FxlBlk& b, uint32_t* lds) { return F{lds, b.bs}; }
    static DEVM bool in_scope(const CodecArgs&, int, const FxlBlk& b) { return b.pfx >= 0; }
    // not this path's: an empty parse (k_fxl_small writes the block behind the emit stage), or no result (-1, as k_l1_parse says it)
    static DEVM int outside(const CodecArgs&, int, int, int, const FxlBlk& b, uint32_t*, int*) { return b.pfx == -1 ? 0 : -1; }
};
struct KMx {                   // level 2, independent blocks (lz4_mx_device.inl): no LDS
    typedef MxFlavour F;
    enum : int { kLds = 0, kHist = 0, kPfx = 0, kBlocks = 13, kRounds = 14, kAgain = 15, kBlocksToo = -1 };
    static DEVM F flavour(const FxlBlk&, uint32_t*) { return F{}; }
    static DEVM bool in_scope(const CodecArgs& a, int n, const FxlBlk&) { return n >= 0 && n <= a.l1MaxLen; }
    // a block the workspace was not sized for: no result, as k_hc_mid says it
    static DEVM int outside(const CodecArgs&, int, int, int, const FxlBlk&, uint32_t*, int*) { return -1; }
};
struct KMxl {                  // level 2, history outside the block (MxlFlavour): no LDS, the segment's length out of a.hcPfx
    typedef MxlFlavour F;
    enum : int { kLds = 0, kHist = 0, kPfx = 1, kBlocks = 13, kRounds = 14, kAgain = 15, kBlocksToo = 16 };
    static DEVM F flavour(const FxlBlk& b, uint32_t*) { return F(b.pfx); }
    static DEVM bool in_scope(const CodecArgs& a, int n, const FxlBlk& b) { return n >= 0 && n <= a.l1MaxLen && b.pfx >= 0; }
    // a length the workspace was not sized for, or a block <= 4 KiB under a dictionary context (pfx -1: the emit stage lays it down
    // stored, hc_ctx_blocks writes it afterwards): no result, as k_hc_mid<true> says it
    static DEVM int outside(const CodecArgs&, int, int, int, const FxlBlk&, uint32_t*, int*) { return -1; }
};

template <class K> __device__ __forceinline__ void piece_body(const CodecArgs& a, const PieceArgs& f, const FxlBlk* xb, int round, uint32_t* lds)
{
    const int k = blockIdx.x, i = blockIdx.y, gi = a.blk0 + i;
    const int n = block_len(a, gi);
    FxlBlk b; b.pfx = 0; b.bs = 0;
    if (K::kHist) b = xb[i];                                                 // (loaded before anything is stored: scalar loads)
    if (K::kPfx) b.pfx = a.hcPfx[gi];
    if (!K::in_scope(a, n, b)) {
        if (round != 1 || k != 0) return;
        int lastAnchor = 0;
        const int nseq = K::outside(a, n, i, gi, b, lds, &lastAnchor);
        if ((threadIdx.x & 63u) == 0) { SeqInfo inf; inf.nseq = nseq; inf.lastAnchor = lastAnchor; inf.total = 0; inf.stored = 0; a.l1Info[i] = inf; }
        return;
    }
    typedef typename K::F F;
    const int64_t pb0 = (int64_t)i * f.P;
    piece_round(K::flavour(b, lds), a.src + (int64_t)gi * a.srcStride, n, k, round, f.pb, f.warm, f.meta + pb0, f.tabIn + pb0 * F::kTab,
                f.tabOut + pb0 * 2 * F::kTab, f.rec + pb0 * f.recStride, f.recStride);
}
template <class K> __global__ __launch_bounds__(64) void k_piece(CodecArgs a, PieceArgs f, const FxlBlk* xb, int round)
{
    if constexpr (K::kLds != 0) {
        __shared__ uint32_t lds[kHashBytes / 4];
        piece_body<K>(a, f, xb, round, lds);
    } else piece_body<K>(a, f, xb, round, nullptr);
}
template <class K> __global__ __launch_bounds__(64) void k_piece_gather(CodecArgs a, PieceArgs f, const FxlBlk* xb)
{
    const int k = blockIdx.x, i = blockIdx.y, gi = a.blk0 + i;
    const int n = block_len(a, gi);
    FxlBlk b; b.pfx = 0; b.bs = 0;
    if (K::kHist) b = xb[i];
    if (K::kPfx) b.pfx = a.hcPfx[gi];
    if (!K::in_scope(a, n, b) || k >= piece_count<K::F::kPiece0>(n, f.pb)) return;
    const int64_t pb0 = (int64_t)i * f.P;
    const PieceMeta* m = f.meta + pb0;
    const int g = piece_gather<K::F::kPiece0>(n, k, f.pb, m, f.rec + pb0 * f.recStride, f.recStride, a.l1Seq + (int64_t)i * a.l1SeqStride,
                                             (int)a.l1SeqStride - 1, a.l1Info + i);
    if ((threadIdx.x & 63u) == 0) {
        atomicMax(&f.cnt[K::kRounds], (unsigned long long)m[k].lastRound);
        if (m[k].runs > 1) atomicAdd(&f.cnt[K::kAgain], 1ull);
        if (g == 2) { atomicAdd(&f.cnt[K::kBlocks], 1ull); if (K::kBlocksToo >= 0) atomicAdd(&f.cnt[K::kBlocksToo], 1ull); }
    }
}
// in front of a call's first round: the "rounds of the last call" counter starts over
__global__ __launch_bounds__(64) void k_piece_begin(unsigned long long* cnt, int index) { if (threadIdx.x == 0) cnt[index] = 0; }

// grid (blocks of the group), one wave each: the segment in front of the block, piece 0's entry table, the block's FxlBlk
__global__ __launch_bounds__(64) void k_fxl_prep(CodecArgs a, PieceArgs f, FxlBlk* xb)
{
    __shared__ uint32_t lds[kHashBytes / 4];
    const int i = blockIdx.x, gi = a.blk0 + i;
    const int n = block_len(a, gi);
    FxlBlk b; b.pfx = -2; b.bs = 0;                                          // -2: a length the workspace was not sized for
    if (n >= 0 && n <= a.l1MaxLen) {
        const DictEnc dc = l1_prime_of(a, gi, n, a.rawMode != 0);
        b = fxl_prep(const_cast<uint8_t*>(a.src) + (int64_t)gi * a.srcStride, n, dc.mode, dc.dict, dc.dictSize, dc.dictTable,
                     f.tabIn + (int64_t)i * f.P * kFxTab, lds);
    }
    if ((threadIdx.x & 63u) == 0) xb[i] = b;
}
__global__ __launch_bounds__(256) void k_fxl_sizes(CodecArgs a, const FxlBlk* xb) { l1_sizes_body<true, true>(a, xb); }
__global__ __launch_bounds__(256) void k_fxl_write(CodecArgs a, const FxlBlk* xb) { l1_write_body<true, true>(a, xb); }
// Behind the emit stage: the blocks <= 4 KiB under a dictionary context (two tables, wave_encode_block_dict), as k_encode_rec_dict /
// k_encode_raw_dict write them -- record or block, checksum and result; what the emit stage wrote for them does not survive.
__global__ __launch_bounds__(64) void k_fxl_small(CodecArgs a)
{
    __shared__ uint32_t lds[kHashBytes / 4];
    for (int i = blockIdx.x; i < a.nBlocks; i += gridDim.x) {
        const int gi = a.blk0 + i;
        const int n = block_len(a, gi);
        if (n < 0 || n > kCtxMaxBlock) continue;
        const DictEnc dc = l1_prime_of(a, gi, n, a.rawMode != 0);
        if (dc.mode != kDictCtxLookup) continue;
        const uint8_t* s = a.src + (int64_t)gi * a.srcStride;
        if (!a.rawMode && a.bodyOff) {
            // records back to back: this launch runs between k_l1_scan and the scan over the records' lengths.  The block's bytes go
            // where its records would lie (it has none; bsz + 8 <= 8 bytes per possible sequence), its length to result, and the
            // emit stage's write and finish kernels lay it down as any other record (kSeqElsewhere).
            const int c = wave_encode_block_dict(s, n, (uint8_t*)(a.l1Seq + (int64_t)i * a.l1SeqStride), a.bsz, dc, lds);
            if ((threadIdx.x & 63u) == 0) {
                SeqInfo inf; inf.nseq = kSeqElsewhere; inf.lastAnchor = 0; inf.total = c; inf.stored = (c == 0); a.l1Info[i] = inf;
                a.result[gi] = (c ? c : n) + 4 + (a.blockChecksum ? 4 : 0);
            }
            continue;
        }
        encode_out(a, gi, s, n, a.rawMode != 0, [&](uint8_t* out, int cap) { return wave_encode_block_dict(s, n, out, cap, dc, lds); });
    }
}

// ---- many level-1 blocks with history outside the block (a linked frame or a dictionary frame from device-resident plaintext):
// the staged design with one wave per block, pulled from the block queue like k_l1_parse.  Each block is one exact whole-block run
// of the kExt parser (l1x_block, lz4_fx_device.inl): the segment in front of the block (copied only where it does not lie there
// already), the starting table built in the wave's own LDS table, the records into the level-1 workspace; xb[i] tells the kSeg emit
// stage (k_fxl_sizes / k_fxl_write) the segment's bytes.  W waves per workgroup, each with its own 16 KiB table, never synchronised
// (ENC_WAVE_TABLE): a whole-block run has none of the piece flow's live state (k_piece<KFxl>: 256 VGPRs + 92 AGPRs, one wave per SIMD)
// and fits the register budget of ten waves per CU (W = 10: 85 VGPRs, no AGPRs, no scratch), so the LDS tables are what bounds it,
// as with k_l1_parse.
template <int W> __global__ __launch_bounds__(64 * W) void k_l1x_parse(CodecArgs a, FxlBlk* xb, unsigned long long* cnt)
{
    ENC_WAVE_TABLE(lds);
    int parsed = 0;                                                          // (plz4hip_ctx_counters [8])
    for (int i = next_block(a.queue); i < a.nBlocks; i = next_block(a.queue)) {
        const int gi = a.blk0 + i;
        const int n  = block_len(a, gi);
        int lastAnchor = 0, nseq = -1;                                       // -1: a block the workspace was not sized for
        FxlBlk b; b.pfx = -2; b.bs = 0;
        if (n >= 0 && n <= a.l1MaxLen) {
            const DictEnc dc = l1_prime_of(a, gi, n, a.rawMode != 0);
            nseq = l1x_block(const_cast<uint8_t*>(a.src) + (int64_t)gi * a.srcStride, n, dc.mode, dc.dict, dc.dictSize, dc.dictTable,
                             a.l1Seq + (int64_t)i * a.l1SeqStride, (int)a.l1SeqStride - 1, &lastAnchor, &b, lds);
        }
        if ((threadIdx.x & 63u) == 0) {
            SeqInfo inf; inf.nseq = nseq; inf.lastAnchor = lastAnchor; inf.total = 0; inf.stored = 0; a.l1Info[i] = inf;
            xb[i] = b;
        }
        parsed += (b.pfx >= 0 && nseq >= 0);
    }
    if (parsed && (threadIdx.x & 63u) == 0) atomicAdd(&cnt[8], (unsigned long long)parsed);
}

// One record against an optional dictionary; shared by the independent and the linked decode kernels.
__device__ __forceinline__ void decode_one_record(const CodecArgs& a, int i, const uint8_t* dict, int dictLen, int* rOut, int* stOut, bool* stored, uint8_t* dl)
{
    const uint8_t* rec    = a.recOff ? a.src + a.recOff[i] : a.src + (int64_t)i * a.srcStride;
    const int64_t  recLen = a.recOff ? a.recOff[i + 1] - a.recOff[i] : (int64_t)a.srcLen[i];
    uint8_t*       out    = a.dst + (int64_t)i * a.dstStride;
    uint32_t       word;
    const int      sz     = rec_head<true>(rec, recLen, a.bsz, a.blockChecksum != 0, &word);
    int st = PLZ4HIP_BLK_OK, r = 0;
    *stored = false;
    if (sz < 0) {
        st = PLZ4HIP_BLK_SIZE_OVERFLOW;
    } else {
        if (a.blockChecksum) {
            const uint32_t want = plz4_readfirstlane(ld32u(rec + 4 + sz));
            if (wave_xxh32(rec + 4, sz) != want) st = PLZ4HIP_BLK_HASH_MISMATCH;
        }
        if (st == PLZ4HIP_BLK_OK) {
            if (word & 0x80000000u) {
                if (sz > a.dstCapAll) st = PLZ4HIP_BLK_SIZE_OVERFLOW;
                else { wave_copy(out, rec + 4, sz); r = sz; *stored = true; }
            } else {
                r = wave_decode_block<true>(rec + 4, sz, out, a.dstCapAll, dict, dictLen, dl);    // the batches are assembled in LDS, as in k_decode_rec
                if (r < 0) st = PLZ4HIP_BLK_CORRUPT;
            }
        }
    }
    *rOut = r; *stOut = st;
}

// Independent blocks with a dictionary (indieDecompressorWithDict, compress/decompress.go:42-58, linked == false).
__global__ __launch_bounds__(64) void k_decode_rec_dict(CodecArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t dl[kDecLdsBytes];
    for (int i = next_block(a.queue); i < a.nBlocks; i = next_block(a.queue)) {
        if (a.dxlGood && a.dxlGood[i]) continue;                             // (answered by the few-block path)
        int r, st; bool stored;
        decode_one_record(a, i, a.dict, a.dictLen, &r, &st, &stored, dl);
        if ((threadIdx.x & 63u) == 0) { a.result[i] = r; a.status[i] = st; }
    }
}

// Linked blocks: a serial chain, one wave (dxl_walk, lz4_dx_device.inl).  RecWave: its record decoder.
// The records [first, last) of chain ch from the window (winA, winLen) on; dead: an earlier record of the chain has failed.
static_assert((int)kDxlStCorrupt == (int)PLZ4HIP_BLK_CORRUPT && (int)PLZ4HIP_BLK_OK == 0, "dxl_walk's status codes");
struct RecWave {
    const CodecArgs& a; uint8_t* dl;
    __device__ __forceinline__ void operator()(int i, const uint8_t* hist, int histLen, int* r, int* st, bool* stored) const
    {
        decode_one_record(a, i, hist, histLen, r, st, stored, dl);
    }
};
// the chain's first and last record as the kernels' view of the call has them (a group's view: the call's chainFirst, clamped)
__device__ __forceinline__ int chain_lo(const CodecArgs& a, int ch)
{
    if (!a.chainFirst) return ch == 0 ? 0 : a.nBlocks;
    return dxl_chain_lo(a.chainFirst, a.dxlBlk0, a.nBlocks, ch);
}
__device__ __forceinline__ void linked_walk(const CodecArgs& a, const int ch, const int first, const int last, uint8_t* const win0,
                                            uint8_t* winA, uint8_t* winB, int winLen, bool dead, uint8_t* dl)
{
    DxlCall c{}; c.dst = a.dst; c.dstStride = a.dstStride;
    DxlFin f{}; f.result = a.result; f.status = a.status;
    RecWave rec{a, dl};
    int wl = winLen, dd = 0;
    dxl_walk(c, f, rec, first, last, win0, winA, winB, winLen, dead, &wl, &dd);
    if ((threadIdx.x & 63u) == 0) a.windowLen[ch] = wl;
}
__global__ __launch_bounds__(64) void k_decode_rec_linked(CodecArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t dl[kDecLdsBytes];
    // one wave per chain (frame); chains are independent of each other ("replicas"), the blocks of one chain are not
    for (int ch = next_block(a.queue); ch < a.nChains; ch = next_block(a.queue)) {
        const int first = a.chainFirst ? a.chainFirst[ch] : 0;
        const int last  = a.chainFirst ? a.chainFirst[ch + 1] : a.nBlocks;
        uint8_t* const win0 = a.window + (size_t)ch * 131072;
        linked_walk(a, ch, first, last, win0, win0, win0 + 65536, a.windowLen[ch], false, dl);
    }
}

__global__ __launch_bounds__(64) void k_decode_raw_dict(CodecArgs a)
{
    for (int i = next_block(a.queue); i < a.nBlocks; i = next_block(a.queue)) {
        if (a.dxlGood && a.dxlGood[i]) continue;                             // (answered by the few-block path)
        const int cap = cap_of(a, i);
        const int r = wave_decode_block(a.src + (int64_t)i * a.srcStride, a.srcLen[i], a.dst + (int64_t)i * a.dstStride, cap, a.dict, a.dictLen);
        if ((threadIdx.x & 63u) == 0) a.result[i] = r;
    }
}

// HC levels 2..12 (config 4 = level 12): LZ4_compress_HC per block; mode 0 = raw LZ4 block, 1 = frame record.
__device__ __forceinline__ HcWork hc_work_of(const CodecArgs& a)
{
    uint8_t* ws = a.hcWork + (size_t)blockIdx.x * kHcWorkBytes;
    HcWork w; w.hash = (uint32_t*)ws; w.chain = (uint16_t*)(ws + kHcHashEntries * 4);
    w.opt = (HcOpt*)(ws + kHcHashEntries * 4 + kHcChainEntries * 2); w.pre = nullptr; w.rank = nullptr; w.list = nullptr;
    return w;
}
// independent block without dictionary, the i-th of its group: its chain (and lists) were built up front when the call's
// launcher found room for them
__device__ __forceinline__ HcWork hc_with_pre(HcWork w, const CodecArgs& a, int i)
{
    w.pre = a.h12Chain ? a.h12Chain + (int64_t)i * a.h12ChainStride : nullptr;
    w.rank = (a.h12Chain && a.h12Rank) ? a.h12Rank + (int64_t)i * a.h12ChainStride : nullptr;
    w.list = (a.h12Chain && a.h12Rank) ? a.h12List + (int64_t)i * (a.h12ChainStride + 8) + 8 : nullptr;
    return w;
}
// One thread of search per block: raw LZ4 blocks (kRaw) or records.  hcEx: the call has a dictionary and / or linked blocks.
template <bool kRaw> __device__ __forceinline__ void hc_one_thread(const CodecArgs& a)
{
    const HcWork w = hc_work_of(a);
    for (int g = next_block(a.queue); g < a.nBlocks; g = next_block(a.queue)) {
        const int      i = a.blk0 + g;                                   // (the chain / lists workspace is the group's: index g)
        const int      n = block_len(a, i);
        const uint8_t* s = a.src + (int64_t)i * a.srcStride;
        if (a.hcPfx && a.hcPfx[i] >= 0) continue;                          // (done on the list path)
        if (a.hcx && hc_is_ctx(a, i, n, kRaw)) continue;                   // (k_hcx's)
        encode_out(a, i, s, n, kRaw, [&](uint8_t* out, int cap) {
            if (a.hcEx) return hc_compress(s, n, out, cap, a.level, w, hc_prime_of(a, i, n, s, kRaw));
            return hc_compress(s, n, out, cap, a.level, hc_with_pre(w, a, g));
        });
    }
}
__global__ __launch_bounds__(64) void k_encode_raw_hc(CodecArgs a) { hc_one_thread<true>(a); }
__global__ __launch_bounds__(64) void k_encode_rec_hc(CodecArgs a) { hc_one_thread<false>(a); }

// HC levels 2..12, the blocks <= 4 KiB under a dictionary context (usingDictCtxHc) of a call: one wave per block off the block queue,
// the block's lists in LDS (17 KiB: nine waves per CU), the dictionary's lists read-only, nothing else in device memory but the
// price table of levels 10..12 (lz4hcx_device.inl).  kRaw: LZ4 blocks (dstCap per block), else records [size word][payload][xxh32?] with the stored fallback, as
// k_encode_rec_hc writes them.  Blocks of any other kind are not its business.  cnt[9]: the blocks it encoded.
// kMid: level 2 -- its two tables in LDS instead (21 KiB: seven waves per CU), its sequence records where the price table would be.
template <bool kRaw, bool kMid> __global__ __launch_bounds__(64) void k_hcx(CodecArgs a, unsigned long long* cnt)
{
    __shared__ typename std::conditional<kMid, HcxMidLds, HcxLds>::type lds;
    HcOpt* const opt = (kMid || a.level >= 10) ? hc_work_of(a).opt : nullptr;   // (levels 10..12: the wave's price table)
    const auto compress = [&](const uint8_t* s, int n, uint8_t* out, int cap, const HcxDict& d) {
        if constexpr (kMid) return hcx_mid_block(s, n, out, cap, lds, d, a.hcDictHash, (uint64_t*)opt);
        else return hcx_compress(s, n, out, cap, a.level, lds, d, opt);
    };
    HcxDict d; d.bytes = a.dict; d.len = a.dictLen > 0 ? a.dictLen : 0; d.start = a.hcxStart; d.list = (a.dict && d.len > 0) ? a.hcxList : nullptr;
    int done = 0;
    for (int i = next_block(a.queue); i < a.nBlocks; i = next_block(a.queue)) {
        const int n = block_len(a, i);
        if (a.hcPfx ? a.hcPfx[i] != -1 : !hc_is_ctx(a, i, n, kRaw)) continue;
        if (n < 0) { if (kRaw && (threadIdx.x & 63u) == 0) a.result[i] = 0; continue; }      // (LZ4_compress_HC: 0)
        const uint8_t* s = a.src + (int64_t)i * a.srcStride;
        uint8_t* const out = a.dst + (int64_t)i * a.dstStride;
        ++done;
        // (its loop body as it always was, the writer called directly and not through encode_out: the parsers in this kernel live on
        // spilled scalars, and the body's shape decides where they are reloaded -- profiles/block_io_resources.txt)
        if (kRaw) {
            const int r = compress(s, n, out, cap_of(a, i), d);
            if ((threadIdx.x & 63u) == 0) a.result[i] = r;
            continue;
        }
        const int c = compress(s, n, out + 4, a.bsz, d);    // capacity == bsz (blk.go:73)
        const int len = wave_finish_record(out, s, n, c, a.blockChecksum != 0);
        if ((threadIdx.x & 63u) == 0) a.result[i] = len;
    }
    if (done && (threadIdx.x & 63u) == 0) atomicAdd(&cnt[9], (unsigned long long)done);
}

// HC levels 3..12 with a dictionary and/or linked blocks on the list path (round 4): how every block of the call is primed
// (hc_prime), its external segment copied right in front of it, its length noted (hc_pfx: no segment and no context -- the first
// block of a linked frame without a dictionary -- is an empty segment).  One wave per block.
__global__ __launch_bounds__(64) void k_hc_ext_prep(CodecArgs a)
{
    for (int i = next_block(a.queue); i < a.nBlocks; i = next_block(a.queue)) {
        const int pfx = hc_pfx(hc_prime_of(a, i, block_len(a, i), a.src + (int64_t)i * a.srcStride, a.rawMode != 0));
        if ((threadIdx.x & 63u) == 0) a.hcPfx[i] = pfx;
    }
}
// the segment length of block i of an HC call (0: none), and the positions in front of the block that are never inserted
__device__ __forceinline__ int hc_pfx_of(const CodecArgs& a, int i) { return a.hcPfx ? a.hcPfx[i] : 0; }

// ---------------------------------------------------------------------------------------------- HC level 12, three phases
// Phase 1a: how many positions every hash has, then where its run starts in the list (exclusive prefix sum).  One 16-wave
// workgroup per block, the 32768 counters in LDS.
__global__ __launch_bounds__(1024) void k_hc12_hist(CodecArgs a)
{
    __shared__ uint32_t hist[kHcHashEntries];
    __shared__ uint32_t part[1024];
    __shared__ int cur;
    const int tid = (int)threadIdx.x;
    for (;;) {
        if (tid == 0) cur = (int)atomicAdd(a.queue, 1u);
        __syncthreads();
        const int g = cur;
        if (g >= a.nBlocks) break;
        const int i = a.blk0 + g;
        const int pfx = hc_pfx_of(a, i);                                   // (an external segment in front of the block: positions count from its first byte)
        if (pfx < 0) { __syncthreads(); continue; }
        const int n = pfx + block_len(a, i);
        const uint8_t* const src = a.src + (int64_t)i * a.srcStride - pfx;
        for (int h = tid; h < kHcHashEntries; h += 1024) hist[h] = 0u;
        __syncthreads();
        const int nIns = n >= 4 ? n - 3 : 0;
        const int skipLo = pfx > 3 ? pfx - 3 : 0;                           // the segment's last three positions are never inserted (lz4hc.c:1660-1678)
        for (int p = tid; p < nIns; p += 1024) if (p < skipLo || p >= pfx) atomicAdd(&hist[hc12_hash(ld32u(src + p))], 1u);
        __syncthreads();
        uint32_t sum = 0;
        for (int k = 0; k < 32; ++k) sum += hist[tid * 32 + k];
        part[tid] = sum;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            const uint32_t v = (tid >= d) ? part[tid - d] : 0u;
            __syncthreads();
            part[tid] += v;
            __syncthreads();
        }
        uint32_t run = part[tid] - sum;
        uint32_t* const off = a.h12Offsets + (size_t)g * kHcHashEntries;
        for (int k = 0; k < 32; ++k) { const uint32_t c = hist[tid * 32 + k]; off[tid * 32 + k] = run; run += c; }
        __syncthreads();
    }
}

// Phase 1b: chain, rank and list of every block of the group.  One wave per workgroup, two 64 KiB tables in LDS.
__global__ __launch_bounds__(64) void k_hc12_chain(CodecArgs a)
{
    __shared__ uint32_t lastT[kHcHashEntries / 2];
    __shared__ uint32_t curT[kHcHashEntries / 2];
    for (int g = next_block(a.queue); g < a.nBlocks; g = next_block(a.queue)) {
        const int i = a.blk0 + g;
        const int pfx = hc_pfx_of(a, i);
        if (pfx < 0) continue;
        const int n = pfx + block_len(a, i);
        int nPad = (n + 1 + 1023) & ~1023;
        if (nPad > a.h12ChainStride) nPad = (int)a.h12ChainStride;
        hc12_build_lists(a.src + (int64_t)i * a.srcStride - pfx, n, a.h12Offsets + (size_t)g * kHcHashEntries,
                         a.h12Chain + (int64_t)g * a.h12ChainStride, a.h12Rank + (int64_t)g * a.h12ChainStride,
                         a.h12List + (int64_t)g * (a.h12ChainStride + 8) + 8, nPad, lastT, curT, pfx > 3 ? pfx - 3 : 0, pfx);
    }
}

// Phase 1 of a few blocks, in pieces across the chip (lz4hc_lists_device.inl): the same offsets, chain, rank and list as the two
// kernels above, by four launches in which nobody waits for anybody.  cnt / slot: [block of the group][piece][hash].
struct HbArgs { uint32_t* cnt; uint32_t* slot; int P, piece; unsigned long long* counters; };
struct HbBlk { const uint8_t* src; int n, nIns, pfx, skipLo, pieces; };
// block g of the group as the builder sees it: segment + block, the positions that are inserted, its own number of pieces
__device__ __forceinline__ bool hb_blk(const CodecArgs& a, const HbArgs& hb, int g, HbBlk* b)
{
    const int i = a.blk0 + g;
    b->pfx = hc_pfx_of(a, i);
    if (b->pfx < 0) return false;                                          // (k_hcx's, as for k_hc12_hist)
    b->n = b->pfx + block_len(a, i);
    b->src = a.src + (int64_t)i * a.srcStride - b->pfx;
    b->nIns = b->n >= 4 ? b->n - 3 : 0;
    b->skipLo = b->pfx > 3 ? b->pfx - 3 : 0;
    b->pieces = (b->nIns + hb.piece - 1) / hb.piece;
    if (b->pieces > hb.P) b->pieces = hb.P;                                // (never: P is cut from the call's largest segment + block)
    return true;
}
// count: one 16-wave workgroup per (piece, block), the piece's 32768 counters in LDS, then out to cnt
__global__ __launch_bounds__(1024) void k_hb_count(CodecArgs a, HbArgs hb)
{
    __shared__ uint32_t hist[kHcHashEntries];
    const int tid = (int)threadIdx.x, g = (int)blockIdx.y, k = (int)blockIdx.x;
    HbBlk b;
    if (!hb_blk(a, hb, g, &b) || k >= b.pieces) return;
    for (int h = tid; h < kHcHashEntries; h += 1024) hist[h] = 0u;
    __syncthreads();
    const int lo = k * hb.piece, hi = lo + hb.piece;
    hb_count(b.src, b.nIns, b.skipLo, b.pfx, lo + (tid & ~63), hi, 1024, hist);
    __syncthreads();
    uint32_t* const out = hb.cnt + ((size_t)g * hb.P + k) * kHcHashEntries;
    for (int h = tid; h < kHcHashEntries; h += 1024) out[h] = hist[h];
}
// scan: one workgroup per block.  A thread per hash adds up the pieces (neighbouring threads, neighbouring words); the prefix over
// the 32768 totals as in k_hc12_hist; then every piece's first slot.
__global__ __launch_bounds__(1024) void k_hb_scan(CodecArgs a, HbArgs hb)
{
    __shared__ uint32_t hist[kHcHashEntries];
    __shared__ uint32_t part[1024];
    const int tid = (int)threadIdx.x, g = (int)blockIdx.x;
    HbBlk b;
    if (!hb_blk(a, hb, g, &b)) return;
    const uint32_t* const cnt = hb.cnt + (size_t)g * hb.P * kHcHashEntries;
    uint32_t* const slot = hb.slot + (size_t)g * hb.P * kHcHashEntries;
    for (int h = tid; h < kHcHashEntries; h += 1024) hist[h] = hb_total(cnt, b.pieces, h);
    __syncthreads();
    uint32_t sum = 0;
    for (int k = 0; k < 32; ++k) sum += hist[tid * 32 + k];
    part[tid] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const uint32_t v = (tid >= d) ? part[tid - d] : 0u;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    uint32_t run = part[tid] - sum;
    uint32_t* const off = a.h12Offsets + (size_t)g * kHcHashEntries;
    for (int k = 0; k < 32; ++k) { const uint32_t c = hist[tid * 32 + k]; off[tid * 32 + k] = run; hist[tid * 32 + k] = run; run += c; }
    __syncthreads();
    for (int h = tid; h < kHcHashEntries; h += 1024) hb_slots(cnt, slot, b.pieces, h, hist[h]);
    if (tid == 0) { atomicAdd(&hb.counters[17], 1ull); hb.counters[18] = (unsigned long long)hb.P; }
}
// fill: one wave per (piece, block) around two 64 KiB tables in LDS
__global__ __launch_bounds__(64) void k_hb_fill(CodecArgs a, HbArgs hb)
{
    __shared__ uint32_t lastT[kHcHashEntries / 2];
    __shared__ uint32_t curT[kHcHashEntries / 2];
    const int g = (int)blockIdx.y, k = (int)blockIdx.x;
    HbBlk b;
    if (!hb_blk(a, hb, g, &b) || k >= b.pieces) return;
    hb_fill(b.src, b.n, a.h12Offsets + (size_t)g * kHcHashEntries, hb.slot + ((size_t)g * hb.P + k) * kHcHashEntries,
            a.h12Rank + (int64_t)g * a.h12ChainStride, a.h12List + (int64_t)g * (a.h12ChainStride + 8) + 8,
            k * hb.piece, (k + 1) * hb.piece, lastT, curT, b.skipLo, b.pfx);
}
// chain: a wave per 64 positions of [0, nPad), nPad as k_hc12_chain has it
__global__ __launch_bounds__(256) void k_hb_chain(CodecArgs a, HbArgs hb)
{
    const int g = (int)blockIdx.y;
    HbBlk b;
    if (!hb_blk(a, hb, g, &b)) return;
    int nPad = (b.n + 1 + 1023) & ~1023;
    if (nPad > a.h12ChainStride) nPad = (int)a.h12ChainStride;
    for (int base = (int)(blockIdx.x * 256u + (threadIdx.x & ~63u)); base < nPad; base += (int)gridDim.x * 256)
        hb_chain(b.n, b.skipLo, b.pfx, a.h12Chain + (int64_t)g * a.h12ChainStride, a.h12Rank + (int64_t)g * a.h12ChainStride,
                 a.h12List + (int64_t)g * (a.h12ChainStride + 8) + 8, base);
}

// The chain alone, for levels 3..11 (HcWork::pre): one pass per block with the whole 128 KiB table in LDS.
__global__ __launch_bounds__(64) void k_hc_chain(CodecArgs a)
{
    __shared__ uint32_t tab[kHcHashEntries];
    for (int g = next_block(a.queue); g < a.nBlocks; g = next_block(a.queue)) {
        const int i = a.blk0 + g;
        const int n = block_len(a, i);
        int nPad = (n + 1 + 1023) & ~1023;
        if (nPad > a.h12ChainStride) nPad = (int)a.h12ChainStride;
        hc12_build_chain(a.src + (int64_t)i * a.srcStride, n, a.h12Chain + (int64_t)g * a.h12ChainStride, nPad, tab);
    }
}

// Phase 2: F(p) for the positions of every block of the group.  One 16-wave workgroup per block at a time; the 64 KiB of source
// behind the positions in flight (and what lies ahead of them) sit in a 128 KiB ring in LDS, fed 1 KiB at a time; the chains
// come from the lists of phase 1.  Every lane runs one position (Hc12Walk); a loop trip runs each phase's code once for the
// lanes that are in it; a lane that has finished takes the next position from the block's queue, so lanes never wait for the
// longest search of their wave.
struct Hc12Ctl { int qNext; int loaded; int skipUntil; int lock; int waveMin[16]; int cur; };

__device__ __forceinline__ int h12_wave_min(int v)
{
    const int big = 0x7FFFFFFF;
    int t;
    t = __builtin_amdgcn_update_dpp(big, v, 0x111, 0xF, 0xF, false); v = v < t ? v : t;
    t = __builtin_amdgcn_update_dpp(big, v, 0x112, 0xF, 0xF, false); v = v < t ? v : t;
    t = __builtin_amdgcn_update_dpp(big, v, 0x114, 0xF, 0xF, false); v = v < t ? v : t;
    t = __builtin_amdgcn_update_dpp(big, v, 0x118, 0xF, 0xF, false); v = v < t ? v : t;
    t = __builtin_amdgcn_update_dpp(big, v, 0x142, 0xA, 0xF, false); v = v < t ? v : t;
    t = __builtin_amdgcn_update_dpp(big, v, 0x143, 0xC, 0xF, false); v = v < t ? v : t;
    return __builtin_amdgcn_readlane(v, 63);
}
#define H12_LD(x)     (*(volatile int*)&(x))
#define H12_ST(x, v)  (*(volatile int*)&(x) = (v))
#define H12_ORDER()   __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup")

__global__ __launch_bounds__(1024) void k_hc12_search(CodecArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t ring[kHc12SrcRing + kHc12SrcRingPad];
    __shared__ Hc12Ctl ctl;
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (;;) {
        if (tid == 0) ctl.cur = (int)atomicAdd(a.queue, 1u);
        __syncthreads();
        const int g = ctl.cur;
        if (g >= a.nBlocks) break;
        const int i = a.blk0 + g;
        const int n = block_len(a, i);
        Hc12Tabs t;
        t.src = a.src + (int64_t)i * a.srcStride;
        t.chain = a.h12Chain + (int64_t)g * a.h12ChainStride;
        t.rank = a.h12Rank + (int64_t)g * a.h12ChainStride;
        t.list = a.h12List + (int64_t)g * (a.h12ChainStride + 8) + 8;
        Hc12F* const F = a.h12F + (int64_t)g * a.h12FStride;
        const int nPos = n - kMfLimit + 1 > 0 ? n - kMfLimit + 1 : 0;                // positions the parser can search
        if (tid == 0) { ctl.qNext = 0; ctl.loaded = 0; ctl.skipUntil = 0; ctl.lock = 0; }
        if (tid < 16) ctl.waveMin[tid] = 0;
        __syncthreads();

        Hc12SrcRing sw; sw.ring = ring; sw.g = t.src; sw.hi = 0;
        STAT_DECL;                              // diagnostics build: cycles and lane counts per section (scripts/stats_probe12.py)
        const unsigned long long tS0 = STAT_NOW(); (void)tS0;
        Hc12Walk<Hc12SrcRing> L;
        L.phase = kPhIdle;                      // kPhIdle: wants a position; kPhWait: holds p, its bytes are not in the ring yet
        int p = 0;
        unsigned idleTrips = 0;
        auto finish = [&]() {                   // the lane's search has ended: publish F(p)
            const Hc12F f = L.result();
            F[p] = f;
            if (f.len > kHc12Sufficient + 8) atomicMax(&ctl.skipUntil, p + f.len - kHc12Sufficient);
        };
        for (;;) {
            const uint64_t mF = __builtin_amdgcn_ballot_w64(L.phase == kPhFilter);
            const uint64_t mC = __builtin_amdgcn_ballot_w64(L.phase == kPhCount);
            const uint64_t mS = __builtin_amdgcn_ballot_w64(L.phase == kPhScan);
            const uint64_t mK = __builtin_amdgcn_ballot_w64(L.phase == kPhRank);
            const uint64_t mP = __builtin_amdgcn_ballot_w64(L.phase == kPhPattern);
            const uint64_t mI = __builtin_amdgcn_ballot_w64(L.phase == kPhIdle || L.phase == kPhWait);
            const bool busy = (mF | mC | mS | mK | mP) != 0;
            const unsigned long long tq0 = STAT_NOW(); (void)tq0;
            if (mI && (__builtin_popcountll(mI) >= a.h12Idle || !busy)) { SSTAT(13, 1);
                // (1) this wave's lower bound on the positions it holds or may still take: published BEFORE it takes new ones
                const int q0 = H12_LD(ctl.qNext);
                int m = h12_wave_min((L.phase != kPhIdle && L.phase != kPhDone) ? p : 0x7FFFFFFF);
                if (q0 < m) m = q0;
                if (lane == 0) H12_ST(ctl.waveMin[wv], m);
                H12_ORDER();
                // (2) keep the ring ahead of the queue: one wave at a time loads the next KiBs.  The ring must still hold the
                // 64 KiB behind every position in flight or yet to be taken: loaded - ring <= min(p) - 65535.
                int loaded = H12_LD(ctl.loaded);
                if (loaded < n && loaded < q0 + 8192) {
                    int got = 0;
                    if (lane == 0) got = atomicCAS(&ctl.lock, 0, 1) == 0;
                    if (__builtin_amdgcn_readfirstlane(got)) {
                        loaded = H12_LD(ctl.loaded);
                        const int qn = H12_LD(ctl.qNext);               // first the queue head, then the waves' bounds
                        H12_ORDER();
                        int mn = h12_wave_min(lane < 16 ? H12_LD(ctl.waveMin[lane]) : 0x7FFFFFFF);
                        if (qn < mn) mn = qn;
                        while (loaded < n && loaded < qn + 16384 && loaded + 1024 <= mn + 65536) {
                            const int at = loaded + lane * 16;
                            uint8_t* d = ring + (at & (kHc12SrcRing - 1));
                            if (at + 16 <= n) {
                                const uint4 v = *(const uint4*)(t.src + at);
                                *(uint4*)d = v;
                                if ((at & (kHc12SrcRing - 1)) == 0) *(uint4*)(ring + kHc12SrcRing) = v;           // the mirror behind the ring's end
                            } else for (int k = 0; k < 16; ++k) if (at + k < n) { d[k] = t.src[at + k]; if ((at & (kHc12SrcRing - 1)) == 0) ring[kHc12SrcRing + k] = d[k]; }
                            loaded += 1024;
                        }
                        H12_ORDER();
                        if (lane == 0) { H12_ST(ctl.loaded, loaded); H12_ORDER(); atomicExch(&ctl.lock, 0); }
                    }
                }
                // (3) idle lanes take the next positions
                const uint64_t idle = __builtin_amdgcn_ballot_w64(L.phase == kPhIdle);
                if (idle) {
                    const int first = __builtin_ctzll(idle);
                    int base = 0;
                    if (lane == first) base = atomicAdd(&ctl.qNext, __builtin_popcountll(idle));
                    base = __builtin_amdgcn_readlane(base, first);
                    if (L.phase == kPhIdle) {
                        p = base + __builtin_popcountll(idle & ((1ull << lane) - 1));
                        L.phase = p < nPos ? kPhWait : kPhDone;
                        // (the block's last positions -- no wide loads there -- are the parser's)
                        if (p < nPos && p + 32 > n) { Hc12F f; f.len = kHc12NotComputed; f.off = 0; F[p] = f; L.phase = kPhIdle; }
                    }
                }
                // (4) a lane starts its position once the bytes around it are in the ring; positions inside a match longer than
                // the parser's "sufficient" length are left to the parser (it jumps over them, lz4hc.c:1871-1882)
                loaded = H12_LD(ctl.loaded);
                const int skip = H12_LD(ctl.skipUntil);
                sw.hi = (uint32_t)(loaded < n ? loaded : n);
                if (L.phase == kPhWait) {
                    if (p < skip) { Hc12F f; f.len = kHc12NotComputed; f.off = 0; F[p] = f; L.phase = kPhIdle; }
                    else if (p + 64 <= loaded || loaded >= n) L.init(t, sw, n, p, (uint32_t)t.chain[p]);
                }
            }
            if (!__builtin_amdgcn_ballot_w64(L.phase != kPhDone)) break;
            SSTAT(12, STAT_NOW() - tq0);
            sw.hi = (uint32_t)min(H12_LD(ctl.loaded), n);
            // One phase's code per section.  A section costs the same whether 3 or 60 lanes are in it, so it runs when enough
            // lanes have gathered; when no phase has that many, the fullest one runs (nothing ever waits for good).
            {
                const int cF = __builtin_popcountll(mF), cC = __builtin_popcountll(mC), cS = __builtin_popcountll(mS),
                          cK = __builtin_popcountll(mK), cP = __builtin_popcountll(mP);
                int top = cF; top = cC > top ? cC : top; top = cS > top ? cS : top; top = cK > top ? cK : top; top = cP > top ? cP : top;
                const int need = top < a.h12Gather ? top : a.h12Gather;
                unsigned long long tx = STAT_NOW(); (void)tx;
                if (cF && cF >= need) {
                    SSTAT(0, 1); SSTAT(1, cF);
                    const bool fl = L.phase == kPhFilter;
                    if (__builtin_amdgcn_ballot_w64(fl && !L.is_near())) { if (fl && !L.is_near() && L.filter_trip<false>(t, sw)) finish(); }
                    if (fl && L.is_near() && L.filter_trip<true>(t, sw)) finish();
                    SSTAT(2, STAT_NOW() - tx); tx = STAT_NOW();
                }
                if (cC && cC >= need) { SSTAT(3, 1); SSTAT(4, cC); if (L.phase == kPhCount) L.count_trip(t, sw); SSTAT(5, STAT_NOW() - tx); tx = STAT_NOW(); }
                if (cS && cS >= need) { SSTAT(6, 1); SSTAT(7, cS); if (L.phase == kPhScan && L.scan_trip(t)) finish(); SSTAT(8, STAT_NOW() - tx); tx = STAT_NOW(); }
                if (cK && cK >= need) { SSTAT(9, 1); SSTAT(10, cK); if (L.phase == kPhRank) L.rank_trip(t); SSTAT(11, STAT_NOW() - tx); tx = STAT_NOW(); }
                if (cP && cP >= need) { if (L.phase == kPhPattern && L.pattern_trip(t, sw)) finish(); }
            }
            if (!busy) {
                __builtin_amdgcn_s_sleep(2);
                if (++idleTrips > (1u << 27)) { if (lane == 0) atomicExch(a.h12Err, 1); break; }      // never seen; bounds every spin
            } else idleTrips = 0;
            SSTAT(14, 1);
        }
        SSTAT(15, STAT_NOW() - tS0); SSTAT(16, 1);
        SSTAT_FLUSH();
        __syncthreads();
    }
}

// Phase 3: the parser + writer + record framing, one wave per block.  The first kH12OptLds entries of the price table are in LDS.
constexpr int kH12OptLds = 1024;
__global__ __launch_bounds__(64) void k_hc12_parse(CodecArgs a)
{
    __shared__ Hc12Ent  oEnt[kH12OptLds];
    __shared__ uint64_t seqs[64];
    Hc12Ws w;
    w.ent = oEnt; w.nl = kH12OptLds; w.seq = seqs;
    {
        uint8_t* gws = a.h12Ws + (size_t)blockIdx.x * kHc12WsGlobalBytes;
        w.gprice = (int*)gws; w.glitlen = (int*)(gws + kHc12OptEntries * 4); w.gmloff = (uint32_t*)(gws + kHc12OptEntries * 8);
    }
    for (int g = next_block(a.queue); g < a.nBlocks; g = next_block(a.queue)) {
        const int i = a.blk0 + g;
        const int      n   = block_len(a, i);
        const uint8_t* s   = a.src + (int64_t)i * a.srcStride;
        const Hc12F*   F   = a.h12F + (int64_t)g * a.h12FStride;
        const uint16_t* ch = a.h12Chain + (int64_t)g * a.h12ChainStride;
        if (plz4_readfirstlane(*(volatile int32_t*)a.h12Err)) {               // the search kernel gave up on this group (spin guard):
            if ((threadIdx.x & 63u) == 0) a.result[i] = PLZ4HIP_E_DEVICE;     // its F is not to be trusted -- an engine failure, not a result
            continue;
        }
        encode_out(a, i, s, n, a.rawMode != 0, [&](uint8_t* out, int cap) { return hc12_parse(s, n, out, cap, F, ch, w); });
    }
}

// Levels 3..9 on independent blocks (lz4hc_lazy_device.inl), the chain and the lists being there.  k_hc_lazy: one wave per
// (block, segment) walks its segment and writes records; k_hc_stitch: one wave per block joins the segments' walks into the
// one walk from position 0; k_hc_gather lays the pieces out as one array; the emit kernels of level 1 (k_l1_sizes<false> ..
// k_l1_finish) make the block from it.
__device__ __forceinline__ HcWork lz_work(const CodecArgs& a, int g)
{
    HcWork w; w.hash = nullptr; w.chain = nullptr; w.opt = nullptr; w.pre = nullptr; w.rank = nullptr; w.list = nullptr;
    if (a.level >= 10) w.opt = hc_work_of(a).opt;                           // levels 10..11: the wave's price table (its slot of the HC workspace)
    return hc_with_pre(w, a, g);
}
// kD: the call's blocks have external segments in front of them (a.hcPfx: dictionary / linked blocks, every level 3..12; lz4hc.c:
// 1438-1461, :1626-1720); chain and lists then cover segment + block.  A kernel of its own, so that the independent blocks'
// kernel does not carry the segment rules (and level 12's parameters).
template <bool kD> __global__ __launch_bounds__(64) void k_hc_lazy(CodecArgs a)
{
    const int items = a.nBlocks * a.lzSegs;
    const bool broken = plz4_readfirstlane(*(volatile int32_t*)a.h12Err) != 0;
    for (int it = next_block(a.queue); it < items; it = next_block(a.queue)) {
        const int g = it / a.lzSegs, j = it - g * a.lzSegs;                  // (a block's segments are taken one after the other)
        const int i = a.blk0 + g;
        const int n = block_len(a, i);
        const int pfx = kD ? hc_pfx_of(a, i) : 0;
        if (broken || n < 0 || n > a.l1MaxLen || pfx < 0) continue;
        const int segs = lz_segments(n, a.lzSegs, a.lzMinSeg);
        if (j >= segs) continue;
        hc_lazy_segment<kD>(a.src + (int64_t)i * a.srcStride, n, a.level, lz_work(a, g), segs, j,
                            a.lzRec + (int64_t)g * a.lzRecStride, a.lzMeta + (int64_t)g * a.lzSegs, a.lzStarts + (int64_t)g * a.lzSegs * kLzStarts, pfx);
    }
}
template <bool kD> __global__ __launch_bounds__(64) void k_hc_stitch(CodecArgs a)
{
    const bool broken = plz4_readfirstlane(*(volatile int32_t*)a.h12Err) != 0;
    for (int g = next_block(a.queue); g < a.nBlocks; g = next_block(a.queue)) {
        const int i = a.blk0 + g;
        const int n = block_len(a, i);
        LzPiece* const pieces = a.lzPieces + (int64_t)g * 2 * a.lzSegs;
        int lastAnchor = 0, nseq = -1, segs = 0;                             // -1: a block the workspace was not sized for, or one that is not this path's
        const int pfx = kD ? hc_pfx_of(a, i) : 0;
        if (broken) nseq = kSeqEngineFailed;                                 // the search phase gave up: its F is not to be trusted
        else if (n >= 0 && n <= a.l1MaxLen && pfx >= 0) {
            segs = lz_segments(n, a.lzSegs, a.lzMinSeg);
            nseq = hc_lazy_stitch<kD>(a.src + (int64_t)i * a.srcStride, n, a.level, lz_work(a, g), segs,
                                      a.lzRec + (int64_t)g * a.lzRecStride, a.lzBridge + (int64_t)g * a.lzRecStride,
                                      a.lzMeta + (int64_t)g * a.lzSegs, a.lzStarts + (int64_t)g * a.lzSegs * kLzStarts, pieces, &lastAnchor, pfx);
        }
        if ((threadIdx.x & 63u) == 0) {
            for (int k = 2 * segs; k < 2 * a.lzSegs; ++k) pieces[k].cnt = 0;
            SeqInfo inf; inf.nseq = nseq; inf.lastAnchor = lastAnchor; inf.total = 0; inf.stored = 0; a.l1Info[g] = inf;
        }
    }
}
// grid (workgroups per block, blocks of the group)
__global__ __launch_bounds__(256) void k_hc_gather(CodecArgs a)
{
    const int g = blockIdx.y;
    const LzPiece* const pieces = a.lzPieces + (int64_t)g * 2 * a.lzSegs;
    uint64_t* const seq = a.l1Seq + (int64_t)g * a.l1SeqStride;
    const int t = blockIdx.x * 256 + (int)threadIdx.x, nT = gridDim.x * 256;
    for (int k = 0; k < 2 * a.lzSegs; ++k) {
        const LzPiece pc = pieces[k];
        for (int e = t; e < pc.cnt; e += nT) seq[pc.dst + e] = pc.src[e];
    }
}

// Level 12 up to 4 MiB: its parser (the price DP over F, lz4hc12_device.inl) walked in segments and stitched like levels 3..11,
// records out.  The price table's LDS part is 256 entries here (4 KiB: windows beyond that spill to the wave's global slot), so
// that registers, not LDS, bound the waves per CU.
constexpr int kH12SegLds = 256;
__device__ __forceinline__ Hc12Ws h12_seg_ws(const CodecArgs& a, Hc12Ent* ent, uint64_t* seqs)
{
    Hc12Ws w; w.ent = ent; w.nl = kH12SegLds; w.seq = seqs;
    uint8_t* gws = a.h12Ws + (size_t)blockIdx.x * kHc12WsGlobalBytes;
    w.gprice = (int*)gws; w.glitlen = (int*)(gws + kHc12OptEntries * 4); w.gmloff = (uint32_t*)(gws + kHc12OptEntries * 8);
    return w;
}
__global__ __launch_bounds__(64) void k_hc12_seg(CodecArgs a)
{
    __shared__ Hc12Ent oEnt[kH12SegLds];
    __shared__ uint64_t seqs[64];
    const Hc12Ws w = h12_seg_ws(a, oEnt, seqs);
    const int items = a.nBlocks * a.lzSegs;
    const bool broken = plz4_readfirstlane(*(volatile int32_t*)a.h12Err) != 0;
    for (int it = next_block(a.queue); it < items; it = next_block(a.queue)) {
        const int g = it / a.lzSegs, j = it - g * a.lzSegs;
        const int i = a.blk0 + g;
        const int n = block_len(a, i);
        if (broken || n < 0 || n > a.l1MaxLen) continue;
        const int segs = lz_segments(n, a.lzSegs, a.lzMinSeg);
        if (j >= segs) continue;
        hc12_segment(a.src + (int64_t)i * a.srcStride, n, a.h12F + (int64_t)g * a.h12FStride, a.h12Chain + (int64_t)g * a.h12ChainStride, w, segs, j,
                     a.lzRec + (int64_t)g * a.lzRecStride, a.lzMeta + (int64_t)g * a.lzSegs, a.lzStarts + (int64_t)g * a.lzSegs * kLzStarts);
    }
}
__global__ __launch_bounds__(64) void k_hc12_stitch(CodecArgs a)
{
    __shared__ Hc12Ent oEnt[kH12SegLds];
    __shared__ uint64_t seqs[64];
    const Hc12Ws w = h12_seg_ws(a, oEnt, seqs);
    const bool broken = plz4_readfirstlane(*(volatile int32_t*)a.h12Err) != 0;
    for (int g = next_block(a.queue); g < a.nBlocks; g = next_block(a.queue)) {
        const int i = a.blk0 + g;
        const int n = block_len(a, i);
        LzPiece* const pieces = a.lzPieces + (int64_t)g * 2 * a.lzSegs;
        int lastAnchor = 0, nseq = -1, segs = 0;
        if (broken) nseq = kSeqEngineFailed;                                 // the search kernel gave up (spin guard): its F is not to be trusted
        else if (n >= 0 && n <= a.l1MaxLen) {
            segs = lz_segments(n, a.lzSegs, a.lzMinSeg);
            nseq = hc12_stitch(a.src + (int64_t)i * a.srcStride, n, a.h12F + (int64_t)g * a.h12FStride, a.h12Chain + (int64_t)g * a.h12ChainStride, w, segs,
                               a.lzRec + (int64_t)g * a.lzRecStride, a.lzBridge + (int64_t)g * a.lzRecStride,
                               a.lzMeta + (int64_t)g * a.lzSegs, a.lzStarts + (int64_t)g * a.lzSegs * kLzStarts, pieces, &lastAnchor);
        }
        if ((threadIdx.x & 63u) == 0) {
            for (int k = 2 * segs; k < 2 * a.lzSegs; ++k) pieces[k].cnt = 0;
            SeqInfo inf; inf.nseq = nseq; inf.lastAnchor = lastAnchor; inf.total = 0; inf.stored = 0; a.l1Info[g] = inf;
        }
    }
}

// Level 2 on independent blocks: the batch walk over the two tables (hc_mid_parse, lz4hc_lazy_device.inl), one wave per block,
// the tables in the wave's slot of the HC workspace; records out, the emit kernels of level 1 behind it.
// kD: blocks behind external segments (a.hcPfx; dictionary / linked blocks): the tables start from LZ4MID_fillHTable over the segment
template <bool kD> __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_hc_mid(CodecArgs a)
{
    uint32_t* const tabs = (uint32_t*)(a.hcWork + (size_t)blockIdx.x * kHcWorkBytes);
    for (int i = next_block(a.queue); i < a.nBlocks; i = next_block(a.queue)) {
        const int gi = a.blk0 + i;
        const int n  = block_len(a, gi);
        const int pfx = kD ? hc_pfx_of(a, gi) : 0;
        int lastAnchor = 0, nseq = -1;                                       // -1: a block the workspace was not sized for, or one that is not this path's
        if (n >= 0 && n <= a.l1MaxLen && pfx >= 0)
            nseq = hc_mid_parse<kD>(a.src + (int64_t)gi * a.srcStride, n, tabs, tabs + 16384, a.l1Seq + (int64_t)i * a.l1SeqStride, &lastAnchor, pfx);
        if ((threadIdx.x & 63u) == 0) { SeqInfo inf; inf.nseq = nseq; inf.lastAnchor = lastAnchor; inf.total = 0; inf.stored = 0; a.l1Info[i] = inf; }
    }
}

// clz4.NewDictCtxHC (clz4.go:122-147): workgroup 0 builds the level-2 (lz4mid) tables of a dictionary, workgroup 1 the
// hash-chain tables every other level shares.  tabs = 2 x kHcWorkBytes.
__global__ __launch_bounds__(64) void k_hc_dict_prime(const uint8_t* dict, int len, uint8_t* tabs)
{
    uint8_t* ws = tabs + (size_t)blockIdx.x * kHcWorkBytes;
    HcWork w; w.hash = (uint32_t*)ws; w.chain = (uint16_t*)(ws + kHcHashEntries * 4);
    w.opt = (HcOpt*)(ws + kHcHashEntries * 4 + kHcChainEntries * 2); w.pre = nullptr; w.rank = nullptr; w.list = nullptr;
    hc_prime_dict(dict, len, blockIdx.x == 0 ? 2 : 3, w);
}

// ---- LZ4_decompress_safe of a few blocks by the whole chip (lz4_dx_device.inl).  grid (segments, blocks) for the per-segment
// kernels, (chunks of 1024 output bytes, blocks) for the per-byte ones; a block that any stage flags is decoded by k_decode_raw behind.
__device__ __forceinline__ const uint8_t* dx_src(const CodecArgs& a, int b) { return a.src + (a.dxSrcOff ? a.dxSrcOff[b] : (int64_t)b * a.srcStride); }
__device__ __forceinline__ int dx_len(const CodecArgs& a, int b) { return a.dxLen ? a.dxLen[b] : a.srcLen[b]; }
// One block's view of the call for the stage bodies (dx_stage_*, lz4_dx_device.inl)
__device__ __forceinline__ DxBlk dx_blk(const CodecArgs& a, int b)
{
    DxBlk k;
    k.src = dx_src(a, b); k.n = dx_len(a, b); k.dst = a.dst + (int64_t)b * a.dstStride; k.cap = cap_of(a, b);
    k.T = a.dxT + (int64_t)b * a.dxTStride; k.ptr = a.dxPtr + (int64_t)b * a.dxPtrStride; k.units = a.dxUnits + (int64_t)b * a.dxMaxSeg;
    k.tStride = a.dxTStride; k.pStride = a.dxPtrStride; k.maxSeg = a.dxMaxSeg;
    k.info = a.dxInfo + b; k.b = b;
    return k;
}
__device__ __forceinline__ DxlCall dxl_call(const CodecArgs& a)
{
    DxlCall c;
    c.ptr = a.dxPtr; c.P = a.dxPtrStride; c.nb = a.nBlocks; c.info = a.dxInfo; c.len = a.dxLen; c.first = a.dxlFirst; c.chain = a.dxlChain;
    if (a.linked) { c.hist = a.window; c.histStride = 131072; c.histLen = a.windowLen; c.histLenAll = 0; }
    else { c.hist = a.dict; c.histStride = 0; c.histLen = nullptr; c.histLenAll = (a.dict && a.dictLen > 0) ? a.dictLen : 0; }
    c.dst = a.dst; c.dstStride = a.dstStride;
    return c;
}

// A flavour at kernel level: the device flavour F for block b of the call, and the block's verdict behind the gather (one thread;
// cnt: plz4hip_ctx_counters).
struct KDx {                   // blocks up to kDxMaxOut
    typedef DxF F;
    static DEVM F flavour(const CodecArgs&, int) { return F{}; }
    static DEVM void verdict(const CodecArgs& a, int b, int outLen, unsigned long long* cnt)
    {
        atomicAdd(&cnt[3], 1ull);                                           // (blocks this path answered)
        // (records: the payload's checksum is verified beside this path, k_dx_rec_hash; frame.go:114-127 rejects before it decodes)
        const bool hashBad = a.dxHashBad && a.dxHashBad[b];
        a.result[b] = hashBad ? 0 : outLen;
        if (a.status) a.status[b] = hashBad ? PLZ4HIP_BLK_HASH_MISMATCH : PLZ4HIP_BLK_OK;
    }
};
struct KDxb {                  // raw blocks above kDxMaxOut (dxb_*): the stitch in three steps, long runs written down by the fill
    typedef DxbF F;            // and run over the whole grid (k_dxb_runs), the jump rounds the call's largest capacity asks for
    static DEVM F flavour(const CodecArgs& a, int b)
    {
        return F{a.dxbTG + (int64_t)b * a.dxbTGStride, a.dxbEnt + (int64_t)b * a.dxbGroups, a.dxbG,
                 a.dxbRuns + (int64_t)b * a.dxbRunRoom, a.dxbRunRoom, a.dxbThr, a.dxbInfo + b};
    }
    static DEVM void verdict(const CodecArgs& a, int b, int outLen, unsigned long long* cnt)
    {
        atomicAdd(&cnt[3], 1ull);
        if (cap_of(a, b) > kDxMaxOut) { atomicAdd(&cnt[10], 1ull); atomicAdd(&cnt[12], (unsigned long long)min_(a.dxbInfo[b].runs, (uint32_t)a.dxbRunRoom)); }
        a.result[b] = outLen;
        if (a.status) a.status[b] = PLZ4HIP_BLK_OK;
    }
};
struct KDxl {                  // history outside the block (dxl_*): k_dxl_link in front of the fill, k_dxl_resolve behind it; the verdicts
    typedef DxlF F;            // are k_dxl_finish's (linked) or k_dxl_verdict's (under a dictionary), behind the gather
    static DEVM F flavour(const CodecArgs& a, int) { return F{dxl_call(a), a.dxlMoved}; }
    static DEVM void verdict(const CodecArgs&, int, int, unsigned long long*) {}
};

__global__ __launch_bounds__(64) void k_dx_tables(CodecArgs a)
{
    dx_stage_tables(dx_blk(a, blockIdx.y), blockIdx.x, gridDim.x);
}
__global__ __launch_bounds__(64) void k_dx_stitch(CodecArgs a)
{
    dx_stage_stitch(dx_blk(a, blockIdx.x));
}
template <class K> __global__ __launch_bounds__(64) void k_dx_fill(CodecArgs a)
{
    const int j = blockIdx.x, b = blockIdx.y;
    dx_stage_fill(K::flavour(a, b), dx_blk(a, b), j);
}
template <class K> __global__ __launch_bounds__(256) void k_dx_jump(CodecArgs a)
{
    const int b = blockIdx.y, p0 = (blockIdx.x * 4 + (int)(threadIdx.x >> 6)) * 256;
    dx_stage_jump(K::flavour(a, b), dx_blk(a, b), a.dxRound, p0);
}
template <class K> __global__ __launch_bounds__(256) void k_dx_gather(CodecArgs a, unsigned long long* cnt)
{
    const int b = blockIdx.y, p0 = (blockIdx.x * 4 + (int)(threadIdx.x >> 6)) * 256;
    const DxBlk k = dx_blk(a, b);
    if (blockIdx.x == 0 && threadIdx.x == 0 && !k.info->bad) K::verdict(a, b, k.info->outLen, cnt);
    dx_stage_gather(K::flavour(a, b), k, p0);
}

// ---- ... of raw blocks above kDxMaxOut (KDxb): the three steps of its stitch, and the listed runs behind its fill
__global__ __launch_bounds__(256) void k_dxb_compose(CodecArgs a)
{
    const int b = blockIdx.y, w = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);     // 128 waves to a group
    dxb_stage_compose(KDxb::flavour(a, b), dx_blk(a, b), w >> 7, w & 127);
}
__global__ __launch_bounds__(64) void k_dxb_hop(CodecArgs a, unsigned long long* cnt)
{
    const int b = blockIdx.x;
    dxb_stage_hop(KDxb::flavour(a, b), dx_blk(a, b));
    if (b == 0 && (threadIdx.x & 63u) == 0) { cnt[11] = (unsigned long long)a.dxbRounds; cnt[12] = 0ull; }   // (plz4hip_ctx_counters: the last call of this kind)
}
__global__ __launch_bounds__(64) void k_dxb_units(CodecArgs a)
{
    const int g = blockIdx.x, b = blockIdx.y;
    dxb_stage_units(KDxb::flavour(a, b), dx_blk(a, b), g);
}
__global__ __launch_bounds__(256) void k_dxb_runs(CodecArgs a)
{
    const int b = blockIdx.y;
    if (a.dxInfo[b].bad) return;
    const uint32_t nr = min_(a.dxbInfo[b].runs, (uint32_t)a.dxbRunRoom);
    const uint32_t W = gridDim.x * 4u, w = blockIdx.x * 4u + (threadIdx.x >> 6);
    const DxRun* const list = a.dxbRuns + (int64_t)b * a.dxbRunRoom;
    uint32_t first = w;                                              // the wave that takes a run's first piece moves on from run to run
    for (uint32_t i = 0; i < nr; ++i) {
        DxRun r;
        r.op = plz4_readfirstlane(list[i].op); r.from = plz4_readfirstlane(list[i].from);
        r.len = plz4_readfirstlane(list[i].len); r.kind = plz4_readfirstlane(list[i].kind);
        const uint32_t pieces = dxb_run_pieces(r);
        for (uint32_t c = first; c < pieces; c += W) dxb_run_piece(r, c, dx_src(a, b), a.dst + (int64_t)b * a.dstStride, a.dxPtr + (int64_t)b * a.dxPtrStride);
        first = (first + W - pieces % W) % W;
    }
}

// records on the few-block path: which records are compressed payloads of a sane size (FrameReader._read's checks, blk/frame.go:
// 79-85; everything else -- stored blocks, size overflows -- is the one-wave kernel's, which runs for the flagged blocks behind)
__global__ __launch_bounds__(256) void k_dx_rec_prep(CodecArgs a, int64_t* srcOff, int32_t* len)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.nBlocks) return;
    const int64_t off = a.recOff ? a.recOff[i] : (int64_t)i * a.srcStride;
    const int64_t recLen = a.recOff ? a.recOff[i + 1] - a.recOff[i] : (int64_t)a.srcLen[i];
    // (k_dx_rec_hash reads payload and checksum where this is >= 0; k_dxl_link leaves a chain's blocks behind a kDxRecBad one alone)
    srcOff[i] = off + 4; len[i] = dx_rec_len(a.src + off, recLen, a.bsz, a.blockChecksum != 0, a.dstCapAll);
}
// ... and their block checksums (frame.go:114-127), one wave per record, on a stream of its own beside the decode
__global__ __launch_bounds__(64) void k_dx_rec_hash(CodecArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t stagebuf[4096];
    const int b = blockIdx.x;
    const int n = a.dxLen[b];
    int bad = 0;
    if (n >= 0) {
        const uint8_t* p = a.src + a.dxSrcOff[b];
        bad = wave_xxh32_staged(p, n, stagebuf) != plz4_readfirstlane(ld32u(p + n));
    }
    if ((threadIdx.x & 63u) == 0) a.dxHashBad[b] = bad;
}

// ---- ... of blocks with history outside the block (KDxl): k_dx_rec_prep / k_dx_rec_hash / k_dx_tables / k_dx_stitch as above,
// then k_dxl_link, the fill, k_dxl_resolve, the jump rounds, the gather and, per chain, k_dxl_finish (linked) or, per block,
// k_dxl_verdict (independent blocks under a dictionary; the flagged ones run k_decode_*_dict behind).
__device__ __forceinline__ DxlFin dxl_fin(const CodecArgs& a)
{
    DxlFin f; f.hashBad = a.dxHashBad; f.moved = a.dxlMoved; f.rounds = a.dxlRounds; f.result = a.result; f.status = a.status;
    return f;
}
__device__ __forceinline__ bool dxl_good(const CodecArgs& a, int b)
{
    return dx_len(a, b) >= 0 && !a.dxInfo[b].bad && !(a.dxHashBad && a.dxHashBad[b])
        && dxl_converged(a.dxlMoved + (int64_t)b * (kDxlMaxRounds + 1), a.dxlRounds);
}
__global__ __launch_bounds__(256) void k_dxl_link(CodecArgs a, unsigned long long* cnt)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    // (plz4hip_ctx_counters: jump rounds of the last such call -- the maximum over its groups -- and how many groups it had)
    if (i == 0 && a.dxlGroup == 0) { cnt[5] = 0; if (a.dxlGroups) cnt[6] = (unsigned long long)a.dxlGroups; }
    if (i >= a.nBlocks) return;
    int first = i, ch = 0;
    if (a.linked) {
        first = 0;
        if (a.chainFirst) { while (ch + 1 < a.nChains && chain_lo(a, ch + 1) <= i) ++ch; first = chain_lo(a, ch); }
    }
    a.dxlFirst[i] = first; a.dxlChain[i] = ch; a.dxlGood[i] = 0;
    // (a chain that is known to have ended in front of this block: the stages stay off it, its output stays as it was)
    if (a.linked && dxl_chain_dead(a.dxLen, first, i, a.dxlDead ? a.dxlDead[ch] : 0)) a.dxInfo[i].bad = 1;
    for (int r = 0; r <= kDxlMaxRounds; ++r) a.dxlMoved[(int64_t)i * (kDxlMaxRounds + 1) + r] = 0;
}
__global__ __launch_bounds__(256) void k_dxl_resolve(CodecArgs a)
{
    const int b = blockIdx.y, p0 = (blockIdx.x * 4 + (int)(threadIdx.x >> 6)) * 256;
    if (p0 >= a.dxPtrStride) return;
    if (!dxl_resolve(dxl_call(a), b, p0, (int)a.dxPtrStride) && (threadIdx.x & 63u) == 0) atomicOr(&a.dxInfo[b].bad, 1);
}
// independent blocks under a dictionary: which blocks the path answers
__global__ __launch_bounds__(256) void k_dxl_verdict(CodecArgs a, unsigned long long* cnt)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.nBlocks || !dxl_good(a, i)) return;
    a.dxlGood[i] = 1;
    a.result[i] = a.dxInfo[i].outLen;
    if (a.status) a.status[i] = PLZ4HIP_BLK_OK;
    atomicAdd(&cnt[4], 1ull);                                               // (plz4hip_ctx_counters: blocks this path answered)
    atomicMax(&cnt[5], (unsigned long long)dxl_rounds_of(a.dxlMoved + (int64_t)i * (kDxlMaxRounds + 1), a.dxlRounds));
}
// linked blocks, one wave per chain: the chain's good blocks are answered (a stored block among them is copied out here and does
// not enter the window), the window they leave is laid down, and from the first block that is not plainly good the one-wave walk
// goes on (linked_walk: its own verdict for that block, CORRUPT for what follows, the window as it was in front of it).
__global__ __launch_bounds__(64) void k_dxl_finish(CodecArgs a, unsigned long long* cnt)
{
    __shared__ __attribute__((aligned(16))) uint8_t dl[kDecLdsBytes];
    const int ch = blockIdx.x;
    const int first = chain_lo(a, ch), last = a.chainFirst ? chain_lo(a, ch + 1) : a.nBlocks;
    if (a.dxlDead && first >= last) return;                                 // (a group of a cut call: the chain has no block in it)
    RecWave rec{a, dl};
    int winLen = plz4_readfirstlane(a.windowLen[ch]);
    int dead = a.dxlDead ? plz4_readfirstlane(a.dxlDead[ch]) : 0;
    int taken = 0, rounds = 0;
    dxl_finish(dxl_call(a), dxl_fin(a), rec, first, last, a.window + (size_t)ch * 131072, &winLen, &dead, &taken, &rounds);
    if ((threadIdx.x & 63u) == 0) {
        a.windowLen[ch] = winLen;
        if (a.dxlDead) a.dxlDead[ch] = dead;
        if (taken) { atomicAdd(&cnt[4], (unsigned long long)taken); atomicMax(&cnt[5], (unsigned long long)rounds); }
    }
}

__global__ __launch_bounds__(64) void k_decode_raw(CodecArgs a)
{
    for (int i = next_block(a.queue); i < a.nBlocks; i = next_block(a.queue)) {
        if (a.dxInfo && !a.dxInfo[i].bad) continue;                          // (answered by the few-block path)
        const int n   = a.srcLen[i];
        const int cap = cap_of(a, i);
        const int r   = wave_decode_block(a.src + (int64_t)i * a.srcStride, n, a.dst + (int64_t)i * a.dstStride, cap);
        if ((threadIdx.x & 63u) == 0) a.result[i] = r;
    }
}

// FrameReader._read's per-block checks + BlkT.Decompress on the device (blk/frame.go:54-127, blk.go:50-61).
// Record i starts at src + recOff[i] when recOff is given, else at src + i*srcStride with srcLen[i] bytes.
// kDx: behind the few-block path (launch_decode): only the records that path has flagged.  A template parameter so that the
// kernels of the bulk path -- k_decode_rec, k_l1_duplex: bound by their scalar registers -- do not carry the test.
template <bool kDx = false>
__device__ __forceinline__ void decode_rec_loop(const CodecArgs& a, uint8_t* dl)
{
    for (int i = next_block(a.queue); i < a.nBlocks; i = next_block(a.queue)) {
        if (kDx && !a.dxInfo[i].bad) continue;                               // (answered by the few-block path)
        const uint8_t* rec    = a.recOff ? a.src + a.recOff[i] : a.src + (int64_t)i * a.srcStride;
        const int64_t  recLen = a.recOff ? a.recOff[i + 1] - a.recOff[i] : (int64_t)a.srcLen[i];
        uint8_t*       out    = a.dst + (int64_t)i * a.dstStride;
        uint32_t       word;
        const int      sz     = rec_head<true>(rec, recLen, a.bsz, a.blockChecksum != 0, &word);
        int st = PLZ4HIP_BLK_OK, r = 0;
        if (sz < 0) {
            st = PLZ4HIP_BLK_SIZE_OVERFLOW;
        } else {
            // the bulk path: k_rec_verify16 has run in front of this launch and left its verdict; what it rejected is not decoded
            if (!kDx && a.blockChecksum) st = plz4_readfirstlane(a.status[i]);
            if (kDx && a.blockChecksum) {
                const uint32_t want = plz4_readfirstlane(ld32u(rec + 4 + sz));
                if (wave_xxh32(rec + 4, sz) != want) st = PLZ4HIP_BLK_HASH_MISMATCH;
            }
            if (st == PLZ4HIP_BLK_OK) {
                if (word & 0x80000000u) {                                    // stored block: straight copy
                    const int cap = a.dstCapAll;
                    if (sz > cap) { st = PLZ4HIP_BLK_SIZE_OVERFLOW; }
                    else { wave_copy(out, rec + 4, sz); r = sz; }
                } else {
                    r = wave_decode_block<true>(rec + 4, sz, out, a.dstCapAll, nullptr, 0, dl);
                    if (r < 0) st = PLZ4HIP_BLK_CORRUPT;
                }
            }
        }
        if ((threadIdx.x & 63u) == 0) { a.result[i] = r; a.status[i] = st; }
    }
}
// The block checksums of the bulk decoder's records, ahead of the decode (frame.go:114-127 rejects before it decodes): one wave per
// 16 records, four lanes each (wave_xxh32_x16), no LDS -- enqueued in front of every launch of decode_rec_loop<false> with block
// checksums.  FrameReader._read's size checks and the comparison; status[i] <- OK / HASH_MISMATCH / SIZE_OVERFLOW, result[i] <- 0
// where it is not OK.  The decoder then skips what is not OK and carries no checksum pass of its own.
__global__ __launch_bounds__(64) void k_rec_verify16(CodecArgs a)
{
    const int i = blockIdx.x * 16 + (int)((threadIdx.x & 63u) >> 2);
    const uint8_t* p[1] = {nullptr};
    int n[1] = {-1};
    uint32_t x[1];
    uint32_t want = 0;
    if (i < a.nBlocks) {
        const uint8_t* rec    = a.recOff ? a.src + a.recOff[i] : a.src + (int64_t)i * a.srcStride;
        const int64_t  recLen = a.recOff ? a.recOff[i + 1] - a.recOff[i] : (int64_t)a.srcLen[i];
        uint32_t word;
        const int sz = rec_head<false>(rec, recLen, a.bsz, true, &word);
        if (sz >= 0) { p[0] = rec + 4; n[0] = sz; want = ld32u(rec + 4 + sz); }
    }
    wave_xxh32_x16(p, n, x);
    if ((threadIdx.x & 3u) == 0 && i < a.nBlocks) {
        const int st = n[0] < 0 ? PLZ4HIP_BLK_SIZE_OVERFLOW : x[0] != want ? PLZ4HIP_BLK_HASH_MISMATCH : PLZ4HIP_BLK_OK;
        a.status[i] = st;
        if (st != PLZ4HIP_BLK_OK) a.result[i] = 0;
    }
}
#if defined(PLZ4_EXP_DEC_EU)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 6))) void k_decode_rec(CodecArgs a)
#else
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6, 6))) void k_decode_rec(CodecArgs a)
#endif
{
    __shared__ __attribute__((aligned(16))) uint8_t dl[kDecLdsBytes];       // the vector path assembles each batch's output here
    decode_rec_loop<false>(a, dl);
}
__global__ __launch_bounds__(64) void k_decode_rec_dx(CodecArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t dl[kDecLdsBytes];
    decode_rec_loop<true>(a, dl);
}

// The level-1 parse of one call and the record decode of another in ONE launch (plz4hip_dev_duplex_records).  The parser is a
// serial chain per block that leaves half of a SIMD's VALU issue slots idle at the 2.5 waves per SIMD its LDS tables allow
// (profiles/r03_summary.json: 51 %), and the decoder is bound by exactly those slots (85-92 %) and needs 1.1 KiB of LDS per
// wave.  Two kernels on two streams do not share a CU that way: the parser's workgroup takes all of a CU's LDS.  So a
// workgroup here is P parser waves (a 16 KiB table each) + D decoder waves -- by default 1 + 1, nine workgroups per CU: 9
// parsers and 9 decoders -- and the parser waves run at a raised priority: the decoders issue when a parser waits.
// Each role pulls block ids from its own queue until it is empty; the waves of a workgroup never synchronise.
// (P parser waves + D decoder waves per workgroup: experiment switch PLZ4HIP_DUPLEX="P,D"; PRIO: the parser waves' s_setprio,
// PLZ4HIP_DUPLEX_PRIO)
constexpr int kWinScratch = 256;          // per parser wave: the dwords its lanes park for the windows of the batch after next
constexpr int duplex_wgs_per_cu(int P, int D) { return (160 * 1024) / (P * (kHashBytes + kWinScratch) + D * kDecLdsBytes); }
#if defined(PLZ4_EXP_DUPLEX_EU)
constexpr int duplex_waves_per_eu(int P, int D) { return PLZ4_EXP_DUPLEX_EU; }       // EXPERIMENT: forced occupancy target
#else
constexpr int duplex_waves_per_eu(int P, int D) { return ((P + D) * duplex_wgs_per_cu(P, D) + 3) / 4; }
#endif
template <int P, int D, int PRIO> __global__ __launch_bounds__(64 * (P + D))
__attribute__((amdgpu_waves_per_eu(duplex_waves_per_eu(P, D), duplex_waves_per_eu(P, D))))
void k_l1_duplex(CodecArgs a, CodecArgs d)
{
    __shared__ uint32_t tabS[P][kHashBytes / 4];
    __shared__ __attribute__((aligned(16))) uint8_t dlS[D][kDecLdsBytes];
    __shared__ __attribute__((aligned(16))) uint8_t winS[P][kWinScratch];
    const int w = plz4_readfirstlane((int)(threadIdx.x >> 6));
    if (w < P) {
        if (PRIO) __builtin_amdgcn_s_setprio(PRIO);
        l1_parse_loop<1>(a, tabS[w], winS[w]);
    } else {
        decode_rec_loop<false>(d, dlS[w - P]);
    }
}

__global__ __launch_bounds__(64) void k_xxh32(const uint8_t* base, int64_t stride, const int32_t* len, uint32_t* out,
                                              int n, uint32_t* queue)
{
    for (int i = next_block(queue); i < n; i = next_block(queue)) {
        const uint32_t x = wave_xxh32(base + (int64_t)i * stride, len[i]);
        if ((threadIdx.x & 63u) == 0) out[i] = x;
    }
}

// Streaming content checksum (xxh32.XXHZero): one wave writes the buffers base + i*stride (lens[i] bytes each, or `single`
// bytes at base when lens is null) into the stream state, in order.  lens may be a result array: entries <= 0 are skipped.
__global__ __launch_bounds__(64) void k_xxh32_stream(XxhStream* st, const uint8_t* base, int64_t stride, const int32_t* lens, int n, int64_t single, int reset)
{
    if (reset) wave_xxh32_stream_reset(st);
    if (!lens) { wave_xxh32_stream_update(st, base, single); return; }
    for (int i = 0; i < n; ++i) {
        const int len = plz4_readfirstlane(lens[i]);
        if (len > 0) wave_xxh32_stream_update(st, base + (int64_t)i * stride, len);
    }
}

// The index of a frame body that lies in device memory (plz4hip_dev_index_body): FrameReader._read's size-word walk, one wave,
// no LDS, no workspace (wave_index_body, lz4_body_index_device.inl).
static_assert(kBodyEndMark == PLZ4HIP_BODY_END_MARK && kBodyEndOfBytes == PLZ4HIP_BODY_END_OF_BYTES && kBodyFull == PLZ4HIP_BODY_FULL &&
              kBodySizeOverflow == PLZ4HIP_BODY_SIZE_OVERFLOW && kBodyTruncatedWord == PLZ4HIP_BODY_TRUNCATED_WORD &&
              kBodyTruncatedBlock == PLZ4HIP_BODY_TRUNCATED_BLOCK, "lz4_body_index_device.inl and plz4hip.h name the same status");
static_assert(sizeof(BodyIndex) == sizeof(plz4hip_body_index) && sizeof(BodyIndex) == 16, "plz4hip_body_index is {int64, int32, int32}");
__global__ __launch_bounds__(64) void k_index_body(const uint8_t* body, int64_t bodyBytes, int bsz, int blockChecksum, int maxBlocks,
                                                   int64_t* recOff, BodyIndex* info)
{
    wave_index_body(body, bodyBytes, bsz, blockChecksum != 0, maxBlocks, recOff, info);
}

// The index of a whole stream that lies in device memory (plz4hip_dev_index_stream): the reader's header-mode / body-mode walk, one
// wave, no LDS, no workspace (wave_index_stream, lz4_stream_index_device.inl).
static_assert(kStreamEnd == PLZ4HIP_STREAM_END && kStreamFramesFull == PLZ4HIP_STREAM_FRAMES_FULL && kStreamRecordsFull == PLZ4HIP_STREAM_RECORDS_FULL &&
              kStreamHeaderRead == PLZ4HIP_STREAM_HEADER_READ && kStreamMagic == PLZ4HIP_STREAM_MAGIC && kStreamVersion == PLZ4HIP_STREAM_VERSION &&
              kStreamReservedBit == PLZ4HIP_STREAM_RESERVED_BIT && kStreamBlockDescriptor == PLZ4HIP_STREAM_BLOCK_DESCRIPTOR &&
              kStreamHeaderHash == PLZ4HIP_STREAM_HEADER_HASH && kStreamSkip == PLZ4HIP_STREAM_SKIP && kStreamBody == PLZ4HIP_STREAM_BODY &&
              kStreamContentHashRead == PLZ4HIP_STREAM_CONTENT_HASH_READ, "lz4_stream_index_device.inl and plz4hip.h name the same status");
static_assert(sizeof(FrameIndex) == sizeof(plz4hip_frame_index) && sizeof(FrameIndex) == 64 && offsetof(FrameIndex, status) == 56 &&
              offsetof(plz4hip_frame_index, status) == 56 && offsetof(plz4hip_frame_index, flags) == 52 && offsetof(plz4hip_frame_index, dictId) == 32,
              "plz4hip_frame_index is 64 bytes, as wave_store_frame lays it out");
static_assert(sizeof(StreamIndex) == sizeof(plz4hip_stream_index) && sizeof(StreamIndex) == 32 && offsetof(plz4hip_stream_index, flagsAnd) == 28 &&
              offsetof(StreamIndex, flagsAnd) == 28, "plz4hip_stream_index is 32 bytes");
__global__ __launch_bounds__(64) void k_index_stream(const uint8_t* bytes, int64_t nBytes, int maxFrames, int maxRecs, FrameIndex* frames,
                                                     int64_t* recOff, StreamIndex* info)
{
    wave_index_stream(bytes, nBytes, maxFrames, maxRecs, frames, recOff, info);
}

// The verdict on every frame of a decoded stream (plz4hip_dev_verify_frames): sixteen frames' xxh32 chains per wave over the pieces
// a record decode left, one-wave workgroups that stride over the table, no LDS, no workspace (wave_verify_frames,
// lz4_frame_verify_device.inl); behind it one wave that folds the verdicts into the stream's (wave_verify_summary).
static_assert(kFrameOk == PLZ4HIP_FRAME_OK && kFrameSkippable == PLZ4HIP_FRAME_SKIPPABLE && kFrameRange == PLZ4HIP_FRAME_RANGE &&
              kFrameBlock == PLZ4HIP_FRAME_BLOCK && kFrameIncomplete == PLZ4HIP_FRAME_INCOMPLETE && kFrameContentHash == PLZ4HIP_FRAME_CONTENT_HASH &&
              kFrameContentSize == PLZ4HIP_FRAME_CONTENT_SIZE && PLZ4HIP_BLK_OK == 0, "lz4_frame_verify_device.inl and plz4hip.h name the same status");
static_assert(sizeof(FrameVerdict) == sizeof(plz4hip_frame_verdict) && sizeof(FrameVerdict) == 32 && offsetof(plz4hip_frame_verdict, status) == 12 &&
              offsetof(FrameVerdict, status) == 12 && offsetof(plz4hip_frame_verdict, blockStatus) == 20, "plz4hip_frame_verdict is 32 bytes");
static_assert(sizeof(StreamVerdict) == sizeof(plz4hip_stream_verdict) && sizeof(StreamVerdict) == 32 && offsetof(plz4hip_stream_verdict, nFrames) == 16 &&
              offsetof(StreamVerdict, nFrames) == 16, "plz4hip_stream_verdict is 32 bytes");
__global__ __launch_bounds__(64) void k_verify_frames(const FrameIndex* frames, const StreamIndex* info, int maxFrames, const uint8_t* dst,
                                                      int64_t dstStride, int dstCap, const int32_t* result, const int32_t* status, int maxRecs,
                                                      FrameVerdict* verdicts)
{
    wave_verify_frames(frames, info, maxFrames, dst, dstStride, dstCap, result, status, maxRecs, verdicts, (int)blockIdx.x, (int)gridDim.x);
}
__global__ __launch_bounds__(64) void k_verify_summary(const StreamIndex* info, int maxFrames, const FrameVerdict* verdicts, StreamVerdict* sv)
{
    wave_verify_summary(info, maxFrames, verdicts, sv);
}

// Whole frames around an encoded block section (plz4hip_dev_write_frames): sixteen frames' headers, trailers and content checksums per
// wave over the plaintext the encoder read (wave_frame_edges, lz4_frame_write_device.inl), the records into their places
// (wave_frame_move: grid (nBlocks, slices), four waves a workgroup), and one wave that writes info (wave_frame_summary).
static_assert(kWriteOk == PLZ4HIP_WRITE_OK && kWriteNoRoom == PLZ4HIP_WRITE_NO_ROOM && kWriteRecord == PLZ4HIP_WRITE_RECORD,
              "lz4_frame_write_device.inl and plz4hip.h name the same status");
static_assert(sizeof(WriteInfo) == sizeof(plz4hip_write_info) && sizeof(WriteInfo) == 32 && offsetof(plz4hip_write_info, status) == 16 &&
              offsetof(WriteInfo, status) == 16 && offsetof(plz4hip_write_info, firstBadRec) == 20 && offsetof(WriteInfo, firstBadRec) == 20,
              "plz4hip_write_info is 32 bytes");
static_assert(offsetof(plz4hip_write_info, end) == offsetof(plz4hip_stream_index, end) && offsetof(plz4hip_write_info, nFrames) == offsetof(plz4hip_stream_index, nFrames) &&
              offsetof(plz4hip_write_info, nRecs) == offsetof(plz4hip_stream_index, nRecs), "plz4hip_write_info starts as plz4hip_stream_index does");
static_assert(sizeof(plz4hip_frame_opts) == 32 && offsetof(plz4hip_frame_opts, dictId) == 24, "plz4hip_frame_opts is eight 32-bit words");
__global__ __launch_bounds__(64) void k_frame_edges(FrameWriteGeom g, const uint8_t* src, const uint8_t* body, const int64_t* recOff, uint8_t* out,
                                                    FrameIndex* frames, int64_t* outRecOff)
{
    wave_frame_edges(g, src, body, recOff, out, frames, outRecOff, (int)blockIdx.x, (int)gridDim.x);
}
__global__ __launch_bounds__(256) void k_frame_move(FrameWriteGeom g, const uint8_t* body, const int64_t* recOff, uint8_t* out)
{
    wave_frame_move(g, body, recOff, out, (int)blockIdx.x, (int)(blockIdx.y * 4 + (threadIdx.x >> 6)), (int)(gridDim.y * 4));
}
__global__ __launch_bounds__(64) void k_frame_summary(FrameWriteGeom g, const int64_t* recOff, const FrameIndex* frames, WriteInfo* info)
{
    wave_frame_summary(g, recOff, frames, info);
}

// Exclusive prefix sum int32 -> int64, one wave, no LDS (wave_scan_lengths).
__global__ __launch_bounds__(64) void k_scan(const int32_t* __restrict__ len, int64_t* __restrict__ off, int n)
{
    wave_scan_lengths<false>(len, off, n, 1);
}

// ... continued behind an earlier part: off[0] holds where this part starts (the total the scan of the part before left there);
// lengths that are not positive (an engine failure code) count as 0
__global__ __launch_bounds__(64) void k_scan_from(const int32_t* __restrict__ len, int64_t* __restrict__ off, int n, int first)
{
    wave_scan_lengths<true>(len, off, n, first);
}

// Bytes to hand back per block of a host call: the result if positive (sizes), nothing for 0 / error codes.
// plz4hip_dev_compress: the lengths live on the device and the workspaces are sized from the caller's maxLen.  A private copy with
// every length outside [0, maxLen] replaced by 0 is what the kernels see; such a block's result becomes PLZ4HIP_E_ARG afterwards.
__global__ __launch_bounds__(256) void k_check_len(const int32_t* __restrict__ srcLen, int maxLen, int n, int32_t* __restrict__ lenOut, int32_t* __restrict__ result, int after)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const bool bad = srcLen[i] < 0 || srcLen[i] > maxLen;
    if (!after) lenOut[i] = bad ? 0 : srcLen[i];
    else if (bad) result[i] = PLZ4HIP_E_ARG;
}

__global__ __launch_bounds__(256) void k_out_len(const int32_t* __restrict__ res, int32_t* __restrict__ len, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) len[i] = res[i] > 0 ? res[i] : 0;
}

// Record mover: dst + dstOff[i] <- src + (srcOff ? srcOff[i] : i*stride), len[i] bytes.  Compaction of the staging
// area into the frame body is the srcOff == nullptr case.  grid = (n, slices); 256 threads move 16 bytes each per
// step (unaligned on both sides is fine on gfx950: global_load/store_dwordx4).
__global__ __launch_bounds__(256) void k_move_records(const uint8_t* __restrict__ src, const int64_t* __restrict__ srcOff,
                                                      int64_t stride, const int32_t* __restrict__ len,
                                                      const int64_t* __restrict__ dstOff, uint8_t* __restrict__ dst,
                                                      int64_t dstCap)
{
    const int      i = blockIdx.x;
    const int      n = len[i];
    if (n <= 0 || dstOff[i] < 0 || dstOff[i] + n > dstCap) return;      // (an overflow shows to the caller as recOff[n] > bodyCap)
    const uint8_t* s = src + (srcOff ? srcOff[i] : (int64_t)i * stride);
    uint8_t*       d = dst + dstOff[i];
    const int full = n & ~15;
    for (int p = (blockIdx.y * 256 + threadIdx.x) * 16; p < full; p += gridDim.y * 256 * 16)
        *(v16u_t*)(d + p) = *(const v16u_t*)(s + p);
    if (blockIdx.y == 0 && (int)threadIdx.x < (n - full)) d[full + threadIdx.x] = s[full + threadIdx.x];
}

}  // namespace

// ------------------------------------------------------------------------------------------------ context
struct plz4hip_xxh32_stream;
struct plz4hip_ctx {
    int          device = 0;
    hipStream_t  stream = nullptr;
    std::mutex   mu;
    std::mutex   errMu;                // guards err alone: argument checks report before `mu` is taken
    std::string  err;
    uint32_t*    d_queues = nullptr;   // ring of work-queue counters
    int          qslot = 0;
    int          cus = 0;
    int          encWaves = 0, decWaves = 0;
    // host-API staging (grown on demand): a ring of chunks in flight, each with pinned host memory, device memory and a stream
    // l1: level 1 in stages, the sequence records + chunk tables of one group of blocks (launch_l1), ordered by the slot's stream
    struct HostSlot { uint8_t* h = nullptr; size_t hcap = 0; uint8_t* d = nullptr; size_t dcap = 0; hipStream_t s = nullptr;
                      hipEvent_t evData = nullptr, evHash = nullptr; bool hashBusy = false; DeviceBuffer l1; };
    plz4hip_xxh32_stream* contentHash = nullptr;   // plz4hip_ctx_set_content_hash
    static constexpr int kSlots = 3;
    HostSlot     slot[kSlots];
    // The workspaces below belong to one job at a time each and are ordered across the callers' streams on the device: a
    // DeviceBuffer and the StreamOrder behind its last job (stream_ws.h).  Every one of them is listed in owned().
    DeviceBuffer hc;  int hcWaves = 0;                  // HC workspace, one slot per resident HC wave (allocated on first use)
    // level 12 in three phases: chain + search results of one group of blocks, the parser's table overflow, an error flag
    DeviceBuffer h12;  int h12ParseWaves = 0;  int h12SegWaves = 0;  int hcLazyWaves = 0;  size_t h12ErrOff = 0;
    StreamOrder  hcOrder;                               // one HC job at a time: hc, h12 and hcPfx
    hipStream_t  hashStream = nullptr;   // the streaming content checksum runs here, beside the codec kernels
    // the level-1 workspaces of the device-resident calls (the host-buffer calls have one per staging slot).  Two of them, so that calls on two streams need not
    // wait for each other: the emit kernels of one call then run beside the parse of the next (the second one is only
    // allocated when a second stream shows up while the first workspace is another stream's; PLZ4HIP_L1_WORKSPACES=1: one)
    static constexpr int kL1Shared = 2;
    DeviceBuffer l1[kL1Shared];  StreamOrder l1Order[kL1Shared];
    // The parse kernel of a staged call fills the device by itself (persistent workgroups around all of a CU's LDS).  Two of them
    // started together on two streams share the CUs half and half and stay in step, so that nothing of one call runs beside the
    // other's parse.  They are therefore ordered on the device: a call's parse on another stream than the last one's waits (behind
    // k_parse_gate) until that one has run its queue dry; it then moves into the CUs as the first one's workgroups leave, and the
    // emit kernels of the first call run beside it.
    int          l1Refused = 0;                // calls left before a refused second workspace is asked for again
    uint32_t*    d_gate = nullptr; uint32_t gateSeq = 0; hipStream_t gateStream = nullptr; bool gatePending = false; int gateBlocks = 0;
    // levels 3..11 on independent blocks: the list builder of the next group of blocks runs on this stream beside the walk of the
    // current one (launch_hc)
    hipStream_t  hcBuildStream = nullptr; hipEvent_t evHcFork = nullptr, evHcHist = nullptr, evHcChain[2] = {nullptr, nullptr}, evHcFree[2] = {nullptr, nullptr};
    // HC levels 3..12 with a dictionary / linked blocks on the list path: the blocks' segment lengths (k_hc_ext_prep), int32 each
    DeviceBuffer hcPfx;  int hcLazyExWaves = 0;
    // levels 3..12 on a few blocks: the counts and first slots of the pieces their chains and lists are built in (HbLayout), sized per call
    DeviceBuffer hb;
    int hcxWaves[4] = {0, 0, 0, 0};                     // resident waves of k_hcx<kRaw, kMid>, [kRaw + 2 * kMid]
    // LZ4_decompress_safe of a few blocks by the whole chip (lz4_dx_device.inl): its tables
    DeviceBuffer dx;  StreamOrder dxOrder;
    hipStream_t  dxHashStream = nullptr; hipEvent_t evDxFork = nullptr, evDxHash = nullptr;   // records: the block checksums beside the decode
    // the level-1 parse of a few blocks cut across the chip (lz4_fx_device.inl): pieces' states and records, sized per call
    DeviceBuffer fx;  StreamOrder fxOrder;
    // level 2 on a few independent blocks cut across the chip (lz4_mx_device.inl): pieces' states and records, sized per call
    DeviceBuffer mx;  StreamOrder mxOrder;
    // plz4hip_dev_encode_body_ex on the one-kernel encoder (PLZ4HIP_L1X=0, PLZ4HIP_L1_FUSED): its records before they are compacted
    DeviceBuffer xstage;  StreamOrder xstageOrder;
    // plz4hip_ctx_counters: [0] blocks encoded by the few-block level-1 path, [1] its rounds in the last such call, [2] pieces it
    // parsed more than once, [3] blocks answered by the few-block decoder, [4] blocks with history outside the block (dictionary,
    // linked) answered by it, [5] its jump rounds in the last such call (the maximum over the groups of a call cut into groups),
    // [6] the groups of the last call that was cut into groups, [7] blocks with history outside the block (dictionary, linked)
    // encoded by the few-block level-1 path (a subset of [0]), [8] blocks with history outside the block parsed by the bulk staged
    // route (k_l1x_parse), [9] blocks of at most 4 KiB under a dictionary context encoded by the wave-wide HC parser (k_hcx),
    // [13] blocks encoded by the few-block level-2 path, [14] its rounds that parsed something in the last such call, [15] pieces
    // it parsed more than once, [16] blocks with history outside the block encoded by the few-block level-2 path (a subset of [13]),
    // [17] blocks of levels 3..12 whose chain and lists were built in pieces across the chip (k_hb_count .. k_hb_chain), [18] the
    // pieces per block of the last such call (its largest segment + block, cut)
    static constexpr int kCounters = 19;
    unsigned long long* d_counters = nullptr;
    // plz4hip_dev_compress: the sanitised block lengths of the last call (int32 each), which that job's kernels read
    DeviceBuffer lenCopy;  StreamOrder lenOrder;
    // plz4hip_dev_decode_records_ex: the chainFirst of the last call (int32 each), which that job's kernels read
    DeviceBuffer chainCopy;  StreamOrder chainOrder;
    struct Owned { DeviceBuffer* buf; StreamOrder* order; bool trimmed; };     // trimmed: plz4hip_ctx_trim gives it back
    std::array<Owned, 12> owned()
    {
        return {{{&hc, &hcOrder, true}, {&h12, &hcOrder, true}, {&hcPfx, &hcOrder, false}, {&l1[0], &l1Order[0], true},
                 {&l1[1], &l1Order[1], true}, {&dx, &dxOrder, true}, {&fx, &fxOrder, true}, {&lenCopy, &lenOrder, false},
                 {&chainCopy, &chainOrder, false}, {&xstage, &xstageOrder, true}, {&mx, &mxOrder, true}, {&hb, &hcOrder, true}}};
    }
};

// == clz4.DictCtx (clz4.go:96-120): a private device copy of the last 64 KiB of the dictionary + the LZ4_loadDictSlow table.
// == xxh32.XXHZero (xxh32zero.go:58-86, :204-235): the stream state in device memory + an event behind its last update
struct plz4hip_xxh32_stream { XxhStream* d_state = nullptr; hipEvent_t done = nullptr; };

struct plz4hip_dict {
    uint8_t*  d_bytes = nullptr;  int len = 0;      // len < 8: the dictionary is dropped by liblz4 (lz4.c:1613-1615)
    uint32_t* d_table = nullptr;
    uint8_t*  d_hc = nullptr;                       // clz4.DictCtxHC: [level-2 tables][hash-chain tables], kHcWorkBytes each
    uint8_t*  d_hcx = nullptr;                      // the hash chain's positions as runs per hash (hcx_dict_build): [start][list], kHcxDictBytes
    std::vector<uint8_t> h_bytes;
};

namespace {

constexpr int kQueueSlots = 4096;

// LZ4_loadDict_internal(_ld_slow) on the host (lz4.c:1587-1646): the table a dictionary context carries.
void build_dict_table_slow(const uint8_t* p, int n, uint32_t* tab)
{
    memset(tab, 0, 4096 * sizeof(uint32_t));
    if (n < 8) return;
    auto hash5 = [](const uint8_t* q) { uint64_t v; memcpy(&v, q, 8); return (uint32_t)(((v << 24) * 889523592379ull) >> 52); };
    const uint32_t cur = 65536, base = cur - (uint32_t)n;
    for (int i = 0; i <= n - 8; i += 3) tab[hash5(p + i)] = base + (uint32_t)i;                 // later entries overwrite
    const uint32_t limit = cur - 65536;
    for (int i = 0; i <= n - 8; i++) { const uint32_t h = hash5(p + i); if (tab[h] <= limit) tab[h] = base + (uint32_t)i; }
}

int fail(plz4hip_ctx* c, int code, const char* what, hipError_t e = hipSuccess)
{
    if (c) {
        char buf[512];
        if (e != hipSuccess) snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
        else snprintf(buf, sizeof buf, "%s", what);
        std::lock_guard<std::mutex> g(c->errMu);
        c->err = buf;
    }
    return code;
}

// Entry points run on the ctx's device and leave the calling thread's current device as they found it.
struct DeviceGuard {
    int prev = -1; hipError_t err = hipSuccess;
    explicit DeviceGuard(int dev) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; if (prev != dev) err = hipSetDevice(dev); else prev = -1; }
    ~DeviceGuard() { if (prev >= 0) hipSetDevice(prev); }
};
#define ENTER_DEVICE(ctx) DeviceGuard dg_((ctx)->device); HIPCHK((ctx), dg_.err)

#define HIPCHK(ctx, call)                                                         \
    do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail((ctx), PLZ4HIP_E_DEVICE, #call, e_); } while (0)

uint32_t* next_queue(plz4hip_ctx* c, hipStream_t s, hipError_t* e)
{
    uint32_t* q = c->d_queues + c->qslot;
    c->qslot = (c->qslot + 1) % kQueueSlots;
    *e = hipMemsetAsync(q, 0, sizeof(uint32_t), s);
    return q;
}

// Zero a few bytes of device memory and wait for it -- on the ctx's own stream.  (A plain hipMemset would be the process's first
// use of the NULL stream, which then takes one of the four hardware queues: the staging slots of the host-buffer calls end up
// sharing queues and their chunks stop overlapping -- 2560 blocks through host memory 470 -> 790 ms, scripts/host_rate_ab.py.)
inline hipError_t zero_sync(plz4hip_ctx* c, void* p, size_t n)
{
    hipError_t e = hipMemsetAsync(p, 0, n, c->stream);
    return e == hipSuccess ? hipStreamSynchronize(c->stream) : e;
}

// ... and a small blocking copy the same way (hipMemcpy is a NULL-stream operation as well)
inline hipError_t copy_sync(plz4hip_ctx* c, void* dst, const void* src, size_t n, hipMemcpyKind kind)
{
    hipError_t e = hipMemcpyAsync(dst, src, n, kind, c->stream);
    return e == hipSuccess ? hipStreamSynchronize(c->stream) : e;
}

int ensure_slot(plz4hip_ctx* c, int i, size_t hostBytes, size_t devBytes)
{
    plz4hip_ctx::HostSlot& sl = c->slot[i];
    if (!sl.s && hipStreamCreateWithFlags(&sl.s, hipStreamNonBlocking) != hipSuccess) return fail(c, PLZ4HIP_E_DEVICE, "hipStreamCreate");
    if (hostBytes > sl.hcap) {
        if (sl.h) hipHostFree(sl.h);
        sl.h = nullptr; sl.hcap = 0;
        const size_t want = round_up(hostBytes + (hostBytes >> 3), 1 << 20);
        if (hipHostMalloc((void**)&sl.h, want, hipHostMallocDefault) != hipSuccess) return fail(c, PLZ4HIP_E_NOMEM, "hipHostMalloc");
        sl.hcap = want;
    }
    if (devBytes > sl.dcap) {
        if (sl.d) hipFree(sl.d);
        sl.d = nullptr; sl.dcap = 0;
        const size_t want = round_up(devBytes + (devBytes >> 3), 1 << 20);
        if (hipMalloc((void**)&sl.d, want) != hipSuccess) return fail(c, PLZ4HIP_E_NOMEM, "hipMalloc");
        sl.dcap = want;
    }
    return PLZ4HIP_OK;
}

// memcpy of many buffers on a few host threads (one thread cannot feed PCIe); small jobs stay on the caller's thread
template <class F> void parallel_blocks(int n, size_t totalBytes, F&& fn)
{
    unsigned hw = std::thread::hardware_concurrency();
    int nt = (int)(hw ? (hw < 8 ? hw : 8) : 4);
    if (totalBytes < ((size_t)8 << 20) || n < 2 || nt < 2) { for (int i = 0; i < n; ++i) fn(i); return; }
    if (nt > n) nt = n;
    std::atomic<int> next{0};
    auto work = [&]() { for (int i = next.fetch_add(1); i < n; i = next.fetch_add(1)) fn(i); };
    std::vector<std::thread> th;
    th.reserve((size_t)nt - 1);
    for (int t = 1; t < nt; ++t) th.emplace_back(work);
    work();
    for (auto& t : th) t.join();
}

int grid_for(int nBlocks, int resident) { return nBlocks < resident ? nBlocks : resident; }
// workgroups of the level-1 encoder kernels (kEncWavesPerWg waves each) for nBlocks blocks and `resident` resident waves
// Launch of a level-1 encoder kernel: ten-wave workgroups when the call has more blocks than nine-per-CU one-wave workgroups
// could hold at once, one-wave workgroups otherwise.
#define ENC_LAUNCH(kernel, nBlocks, c, s, ...) do { \
        const int waves_ = grid_for((nBlocks), (c)->encWaves); \
        if (waves_ > 9 * (c)->cus) hipLaunchKernelGGL(kernel<kEncWavesPerWg>, dim3((waves_ + kEncWavesPerWg - 1) / kEncWavesPerWg), dim3(64 * kEncWavesPerWg), 0, s, __VA_ARGS__); \
        else hipLaunchKernelGGL(kernel<1>, dim3(waves_), dim3(64), 0, s, __VA_ARGS__); \
    } while (0)

bool is_hc_level(int level) { return level >= 2 && level <= 12; }        // every row of the level table (lz4hc.c:92-106): mid, hash chain, optimal

// The one place that names the instantiations of these kernels: the occupancy queries and the launches ask here.
using Kernel1 = void (*)(CodecArgs);
using HcxKernel = void (*)(CodecArgs, unsigned long long*);
Kernel1 hc_mid_kernel(bool kD) { return !kD ? k_hc_mid<false> : k_hc_mid<true>; }
HcxKernel hcx_kernel(bool raw, bool mid) { return !mid ? (!raw ? k_hcx<false, false> : k_hcx<true, false>) : (!raw ? k_hcx<false, true> : k_hcx<true, true>); }
Kernel1 hc_lazy_kernel(bool kD) { return !kD ? k_hc_lazy<false> : k_hc_lazy<true>; }
Kernel1 hc_stitch_kernel(bool kD) { return kD ? k_hc_stitch<true> : k_hc_stitch<false>; }

int ensure_hc(plz4hip_ctx* c)
{
    if (c->hc.d) return PLZ4HIP_OK;
    // The HC parsers are one dependent memory access after another: the more waves a CU holds, the more of that latency
    // is hidden.  Fill every wave slot the register budget allows (workspace: 320 KiB per wave); PLZ4HIP_HC_WAVES_PER_CU
    // overrides for experiments.
    int per = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, k_encode_rec_hc, 64, 0) != hipSuccess || per < 1) per = 8;
    {   // (level 2's batch walk keeps its tables in these slots as well and holds more waves per CU than the one-thread parsers)
        int perMid = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perMid, hc_mid_kernel(false), 64, 0) == hipSuccess && perMid > per) per = perMid;
    }
    if (const char* v = getenv("PLZ4HIP_HC_WAVES_PER_CU")) { const int w = atoi(v); if (w >= 1 && w <= per) per = w; }
    const int waves = c->cus * per;
    bool refused = false;  HIPCHK(c, c->hc.reserve((size_t)waves * kHcWorkBytes, c->hcOrder, &refused));
    if (refused) return fail(c, PLZ4HIP_E_NOMEM, "HC workspace");
    c->hcWaves = waves;
    return PLZ4HIP_OK;
}

// The per-block HC workspace of at least `need` bytes; [0, 256) of a new one is zeroed (level 12's error flag, sticky).
int reserve_h12(plz4hip_ctx* c, size_t need, bool* refused)
{
    const bool grows = need > c->h12.bytes;
    HIPCHK(c, c->h12.reserve(need, c->hcOrder, refused));
    if (grows && !*refused) HIPCHK(c, zero_sync(c, c->h12.d, 256));
    return PLZ4HIP_OK;
}

// Level 12 on independent blocks without dictionary, levels 3..11 and the external-segment route: the group workspace of c->h12
// (HcLayout, ws_layout.h).  The group size follows from the memory set aside: hc_default_budget of what is free (and whatever the
// ctx holds already) unless PLZ4HIP_HC_BUDGET_GIB says more: the parser runs one wave per block, so the more blocks a group has (up
// to three waves per SIMD: 3072), the better its latency is hidden -- 4096 blocks in two groups of 2048 instead of four of 1024:
// 1418 -> 1664 MiB/s.  PLZ4HIP_HC12_GROUP overrides, for tests.  plz4hip_ctx_trim gives the memory back.
int plan_h12(plz4hip_ctx* c, const HcSwitches& sw, int nBlocks, int maxLen, HcLayout* pl, bool lazy, bool needF)
{
    size_t freeB = 0, totalB = 0;
    if (hipMemGetInfo(&freeB, &totalB) != hipSuccess) return fail(c, PLZ4HIP_E_DEVICE, "hipMemGetInfo");
    if (!c->h12ParseWaves) {
        int per = 0, perSeg = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, k_hc12_parse, 64, 0) != hipSuccess || per < 1) per = 8;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perSeg, k_hc12_seg, 64, 0) != hipSuccess || perSeg < 1) perSeg = 8;
        c->h12SegWaves = c->cus * perSeg;
        c->h12ParseWaves = c->cus * (per > perSeg ? per : perSeg);           // (sizes the waves' global price-table slots: the larger of the two grids)
    }
    const size_t perBlock = hc_layout(1, maxLen, lazy, needF, c->h12ParseWaves).perBlock;
    int rc = PLZ4HIP_OK;
    // groups of equal size: what is allocated is what one of them needs, whatever the budget would allow
    const int got = fit_groups(nBlocks, hc_first_group(freeB, c->h12.bytes, sw.budgetGiB, sw.h12Group, perBlock, nBlocks), true, [&](int per, bool* refused) {
        *pl = hc_layout(per, maxLen, lazy, needF, c->h12ParseWaves);
        if (getenv("PLZ4HIP_VERBOSE"))
            fprintf(stderr, "plz4hip: level 12, %d blocks: free %zu MiB, held %zu MiB, groups of %d (%zu MiB)\n", nBlocks, freeB >> 20, c->h12.bytes >> 20, pl->group, pl->total >> 20);
        return reserve_h12(c, pl->total, refused);
    }, &rc);
    if (rc) return rc;
    return got ? PLZ4HIP_OK : fail(c, PLZ4HIP_E_NOMEM, "level-12 workspace");
}

// The pointers of a group workspace at `base`, every per-block array moved on by k blocks (the half a group of an overlapped call uses)
void bind_hc(CodecArgs& a, uint8_t* base, const HcLayout& L, bool segs, int64_t k)
{
    a.h12ChainStride = L.chainStride; a.h12FStride = L.fStride;
    a.h12Chain = (uint16_t*)(base + L.offChain) + k * L.chainStride;
    a.h12Rank = (uint32_t*)(base + L.offRank) + k * L.chainStride;
    a.h12List = (uint32_t*)(base + L.offList) + k * (L.chainStride + 8);
    a.h12Offsets = (uint32_t*)(base + L.offOffsets) + k * kHcHashEntries;
    a.h12F = (Hc12F*)(base + L.offF) + k * L.fStride;
    a.h12Ws = base + L.offWs; a.h12Err = (int32_t*)(base + L.offErr);
    if (!segs) return;
    a.l1Seq = (uint64_t*)a.h12F; a.l1SeqStride = L.fStride; a.l1MaxChunks = L.maxChunks; a.l1Bk = nullptr;
    a.l1Info = (SeqInfo*)(base + L.offInfo) + k;
    a.l1ChunkBytes = (uint32_t*)(base + L.offChunkB) + k * L.maxChunks; a.l1ChunkOff = (uint32_t*)(base + L.offChunkO) + k * L.maxChunks;
    a.lzRecStride = L.recStride;
    a.lzRec = (uint64_t*)(base + L.offRec) + k * L.recStride; a.lzBridge = (uint64_t*)(base + L.offBridge) + k * L.recStride;
    a.lzMeta = (LzSegMeta*)(base + L.offMeta) + k * kLzMaxSegs; a.lzStarts = (uint64_t*)(base + L.offStarts) + k * kLzMaxSegs * kLzStarts;
    a.lzPieces = (LzPiece*)(base + L.offPieces) + k * 2 * kLzMaxSegs;
}

// ... and of the chain (and lists) built up front for the one-thread parsers
void bind_hc_pre(CodecArgs& a, uint8_t* base, const HcPreLayout& L, bool lists)
{
    a.h12Chain = (uint16_t*)(base + L.offChain); a.h12ChainStride = L.stride;
    a.h12Rank = lists ? (uint32_t*)(base + L.offRank) : nullptr;
    a.h12List = lists ? (uint32_t*)(base + L.offList) : nullptr;
    a.h12Offsets = lists ? (uint32_t*)(base + L.offOffsets) : nullptr;
}

// The launchers' switches (route.h), read once at the top of launch_l1 / launch_hc / launch_decode: every call sees the environment
// as it is when the call is made.
L1Switches read_l1_switches() { return parse_l1_switches([](const char* n) { return (const char*)getenv(n); }); }
MxSwitches read_mx_switches() { return parse_mx_switches([](const char* n) { return (const char*)getenv(n); }); }
HcSwitches read_hc_switches() { return parse_hc_switches([](const char* n) { return (const char*)getenv(n); }); }
DxSwitches read_dx_switches() { return parse_dx_switches([](const char* n) { return (const char*)getenv(n); }); }

// The emit stage of the ng blocks from g0 on: sizes, scan, write, checksums.  Back: level-1 records with catch-up; Mid: records
// without (level 2, the segmented HC walk); Seg: history outside the block (xb: the blocks' segments).  Waves per block so that a
// small call still spreads over the chip.  ctxSmall: the blocks <= 4 KiB under a dictionary context are k_fxl_small's -- their
// lengths before the records are placed in a body, else behind the stage.
enum class Emit { Back, Mid, Seg };
void launch_emit(hipStream_t s, const CodecArgs& a, int ng, int g0, int maxChunks, Emit kind, const FxlBlk* xb = nullptr, bool ctxSmall = false)
{
    int wg = (16384 / ng) / 4;
    if (wg > (maxChunks + 3) / 4) wg = (maxChunks + 3) / 4;
    if (wg < 1) wg = 1;
    if (kind == Emit::Seg) hipLaunchKernelGGL(k_fxl_sizes, dim3(wg, ng), dim3(256), 0, s, a, xb);
    else if (kind == Emit::Mid) hipLaunchKernelGGL(k_l1_sizes<false>, dim3(wg, ng), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_l1_sizes<true>, dim3(wg, ng), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_l1_scan, dim3((ng + 3) / 4), dim3(256), 0, s, a);
    if (ctxSmall && a.bodyOff) hipLaunchKernelGGL(k_fxl_small, dim3(ng < 1024 ? ng : 1024), dim3(64), 0, s, a);
    if (a.bodyOff) hipLaunchKernelGGL(k_scan_from, dim3(1), dim3(64), 0, s, (const int32_t*)(a.result + g0), a.bodyOff + g0, ng, g0 == 0 ? 1 : 0);
    if (kind == Emit::Seg) hipLaunchKernelGGL(k_fxl_write, dim3(wg, ng), dim3(256), 0, s, a, xb);
    else if (kind == Emit::Mid) hipLaunchKernelGGL(k_l1_write<false>, dim3(wg, ng), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_l1_write<true>, dim3(wg, ng), dim3(256), 0, s, a);
    if (!a.rawMode && a.blockChecksum) hipLaunchKernelGGL(k_l1_finish, dim3((ng + 15) / 16), dim3(64), 0, s, a);
    if (ctxSmall && !a.bodyOff) hipLaunchKernelGGL(k_fxl_small, dim3(ng < 1024 ? ng : 1024), dim3(64), 0, s, a);
}

// The block checksums of a record decode on the bulk path, in front of its launch (k_rec_verify16): every launch of k_decode_rec and
// of k_l1_duplex's decode side goes through here first.
void launch_rec_verify(hipStream_t s, const CodecArgs& d)
{
    if (d.blockChecksum && d.nBlocks > 0) hipLaunchKernelGGL(k_rec_verify16, dim3((d.nBlocks + 15) / 16), dim3(64), 0, s, d);
}
int launch_l1(plz4hip_ctx* c, hipStream_t s, CodecArgs a, int nb, int maxLen, int rawMode, DeviceBuffer* ws, bool* midDeclined = nullptr,
              const CodecArgs* rider = nullptr, bool hist = false, bool l1x = false, const L1Switches* read = nullptr);

// Enqueue one HC call of nb blocks (a: everything but queue / workspace filled in) on s.  rawMode: LZ4 blocks, else records.
int launch_hc_body(plz4hip_ctx* c, hipStream_t s, const HcSwitches& sw, CodecArgs a, int nb, int maxLen, int rawMode, bool* forked);
int launch_hc(plz4hip_ctx* c, hipStream_t s, CodecArgs a, int nb, int maxLen, int rawMode)
{
    const HcSwitches sw = read_hc_switches();
    HIPCHK(c, c->hcOrder.wait(s));
    // Whatever was enqueued uses the ctx's workspaces, also when the body left early: the call's stream joins the builder's
    // stream (a completed body has done so group by group) and the job is marked in any case, so that a following trim /
    // destroy / HC job waits for kernels that may still run.
    MarkOnExit job;
    job.arm(c->hcOrder, s);
    bool forked = false;
    const int rc = launch_hc_body(c, s, sw, a, nb, maxLen, rawMode, &forked);
    if (rc != PLZ4HIP_OK && forked && c->hcBuildStream && c->evHcFork
        && hipEventRecord(c->evHcFork, c->hcBuildStream) == hipSuccess) (void)hipStreamWaitEvent(s, c->evHcFork, 0);
    if (rc != PLZ4HIP_OK) return rc;
    HIPCHK(c, job.leave());
    return PLZ4HIP_OK;
}
struct HcCall { plz4hip_ctx* c; hipStream_t s; int nb, maxLen, rawMode; };    // what the routes' functions share

// the blocks' segments laid out, their lengths noted (k_hc_ext_prep)
int hc_prep_ext(const HcCall& k, CodecArgs& a)
{
    plz4hip_ctx* const c = k.c;  hipError_t e;
    if ((size_t)k.nb * 4 > c->hcPfx.bytes) {                                 // (grown with room for 256 blocks more)
        bool refused = false;  HIPCHK(c, c->hcPfx.reserve((size_t)k.nb * 4 + 1024, c->hcOrder, &refused));
        if (refused) return fail(c, PLZ4HIP_E_NOMEM, "HC segment lengths");
    }
    a.hcPfx = (int32_t*)c->hcPfx.d; a.rawMode = k.rawMode; a.nBlocks = k.nb; a.blk0 = 0;
    a.queue = next_queue(c, k.s, &e); HIPCHK(c, e);
    hipLaunchKernelGGL(k_hc_ext_prep, dim3(grid_for(k.nb, c->cus * 8)), dim3(64), 0, k.s, a);
    return PLZ4HIP_OK;
}
// every block of the call that is k_hcx's, one launch
int hc_hcx_blocks(const HcCall& k, CodecArgs x)
{
    plz4hip_ctx* const c = k.c;  hipError_t e;
    const bool mid = x.level == 2;
    const HcxKernel kern = hcx_kernel(k.rawMode != 0, mid);
    const int which = (k.rawMode ? 1 : 0) + (mid ? 2 : 0);
    if (!c->hcxWaves[which]) {                                               // (of the instantiation that is launched)
        int per = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, (const void*)kern, 64, 0) != hipSuccess || per < 1) per = 7;
        c->hcxWaves[which] = c->cus * per;
    }
    int waves = c->hcxWaves[which];
    if (mid || x.level >= 10) {                                              // (a price table / the records per wave: the HC workspace's)
        if (int rc = ensure_hc(c)) return rc;
        x.hcWork = c->hc.d;
        if (c->hcWaves < waves) waves = c->hcWaves;
    }
    x.blk0 = 0; x.nBlocks = k.nb;
    x.queue = next_queue(c, k.s, &e); HIPCHK(c, e);
    hipLaunchKernelGGL(kern, dim3(grid_for(k.nb, waves)), dim3(64), 0, k.s, x, c->d_counters);
    HIPCHK(c, hipGetLastError());
    return PLZ4HIP_OK;
}
// the blocks <= 4 KiB under a dictionary context (hcPfx < 0; the emit stage has laid them down as stored records in the meantime):
// k_hcx, or the one-thread parser over the context's two sets of tables, writes them now
int hc_ctx_blocks(const HcCall& k, const CodecArgs& a0)
{
    plz4hip_ctx* const c = k.c;  hipError_t e;
    if (a0.hcx) return hc_hcx_blocks(k, a0);
    if (int rc = ensure_hc(c)) return rc;
    CodecArgs x = a0; x.hcWork = c->hc.d; x.blk0 = 0; x.nBlocks = k.nb; x.h12Chain = nullptr; x.h12Rank = nullptr; x.h12List = nullptr;
    x.queue = next_queue(c, k.s, &e); HIPCHK(c, e);
    if (k.rawMode) hipLaunchKernelGGL(k_encode_raw_hc, dim3(grid_for(k.nb, c->hcWaves)), dim3(64), 0, k.s, x);
    else           hipLaunchKernelGGL(k_encode_rec_hc, dim3(grid_for(k.nb, c->hcWaves)), dim3(64), 0, k.s, x);
    HIPCHK(c, hipGetLastError());
    return PLZ4HIP_OK;
}
// the histogram and / or the chain and lists of x's blocks on st; hb: both, in pieces (c->hb holds HbLayout of at least x.nBlocks blocks)
int hc_build(plz4hip_ctx* c, hipStream_t st, CodecArgs x, bool hist, bool chain, const HbWant* hb = nullptr)
{
    hipError_t e;
    if (hb) {
        const HbLayout L = hb_layout(x.nBlocks, hb->P);
        const HbArgs h{(uint32_t*)(c->hb.d + L.offCnt), (uint32_t*)(c->hb.d + L.offSlot), hb->P, hb->piece, c->d_counters};
        const int nb = x.nBlocks;
        int cw = (int)((x.h12ChainStride + 255) / 256);                      // chain: about eight workgroups per CU over the call
        if (cw > (c->cus * 8 + nb - 1) / nb) cw = (c->cus * 8 + nb - 1) / nb;
        hipLaunchKernelGGL(k_hb_count, dim3(hb->P, nb), dim3(1024), 0, st, x, h);
        hipLaunchKernelGGL(k_hb_scan, dim3(nb), dim3(1024), 0, st, x, h);
        hipLaunchKernelGGL(k_hb_fill, dim3(hb->P, nb), dim3(64), 0, st, x, h);
        hipLaunchKernelGGL(k_hb_chain, dim3(cw, nb), dim3(256), 0, st, x, h);
        return PLZ4HIP_OK;
    }
    if (hist)  { x.queue = next_queue(c, st, &e); HIPCHK(c, e); hipLaunchKernelGGL(k_hc12_hist, dim3(grid_for(x.nBlocks, c->cus)), dim3(1024), 0, st, x); }
    if (chain) { x.queue = next_queue(c, st, &e); HIPCHK(c, e); hipLaunchKernelGGL(k_hc12_chain, dim3(grid_for(x.nBlocks, c->cus)), dim3(64), 0, st, x); }
    return PLZ4HIP_OK;
}

// Segmented (route.h).  Levels 3..12 with a dictionary and/or linked blocks take the same route as the lazy levels -- chain and lists
// over segment + block, the walk in segments, stitched, records through the emit stage -- with the segment rules of the reference
// kept in the finders (lz4hc_lazy_device.inl, kD); only the blocks <= 4 KiB under a dictionary context are launched behind.
// Levels 3..11: the list builder is one wave per CU around 128 KiB of LDS (0.3 s per 2048 blocks with the chip all but idle), the
// walk needs no LDS.  A call of enough blocks therefore runs in at least four groups over the two halves of the workspace, the
// builder of group g+1 on a second stream beside the walk of group g (which leaves it a wave slot per CU); the histogram of group
// g+1 (1024-thread workgroups that would not find room beside the walk) runs between two walks.
int hc_segmented(const HcCall& k, const HcSwitches& sw, const HcPlan& p, CodecArgs a, bool* forked)
{
    plz4hip_ctx* const c = k.c;  const hipStream_t s = k.s;  hipError_t e;
    const int nb = k.nb;
    HcLayout pl;
    if (int rc = plan_h12(c, sw, nb, k.maxLen + (p.lazyEx ? 65536 : 0), &pl, p.segs, !p.lazy)) return rc;
    if (p.prepExt) { if (int rc = hc_prep_ext(k, a)) return rc; }
    c->h12ErrOff = pl.offErr;
    a.rawMode = k.rawMode;
    if (p.segs) {
        if (p.lazy && a.level >= 10) { if (int rc = ensure_hc(c)) return rc; a.hcWork = c->hc.d; }
        if (!c->hcLazyWaves) {
            int per = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, hc_lazy_kernel(false), 64, 0) != hipSuccess || per < 1) per = 8;
            c->hcLazyWaves = c->cus * per;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, hc_lazy_kernel(true), 64, 0) != hipSuccess || per < 1) per = 8;
            c->hcLazyExWaves = c->cus * per;
        }
        a.l1MaxLen = k.maxLen;
        a.lzMinSeg = p.lzMinSeg;
    }
    a.h12Gather = p.gather; a.h12Idle = p.idle;
    bind_hc(a, c->h12.d, pl, p.segs, 0);
    HIPCHK(c, hipMemsetAsync(a.h12Err, 0, 4, s));                          // the give-up flag is per call (k_hc12_parse reports it per block)
    const HcGroups g = hc_groups(nb, pl.group, p.lazy, sw);
    const bool overlap = g.overlap;
    const int per = g.per, nGroups = g.nGroups;
    // few blocks: chain and lists in pieces across the chip, when the pieces' own workspace is granted (else today's builder)
    const HbWant hbw = hb_want(HbShape{a.level, nb, k.maxLen, k.maxLen + (p.lazyEx ? 65536 : 0), true, overlap}, sw);
    bool hbGranted = false;
    if (hbw.on) {
        bool refused = false;  HIPCHK(c, c->hb.reserve(hb_layout(per, hbw.P).total, c->hcOrder, &refused));
        hbGranted = !refused;
    }
    const HbWant* const hbp = hb_route(hbw, hbGranted) ? &hbw : nullptr;
    if (overlap) {
        if (!c->hcBuildStream) HIPCHK(c, hipStreamCreateWithFlags(&c->hcBuildStream, hipStreamNonBlocking));
        for (hipEvent_t* ev : {&c->evHcFork, &c->evHcHist, &c->evHcChain[0], &c->evHcChain[1], &c->evHcFree[0], &c->evHcFree[1]})
            if (!*ev) HIPCHK(c, hipEventCreateWithFlags(ev, hipEventDisableTiming));
    }
    const CodecArgs a0 = a;
    // the workspace pointers of the half group gi uses (every per-block array moved on by at blocks), and the group's blocks
    const auto group = [&](int at, int gi) { CodecArgs x = a0; bind_hc(x, c->h12.d, pl, p.segs, at); x.blk0 = g.gStart[gi]; x.nBlocks = g.gSize[gi]; return x; };
    const hipStream_t sb = c->hcBuildStream;
    if (overlap) {
        HIPCHK(c, hipEventRecord(c->evHcFork, s));
        HIPCHK(c, hipStreamWaitEvent(sb, c->evHcFork, 0));
        *forked = true;
        if (int rc = hc_build(c, sb, group(0, 0), true, true)) return rc;
        HIPCHK(c, hipEventRecord(c->evHcChain[0], sb));
        if (nGroups > 1) {
            if (int rc = hc_build(c, sb, group(per, 1), true, false)) return rc;
            HIPCHK(c, hipEventRecord(c->evHcHist, sb));
        }
    }
    for (int gi = 0; gi < nGroups; ++gi) {
        const int ng = g.gSize[gi];
        if (overlap) a = group((gi & 1) * per, gi);
        a.blk0 = g.gStart[gi]; a.nBlocks = ng;
        if (overlap) {
            HIPCHK(c, hipStreamWaitEvent(s, c->evHcChain[gi & 1], 0));
            if (gi + 1 < nGroups) {
                HIPCHK(c, hipStreamWaitEvent(s, c->evHcHist, 0));               // the next group's histogram is done: its builder starts now
                if (int rc = hc_build(c, sb, group(((gi + 1) & 1) * per, gi + 1), false, true)) return rc;
                HIPCHK(c, hipEventRecord(c->evHcChain[(gi + 1) & 1], sb));
            }
        } else {
            if (int rc = hc_build(c, s, a, true, true, hbp)) return rc;
        }
        a.queue = next_queue(c, s, &e); HIPCHK(c, e);
        if (!p.lazy) hipLaunchKernelGGL(k_hc12_search, dim3(grid_for(ng, c->cus)), dim3(1024), 0, s, a);
        a.queue = next_queue(c, s, &e); HIPCHK(c, e);
        if (!p.segs) hipLaunchKernelGGL(k_hc12_parse, dim3(grid_for(ng, c->h12ParseWaves)), dim3(64), 0, s, a);
        else {
            // segments per block: as many as there are 8 KiB pieces, at most 512.  Measured at 4096 blocks of 4 MiB, level 3 /
            // level 9: 16 segments 7522 / 4870, 32: 7734 / 4986, 64: 7908 / 5090, 128: 8071 / 5691, 256: 8279 / 5958, 512: 8602 /
            // 6139, 1024: 8642 / 6159 MiB/s.  Far more walks than the chip holds waves: the queue hands neighbouring segments of
            // one block to neighbouring waves, which then share the block's source and lists in L2, and short items even out.
            a.lzSegs = p.lzSegs;
            if (p.seg12) {
                hipLaunchKernelGGL(k_hc12_seg, dim3(grid_for(ng * a.lzSegs, c->h12SegWaves)), dim3(64), 0, s, a);
                a.queue = next_queue(c, s, &e); HIPCHK(c, e);
                hipLaunchKernelGGL(k_hc12_stitch, dim3(grid_for(ng, c->h12SegWaves)), dim3(64), 0, s, a);
            } else {
                const int resident = p.lazyEx ? c->hcLazyExWaves : c->hcLazyWaves;
                int lzWaves = a.level >= 10 && c->hcWaves < resident ? c->hcWaves : resident;   // (a price table per wave)
                if (overlap && lzWaves > 2 * c->cus) lzWaves -= c->cus;                    // a wave slot (and its registers) per CU for the builder
                hipLaunchKernelGGL(hc_lazy_kernel(p.lazyEx), dim3(grid_for(ng * a.lzSegs, lzWaves)), dim3(64), 0, s, a);
                a.queue = next_queue(c, s, &e); HIPCHK(c, e);
                hipLaunchKernelGGL(hc_stitch_kernel(p.lazyEx), dim3(grid_for(ng, lzWaves)), dim3(64), 0, s, a);
            }
            hipLaunchKernelGGL(k_hc_gather, dim3(ng >= 1024 ? 4 : 16, ng), dim3(256), 0, s, a);
            launch_emit(s, a, ng, 0, pl.maxChunks, Emit::Mid);
        }
        HIPCHK(c, hipGetLastError());
        if (overlap && gi + 2 < nGroups) {
            // this half is free again: the histogram of the group after next may overwrite it
            HIPCHK(c, hipEventRecord(c->evHcFree[gi & 1], s));
            HIPCHK(c, hipStreamWaitEvent(sb, c->evHcFree[gi & 1], 0));
            if (int rc = hc_build(c, sb, group((gi & 1) * per, gi + 2), true, false)) return rc;
            HIPCHK(c, hipEventRecord(c->evHcHist, sb));
        }
    }
    return p.ctxBlocks ? hc_ctx_blocks(k, a0) : PLZ4HIP_OK;
}

// OneThread (route.h).  pre -- levels 3..12, independent blocks: the chain of every block built up front (2 B per position): the
// parsers then run without their 4 M dependent table updates per 4 MiB block.  Levels 4..12 (8 candidates and more per search) also
// get the per-hash lists (another 8 B per position): their searches then look at up to 63 candidates per round
// (hc_find_wider_lists).  A call whose blocks do not fit the memory set aside runs in groups of equal size.
int hc_one_thread(const HcCall& k, const HcSwitches& sw, const HcPlan& p, CodecArgs a)
{
    plz4hip_ctx* const c = k.c;  const hipStream_t s = k.s;  hipError_t e;
    const int nb = k.nb, maxLen = k.maxLen;
    if (int rc = ensure_hc(c)) return rc;
    a.hcWork = c->hc.d; a.nBlocks = nb;
    a.h12Chain = nullptr;
    a.blk0 = 0;
    int per = nb;                     // blocks per launch
    bool lists = false;
    if (p.pre) {
        size_t freeB = 0, totalB = 0;
        if (hipMemGetInfo(&freeB, &totalB) != hipSuccess) return fail(c, PLZ4HIP_E_DEVICE, "hipMemGetInfo");
        // The budget: hc_default_budget, for the chain alone and for the lists alike.  The lists are worth more memory than that:
        // these kernels live on the number of blocks in flight (7 waves per SIMD fit), and 4096 blocks of 4 MiB with their lists
        // (40 MiB each) are 160 GiB: a machine that is there for this sets PLZ4HIP_HC_BUDGET_GIB; plz4hip_ctx_trim gives it back.
        // What the ctx already holds is used in any case.
        const HcPrePlan pp = hc_pre_plan(freeB, c->h12.bytes, sw.budgetGiB, sw.group, sw.listsOff, a.level, nb, maxLen);
        lists = pp.lists;
        if (lists && pp.perLists > c->h12.bytes / hc_pre_layout(1, maxLen, true).perBlock) {   // try the large request first: refused -> the chain alone
            bool refused = false;  if (int rc = reserve_h12(c, hc_pre_layout(pp.perLists, maxLen, true).total, &refused)) return rc;
            if (refused) lists = false;
        }
        const int perPre = lists ? pp.perLists : pp.perChain;
        if (getenv("PLZ4HIP_VERBOSE"))
            fprintf(stderr, "plz4hip: HC level %d, %d blocks: free %zu MiB, held %zu MiB, lists %d, %d blocks per group\n", a.level, nb,
                    freeB >> 20, c->h12.bytes >> 20, (int)lists, perPre);
        if (perPre >= 1) {
            per = perPre;
            const HcPreLayout L = hc_pre_layout(per, maxLen, lists);
            bool refused = false;  if (int rc = reserve_h12(c, L.total, &refused)) return rc;
            if (refused) return fail(c, PLZ4HIP_E_NOMEM, "HC chain workspace");
            bind_hc_pre(a, c->h12.d, L, lists);
        }
    }
    for (int g0 = 0; g0 < nb; g0 += per) {
        const int ng = nb - g0 < per ? nb - g0 : per;
        a.blk0 = g0; a.nBlocks = ng;
        if (a.h12Chain && lists) {
            if (int rc = hc_build(c, s, a, true, true)) return rc;
        } else if (a.h12Chain) {
            a.queue = next_queue(c, s, &e); HIPCHK(c, e);
            hipLaunchKernelGGL(k_hc_chain, dim3(grid_for(ng, c->cus)), dim3(64), 0, s, a);
        }
        a.queue = next_queue(c, s, &e); HIPCHK(c, e);
        if (k.rawMode) hipLaunchKernelGGL(k_encode_raw_hc, dim3(grid_for(ng, c->hcWaves)), dim3(64), 0, s, a);
        else           hipLaunchKernelGGL(k_encode_rec_hc, dim3(grid_for(ng, c->hcWaves)), dim3(64), 0, s, a);
        HIPCHK(c, hipGetLastError());
    }
    if (p.hcxBehind) { a.hcPfx = nullptr; return hc_hcx_blocks(k, a); }        // (the one-thread kernels passed them over)
    return PLZ4HIP_OK;
}

int launch_hc_body(plz4hip_ctx* c, hipStream_t s, const HcSwitches& sw, CodecArgs a, int nb, int maxLen, int rawMode, bool* forked)
{
    const HcCall k{c, s, nb, maxLen, rawMode};
    const HcShape shape{a.level, nb, maxLen, rawMode != 0, a.hcEx != 0, a.dict != nullptr, a.dictLen >= 0, a.linked != 0, a.hcxStart != nullptr};
    HcPlan p = hc_route(shape, sw);
    a.hcx = p.hcx;
    // many small records under one dictionary: no segments to lay out, no lists in device memory, no workspace
    if (p.route == HcRoute::HcxOnly) { a.hcPfx = nullptr; return hc_hcx_blocks(k, a); }
    if (p.route == HcRoute::MidStaged) {
        // level 2, blocks up to 4 MiB: the staged call of level 1 with the level-2 walk as its parser (behind external segments too)
        if (int rc = ensure_hc(c)) return rc;
        a.hcWork = c->hc.d;
        if (p.prepExt) { if (int rc = hc_prep_ext(k, a)) return rc; }
        bool declined = false;
        if (int rc = launch_l1(c, s, a, nb, maxLen, rawMode, nullptr, &declined)) return rc;
        if (!declined) return p.ctxBlocks ? hc_ctx_blocks(k, a) : PLZ4HIP_OK;
        a.hcPfx = nullptr;                                                   // (no workspace: every block on the one-thread parser)
        p = hc_route(shape, sw, true);
    }
    return p.route == HcRoute::Segmented ? hc_segmented(k, sw, p, a, forked) : hc_one_thread(k, sw, p, a);
}

// The pointers of a level-1 group workspace (L1Layout) and of a few-block parse's (PieceLayout; returns the blocks' FxlBlk array)
void bind_l1(CodecArgs& a, uint8_t* base, const L1Layout& L)
{
    a.l1SeqStride = (int64_t)L.seqStride; a.l1MaxChunks = L.maxChunks;
    a.l1Info = (SeqInfo*)(base + L.offInfo);
    a.l1ChunkBytes = (uint32_t*)(base + L.offChunkBytes); a.l1ChunkOff = (uint32_t*)(base + L.offChunkOff);
    a.l1Seq = (uint64_t*)(base + L.offSeq); a.l1Bk = base + L.offBk;
}
FxlBlk* bind_pieces(PieceArgs& pc, uint8_t* base, const PieceLayout& L, bool hist)
{
    pc.meta = (PieceMeta*)(base + L.offMeta); pc.tabIn = (uint32_t*)(base + L.offIn); pc.tabOut = (uint32_t*)(base + L.offOut);
    pc.rec = (uint64_t*)(base + L.offRec);
    return hist ? (FxlBlk*)(base + L.offBlk) : nullptr;
}
// The rounds of one group of a few-block call and the gather behind them (K: KFx, KFxl, KMx, KMxl).  P rounds are always enough
// (lz4_pieces_device.inl); the rounds after the last change find nothing to do.  first: the call's first group.
template <class K> void launch_piece_rounds(hipStream_t s, const CodecArgs& a, const PieceArgs& pc, FxlBlk* xb, int ng, bool first)
{
    if (first) hipLaunchKernelGGL(k_piece_begin, dim3(1), dim3(64), 0, s, pc.cnt, (int)K::kRounds);
    // (every block reads block gi - 1's plaintext tail out of the call's input, whichever group that block is in)
    if (K::kHist) hipLaunchKernelGGL(k_fxl_prep, dim3(ng), dim3(64), 0, s, a, pc, xb);
    for (int r = 1; r <= pc.P; ++r) hipLaunchKernelGGL(k_piece<K>, dim3(pc.P, ng), dim3(64), 0, s, a, pc, (const FxlBlk*)xb, r);
    hipLaunchKernelGGL(k_piece_gather<K>, dim3(pc.P, ng), dim3(64), 0, s, a, pc, (const FxlBlk*)xb);
}

// Which of the ctx's level-1 workspaces a call on s takes: the one this stream used last; else one whose last job is over (no second
// allocation for streams that merely take turns); else one that does not exist yet; else the first one (and the wait for it).
int pick_l1_workspace(plz4hip_ctx* c, hipStream_t s, const L1Switches& sw)
{
    const int nws = sw.oneWorkspace ? 1 : plz4hip_ctx::kL1Shared;
    int mine = -1, idle = -1, fresh = -1;
    for (int i = 0; i < nws; ++i) {
        if (c->l1[i].d && c->l1Order[i].stream == s && mine < 0) mine = i;
        if (c->l1[i].d && idle < 0 && c->l1Order[i].idle()) idle = i;
        if (!c->l1[i].d && fresh < 0) fresh = i;
    }
    return mine >= 0 ? mine : (idle >= 0 ? idle : (fresh >= 0 ? fresh : 0));
}

// The parse launch of a group of the staged call that fills the device (Parse, Duplex): ordered behind the other stream's by the gate
int l1_gate(plz4hip_ctx* c, hipStream_t s, CodecArgs& a, int ng)
{
    // (only behind a launch that fills the device: the parse launches of the host-buffer calls' chunks -- a third of the
    // wave slots each -- are meant to share it, and behind the gate they would run one after the other: 2560 blocks through
    // host memory 470 -> 680 ms)
    if (c->gatePending && c->gateStream != s && c->gateBlocks >= 8 * c->cus)
        hipLaunchKernelGGL(k_parse_gate, dim3(1), dim3(64), 0, s, (const uint32_t*)c->d_gate, c->gateSeq);
    if (c->gateSeq >= 0x7FFF0000u) {                                    // (once in two billion launches: start over)
        HIPCHK(c, hipDeviceSynchronize()); HIPCHK(c, zero_sync(c, c->d_gate, sizeof(uint32_t))); c->gateSeq = 0;
    }
    a.gate = c->d_gate; a.gateSeq = ++c->gateSeq;
    c->gatePending = true; c->gateStream = s; c->gateBlocks = ng;
    return PLZ4HIP_OK;
}

// One parse launch shared with the record decode of another call: workgroups of P + D waves, what the device holds at once unless
// neither role has that much to do
int launch_duplex(plz4hip_ctx* c, hipStream_t s, const L1Switches& sw, const CodecArgs& a, const CodecArgs& rider, int ng)
{
    const int P = sw.duplexP, D = sw.duplexD;
#define DUPLEX_CASE(PP, DD) \
    if (P == PP && D == DD) { \
        int wgs = ((ng + PP - 1) / PP > (rider.nBlocks + DD - 1) / DD) ? (ng + PP - 1) / PP : (rider.nBlocks + DD - 1) / DD; \
        const int hold = c->cus * duplex_wgs_per_cu(PP, DD); \
        if (wgs > hold) wgs = hold; \
        if (sw.duplexPrio) hipLaunchKernelGGL((k_l1_duplex<PP, DD, 3>), dim3(wgs), dim3(64 * (PP + DD)), 0, s, a, rider); \
        else               hipLaunchKernelGGL((k_l1_duplex<PP, DD, 0>), dim3(wgs), dim3(64 * (PP + DD)), 0, s, a, rider); \
        return PLZ4HIP_OK; \
    }
    DUPLEX_CASE(1, 1) DUPLEX_CASE(1, 2) DUPLEX_CASE(3, 4) DUPLEX_CASE(9, 7)      // (9+5, 9+3, 3+2 measured as well: DESIGN 3.1b)
#undef DUPLEX_CASE
    return fail(c, PLZ4HIP_E_ARG, "PLZ4HIP_DUPLEX: not a built combination");
}

// Enqueue one level-1 call of nb blocks (a: everything but queue / workspace filled in) on s; the routes and their fallbacks: route.h,
// DESIGN 2.  rawMode: LZ4 blocks (result = bytes or 0), else records.  The staged routes' workspace holds 8 bytes per possible
// sequence -- 2 bytes per input byte -- of one group of blocks; a call that does not fit the memory set aside (half of what is free;
// PLZ4HIP_L1_BUDGET_GIB) runs in groups of equal size.  ws: the workspace to use (a staging slot's own, always used from that slot's
// stream) or null for the ctx's, which is ordered across streams.
// midDeclined: the call is a level-2 call; set when no workspace could be had, the caller then runs its one-kernel path.
// rider: the record decode of another call (queue filled in) that shares the parse kernel's launch; a call that runs in groups
// carries it in its first group, one that takes the fused kernels launches it by itself.
// hist: the blocks have history outside the block (a: dictionary / linked fields filled in, 64 KiB of room in front of every input
// block); l1x: from the device-resident entry points, whose workspace carries one FxlBlk per block of a group behind the records.
int launch_l1(plz4hip_ctx* c, hipStream_t s, CodecArgs a, int nb, int maxLen, int rawMode, DeviceBuffer* ws, bool* midDeclined,
              const CodecArgs* rider, bool hist, bool l1x, const L1Switches* read)
{
    hipError_t e;
    const L1Switches sw = read ? *read : read_l1_switches();                    // (read: the caller had to ask l1_want itself)
    const bool mid = midDeclined != nullptr;
    const L1Shape shape{nb, maxLen, rawMode != 0, mid, rider != nullptr, hist, l1x, a.bodyOff != nullptr, hist && a.dictLen >= 8};
    const L1Want want = l1_want(shape, sw);
    // level 2: whether the few-block walk takes the call (read once; a level-1 call never asks)
    // (a.hcPfx: the blocks have history outside the block and k_hc_ext_prep has noted their segments -- mxl_want's calls)
    const bool mxl = mid && a.hcPfx != nullptr;
    const MxShape mxShape{a.level, nb, maxLen, a.hcEx != 0 || a.hcPfx != nullptr, rider != nullptr};
    const MxWant mxWant = !mid ? MxWant{} : mxl ? mxl_want(mxShape, read_mx_switches()) : mx_want(mxShape, read_mx_switches());
    a.rawMode = rawMode; a.blk0 = 0; a.nBlocks = nb;
    const bool shared = (ws == nullptr);
    int wsi = 0;
    if (shared) { wsi = pick_l1_workspace(c, s, sw); ws = &c->l1[wsi]; }
    bool granted = want.staged;
    const auto need_for = [&](int per) { return l1_layout(per, maxLen, l1x).total; };
    int per = nb;
    if (shared && granted && wsi != 0 && !ws->d && c->l1Refused > 0) { c->l1Refused--; wsi = 0; ws = &c->l1[0]; }   // (refused a moment ago)
    if (shared && granted && wsi != 0 && !ws->d) {
        // a SECOND workspace is there for overlap: it is taken whole or not at all (a smaller one would cut this call into groups,
        // which costs more than waiting for the first workspace does)
        bool refused = false;  HIPCHK(c, ws->reserve(need_for(nb), c->l1Order[wsi], &refused));
        if (refused) {
            wsi = 0; ws = &c->l1[0]; c->l1Refused = 8;                           // (the next calls do not ask again)
            if (getenv("PLZ4HIP_VERBOSE")) fprintf(stderr, "plz4hip: level 1: no room for a second workspace of %zu MiB, sharing the first\n", need_for(nb) >> 20);
        }
    }
    StreamOrder* const order = shared ? &c->l1Order[wsi] : nullptr;                      // (a slot's own workspace: the slot's stream)
    if (granted && need_for(nb) > ws->bytes) {
        size_t freeB = 0, totalB = 0;
        if (hipMemGetInfo(&freeB, &totalB) != hipSuccess) return fail(c, PLZ4HIP_E_DEVICE, "hipMemGetInfo");
        int rc = PLZ4HIP_OK;
        const int64_t grp = l1_first_group(freeB, ws->bytes, sw.budgetGiB, sw.budgetMiB, l1_layout(1, maxLen, l1x).perBlock, nb);
        const int got = fit_groups(nb, grp, false, [&](int p, bool* refused) {
            per = p;
            HIPCHK(c, order ? ws->reserve(need_for(per), *order, refused) : ws->reserve(need_for(per), s, refused));
            return (int)PLZ4HIP_OK;
        }, &rc);
        if (rc) return rc;
        if (!got) granted = false;                                                      // not even one block: the kernels that need no workspace
        if (getenv("PLZ4HIP_VERBOSE"))
            fprintf(stderr, "plz4hip: level 1, %d blocks of <= %d: free %zu MiB, workspace %zu MiB, groups of %d%s\n", nb, maxLen, freeB >> 20, ws->bytes >> 20, per, granted ? "" : " (fused)");
    }
    // from here on the jobs are marked behind whatever was enqueued, whichever way the call ends
    MarkOnExit job, pcJob;
    PieceArgs pc{};
    bool pcGranted = false;                                                     // the pieces' workspace of this call (c->fx, or c->mx for level 2)
    FxlBlk* xb = nullptr;                                                       // hist: per block of a group, its segment (k_fxl_prep)
    L1Layout L{};
    if (granted) {
        if (order) { HIPCHK(c, order->wait(s)); job.arm(*order, s); }
        L = l1_layout(per, maxLen, l1x);
        a.l1MaxLen = maxLen;
        bind_l1(a, ws->d, L);
        const PieceCut cut = mid ? mxWant.cut() : want.cut();
        if (cut.on) {
            // a few-block parse's workspace is sized per call (a group of `per` blocks); when it cannot be had, the call parses as the
            // others: level 1 on the ordinary parse, level 2 one wave per block (k_hc_mid) -- same bytes
            DeviceBuffer& buf = mid ? c->mx : c->fx;
            StreamOrder& ord = mid ? c->mxOrder : c->fxOrder;
            pc.pb = cut.piece; pc.warm = cut.warm; pc.P = cut.P; pc.recStride = piece_rec_stride(pc.pb); pc.cnt = c->d_counters;
            const bool blk = hist && !mid;                                      // (level 2's pieces never carry an FxlBlk array)
            const PieceLayout PL = piece_layout(per, pc.P, pc.recStride, mid ? kMxTab : kFxTab, blk);
            HIPCHK(c, ord.wait(s));
            bool refused = false;  HIPCHK(c, buf.reserve(PL.total, ord, &refused));
            if (!refused) { xb = bind_pieces(pc, buf.d, PL, blk); pcGranted = true; pcJob.arm(ord, s); }
        }
    }
    const L1Route route = l1_route(shape, sw, want, granted, pcGranted);
    const bool mxOn = route == L1Route::Mid && mx_route(mxWant, granted, pcGranted);
    switch (route) {
    case L1Route::NoMemBody:
        return fail(c, PLZ4HIP_E_NOMEM, "records straight into a frame body need the staged call's workspace (blocks up to 4 MiB)");
    case L1Route::MidDeclined:                                                  // (the one-thread parsers write staged records too)
        *midDeclined = true; return PLZ4HIP_OK;
    case L1Route::DictKernels: case L1Route::Fused:
        a.blk0 = 0; a.nBlocks = nb;
        a.queue = next_queue(c, s, &e); HIPCHK(c, e);
        if (route == L1Route::DictKernels) { if (rawMode) ENC_LAUNCH(k_encode_raw_dict, nb, c, s, a); else ENC_LAUNCH(k_encode_rec_dict, nb, c, s, a); }
        else                               { if (rawMode) ENC_LAUNCH(k_encode_raw, nb, c, s, a); else ENC_LAUNCH(k_encode_rec, nb, c, s, a); }
        if (route == L1Route::Fused && rider) { launch_rec_verify(s, *rider); hipLaunchKernelGGL(k_decode_rec, dim3(grid_for(rider->nBlocks, c->decWaves)), dim3(64), 0, s, *rider); }
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, job.leave());
        HIPCHK(c, pcJob.leave());
        return PLZ4HIP_OK;
    default: break;
    }
    if (route == L1Route::L1x) xb = (FxlBlk*)(ws->d + L.offBlk);                 // (the bulk route: behind the group's records)
    for (int g0 = 0; g0 < nb; g0 += per) {
        const int ng = nb - g0 < per ? nb - g0 : per;
        a.blk0 = g0; a.nBlocks = ng;
        a.queue = next_queue(c, s, &e); HIPCHK(c, e);
        if (rider && g0 == 0) launch_rec_verify(s, *rider);                     // (in front of the gate: beside the other stream's launch)
        a.gate = nullptr;                                                       // (only Parse and Duplex wait for and signal the gate)
        if (route == L1Route::Parse || route == L1Route::Duplex) {
            if (sw.noGate) c->gatePending = false;
            else if (int rc = l1_gate(c, s, a, ng)) return rc;
        } else if (route == L1Route::Mid) c->gatePending = false;
        switch (route) {
        case L1Route::Mid:
            if (mxOn && mxl) launch_piece_rounds<KMxl>(s, a, pc, xb, ng, g0 == 0);
            else if (mxOn) launch_piece_rounds<KMx>(s, a, pc, xb, ng, g0 == 0);
            else hipLaunchKernelGGL(hc_mid_kernel(a.hcPfx != nullptr), dim3(grid_for(ng, c->hcWaves)), dim3(64), 0, s, a);
            break;
        case L1Route::Fxl: launch_piece_rounds<KFxl>(s, a, pc, xb, ng, g0 == 0); break;
        case L1Route::Fx:  launch_piece_rounds<KFx>(s, a, pc, xb, ng, g0 == 0); break;
        case L1Route::L1x:                                                       // one wave per block, every block one exact run
            ENC_LAUNCH(k_l1x_parse, ng, c, s, a, xb, c->d_counters);
            break;
        default:
            if (route == L1Route::Duplex && g0 == 0) { if (int rc = launch_duplex(c, s, sw, a, *rider, ng)) return rc; break; }
#if defined(PLZ4_EXP_TABBITS)
            {   // EXPERIMENT: W waves per workgroup, as many workgroups as the device holds
            int W = 10; if (const char* ev = getenv("PLZ4HIP_EXP_W")) W = atoi(ev);
#define EXP_CASE(WW) if (W == WW) { int per = 0; hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, k_l1_parse<WW>, 64 * WW, 0); \
                if (getenv("PLZ4HIP_VERBOSE")) fprintf(stderr, "exp: W=%d workgroups per CU %d\n", WW, per); \
                int wgs = c->cus * per; if (wgs * WW > ng) wgs = (ng + WW - 1) / WW; \
                hipLaunchKernelGGL(k_l1_parse<WW>, dim3(wgs), dim3(64 * WW), 0, s, a); }
            EXP_CASE(4) EXP_CASE(5) EXP_CASE(6) EXP_CASE(8) EXP_CASE(9) EXP_CASE(10) EXP_CASE(12) EXP_CASE(13) EXP_CASE(14) EXP_CASE(16)
#undef EXP_CASE
            }
#else
            ENC_LAUNCH(k_l1_parse, ng, c, s, a);
#endif
        }
        launch_emit(s, a, ng, g0, L.maxChunks, hist ? Emit::Seg : mid ? Emit::Mid : Emit::Back, xb, shape.ctx);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, job.leave());
    HIPCHK(c, pcJob.leave());
    return PLZ4HIP_OK;
}

// The tables both flavours of the few-block decoder start with, at `base`; then DxLayout's record arrays (hashed: and the checksum
// verdicts), link arrays (hist) and the grouped call's word per chain (else null), and DxbLayout's stages for raw blocks above 4 MiB
template <class Layout> void bind_dx_tables(CodecArgs& a, uint8_t* base, const Layout& L)
{
    a.dxT = (uint64_t*)(base + L.offT); a.dxTStride = (int64_t)L.tStride;
    a.dxPtr = (uint32_t*)(base + L.offPtr); a.dxPtrStride = (int64_t)L.pStride;
    a.dxUnits = (DxUnit*)(base + L.offUnits); a.dxMaxSeg = L.maxSeg;
    a.dxInfo = (DxInfo*)(base + L.offInfo);
}
void bind_dx(CodecArgs& a, uint8_t* base, const DxLayout& L, bool records, bool hashed, bool hist)
{
    bind_dx_tables(a, base, L);
    if (records) { a.dxSrcOff = (int64_t*)(base + L.offSrcOff); a.dxLen = (int32_t*)(base + L.offLen); }
    if (hashed) a.dxHashBad = (int32_t*)(base + L.offHashBad);
    if (!hist) return;
    a.dxlFirst = (int32_t*)(base + L.offFirst); a.dxlChain = (int32_t*)(base + L.offChain); a.dxlGood = (int32_t*)(base + L.offGood);
    a.dxlMoved = (uint32_t*)(base + L.offMoved);
}
int32_t* dx_dead(uint8_t* base, const DxLayout& L, bool grouped) { return grouped ? (int32_t*)(base + L.offDead) : nullptr; }
void bind_dxb(CodecArgs& a, uint8_t* base, const DxbLayout& L)
{
    bind_dx_tables(a, base, L);
    a.dxbTG = (uint64_t*)(base + L.offTG); a.dxbTGStride = (int64_t)L.tgStride;
    a.dxbEnt = (DxbEntry*)(base + L.offEnt); a.dxbGroups = L.groups;
    a.dxbRuns = (DxRun*)(base + L.offRuns); a.dxbRunRoom = L.room;
    a.dxbInfo = (DxbInfo*)(base + L.offBi);
}
// DxBig: every block of the call through the dxb stages, the small ones beside the large
void launch_dxb(plz4hip_ctx* c, hipStream_t s, CodecArgs& a, int nb, int64_t maxOut, const DxWant& w, const DxbLayout& L)
{
    bind_dxb(a, c->dx.d, L);
    a.dxbG = w.bigG; a.dxbThr = w.thr; a.dxbRounds = w.rounds;
    const int chunks = (int)((maxOut + 1023) / 1024);
    hipLaunchKernelGGL(k_dx_tables, dim3(L.maxSeg, nb), dim3(64), 0, s, a);
    hipLaunchKernelGGL(k_dxb_compose, dim3(L.groups * 32, nb), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_dxb_hop, dim3(nb), dim3(64), 0, s, a, c->d_counters);
    hipLaunchKernelGGL(k_dxb_units, dim3(L.groups, nb), dim3(64), 0, s, a);
    hipLaunchKernelGGL(k_dx_fill<KDxb>, dim3(L.maxSeg, nb), dim3(64), 0, s, a);
    hipLaunchKernelGGL(k_dxb_runs, dim3(1024, nb), dim3(256), 0, s, a);
    for (int r = 0; r < w.rounds; ++r) { a.dxRound = r; hipLaunchKernelGGL(k_dx_jump<KDxb>, dim3(chunks, nb), dim3(256), 0, s, a); }
    hipLaunchKernelGGL(k_dx_gather<KDxb>, dim3(chunks, nb), dim3(256), 0, s, a, c->d_counters);
}

// Dx, and one group of DxGrouped: the stage train over a's nb blocks (the call, or the group's view of it), L: their layout.  hist:
// the dxl flavour, one pointer space for the blocks; a chain is answered up to its first block that is not plainly good, and the
// one-wave walk goes on from there inside k_dxl_finish.
int launch_dx_train(plz4hip_ctx* c, hipStream_t s, CodecArgs& a, int nb, const DxLayout& L, int64_t maxOut, bool records, int hist)
{
    const int64_t outB = maxOut < kDxMaxOut ? maxOut : kDxMaxOut;
    const int maxSeg = L.maxSeg, chunks = (int)((outB + 1023) / 1024);
    const int nChG = hist == kHistLinked ? a.nChains : 0;
    const bool hashed = records && a.blockChecksum;
    bind_dx(a, c->dx.d, L, records, hashed, hist != kHistNone);
    if (records) {
        hipLaunchKernelGGL(k_dx_rec_prep, dim3((nb + 255) / 256), dim3(256), 0, s, a, (int64_t*)a.dxSrcOff, (int32_t*)a.dxLen);     // (fills them)
        if (hashed) {
            // the block checksums beside the decode, on the ctx's own stream, idle otherwise: one stream more would push the staging
            // slots' streams onto shared hardware queues -- the runtime has four -- and cost the large host calls their overlap:
            // 412 -> 610 ms per 2304 blocks, measured
            c->dxHashStream = c->stream;
            if (!c->evDxFork) HIPCHK(c, hipEventCreateWithFlags(&c->evDxFork, hipEventDisableTiming));
            if (!c->evDxHash) HIPCHK(c, hipEventCreateWithFlags(&c->evDxHash, hipEventDisableTiming));
            HIPCHK(c, hipEventRecord(c->evDxFork, s));
            HIPCHK(c, hipStreamWaitEvent(c->dxHashStream, c->evDxFork, 0));
            hipLaunchKernelGGL(k_dx_rec_hash, dim3(nb), dim3(64), 0, c->dxHashStream, a);
            HIPCHK(c, hipEventRecord(c->evDxHash, c->dxHashStream));
        }
    }
    hipLaunchKernelGGL(k_dx_tables, dim3(maxSeg, nb), dim3(64), 0, s, a);
    hipLaunchKernelGGL(k_dx_stitch, dim3(nb), dim3(64), 0, s, a);
    if (!hist) {
        hipLaunchKernelGGL(k_dx_fill<KDx>, dim3(maxSeg, nb), dim3(64), 0, s, a);
        for (int r = 0; r < DxF::rounds(nb, maxOut); ++r) { a.dxRound = r; hipLaunchKernelGGL(k_dx_jump<KDx>, dim3(chunks, nb), dim3(256), 0, s, a); }
        if (hashed) HIPCHK(c, hipStreamWaitEvent(s, c->evDxHash, 0));
        hipLaunchKernelGGL(k_dx_gather<KDx>, dim3(chunks, nb), dim3(256), 0, s, a, c->d_counters);
    } else {
        // the copy chain of a call (of a group) can be as deep as its output and the history in front of it are long
        const int rounds = DxlF::rounds(nb, maxOut);                           // dx_rounds_for(nb * outB + kDxlHist)
        a.dxlRounds = rounds;
        hipLaunchKernelGGL(k_dxl_link, dim3((nb + 255) / 256), dim3(256), 0, s, a, c->d_counters);
        hipLaunchKernelGGL(k_dx_fill<KDxl>, dim3(maxSeg, nb), dim3(64), 0, s, a);
        hipLaunchKernelGGL(k_dxl_resolve, dim3((int)(L.pStride / 1024), nb), dim3(256), 0, s, a);
        for (int r = 0; r < rounds; ++r) { a.dxRound = r; hipLaunchKernelGGL(k_dx_jump<KDxl>, dim3(chunks, nb), dim3(256), 0, s, a); }
        hipLaunchKernelGGL(k_dx_gather<KDxl>, dim3(chunks, nb), dim3(256), 0, s, a, c->d_counters);
        if (hashed) HIPCHK(c, hipStreamWaitEvent(s, c->evDxHash, 0));
        if (hist == kHistLinked) hipLaunchKernelGGL(k_dxl_finish, dim3(nChG), dim3(64), 0, s, a, c->d_counters);
        else                     hipLaunchKernelGGL(k_dxl_verdict, dim3((nb + 255) / 256), dim3(256), 0, s, a, c->d_counters);
    }
    HIPCHK(c, hipGetLastError());
    return PLZ4HIP_OK;
}

// Enqueue the decode of nb blocks on s (a: everything but the queue filled in) -- raw blocks (LZ4_decompress_safe per block) or, with
// `records`, frame records (FrameReader._read + BlkT.Decompress, blk/frame.go:54-127, blk.go:50-61); the routes: route.h, DESIGN 2.
// maxIn / maxOut: upper bounds of the blocks' compressed and decoded sizes known to the host (the lengths themselves may live on the
// device).  hist -- kHistDict: independent blocks under a.dict; kHistLinked: the chains of a.window / a.chainFirst.  hostFirst: the
// call's chainFirst on the host (nChains + 1 entries; null: one chain).  The stage trains answer plainly valid blocks (1 x 4 MiB in
// about a millisecond of kernels instead of the 66 ms one wavefront needs); the one-wave kernels behind them answer the rest.  The
// grouping constants and their default: profiles/dxl_group_rate.json.
int launch_decode(plz4hip_ctx* c, hipStream_t s, CodecArgs a, int nb, int64_t maxIn, int64_t maxOut, bool records, int hist = kHistNone,
                  const int32_t* hostFirst = nullptr)
{
    hipError_t e;
    MarkOnExit job;
    const DxSwitches sw = read_dx_switches();
    const int nCh = hist == kHistLinked ? a.nChains : 0;
    DxShape shape{nb, maxIn, maxOut, records, hist, a.window != nullptr, a.nChains, 0, hostFirst != nullptr || nCh == 1};
    if (shape.hostFirst) for (int ch = 0; ch < nCh; ++ch) {
        const int n = hostFirst ? hostFirst[ch + 1] - hostFirst[ch] : nb;
        if (n > shape.longest) shape.longest = n;
    }
    const DxWant w = dx_want(shape, sw);
    // groups: [g0, g1) blocks and [ch0, ch1) chains each
    std::vector<DxlGroup> groups;
    int cursor = 0;
    for (int g0 = 0; w.G > 0 && g0 < nb; g0 += w.G) {
        DxlGroup g;
        dxl_group(hostFirst, nCh, nb, w.G, g0, &cursor, &g);
        groups.push_back(g);
        if (g.ch1 - g.ch0 > kDxlGroupChains) { groups.clear(); break; }            // (chains without a block in between, by the thousand)
    }
    const bool grouped = !groups.empty();
    a.dxInfo = nullptr; a.dxSrcOff = nullptr; a.dxLen = nullptr; a.dxHashBad = nullptr; a.dxlGood = nullptr;
    a.dxlDead = nullptr; a.dxlBlk0 = 0; a.dxlGroup = 0; a.dxlGroups = 0;
    // The workspace of either flavour is the ctx's dx buffer, kept until plz4hip_ctx_trim -- DxBig: 8 B per input byte and 4 B per
    // output byte of the call's strides, 8 B x 8192 per group, 16 B per segment and per listed run.  No room: one wave per block.
    // gMax: the blocks a DxLayout is laid out for (the call, or one group); a group's record and link arrays are packed by its own count
    const int gMax = grouped ? w.G : nb;
    const auto layout_for = [&](int n) { return dx_layout(gMax, n, maxIn, maxOut, hist != kHistNone, records, grouped ? nCh : 0); };
    DxbLayout big{};  DxLayout whole{};
    bool granted = false;
    if (w.big || w.dx || grouped) {
        if (w.big) big = dxb_layout(nb, maxIn, maxOut, w.bigG, w.thr); else whole = layout_for(gMax);
        HIPCHK(c, c->dxOrder.wait(s));
        bool refused = false;  HIPCHK(c, c->dx.reserve(w.big ? big.total : whole.total, c->dxOrder, &refused));
        granted = !refused;
        if (granted) job.arm(c->dxOrder, s);
    }
    const DxPlan p = dx_route(shape, w, grouped, granted);
    if (p.route == DxRoute::DxBig) { launch_dxb(c, s, a, nb, maxOut, w, big); HIPCHK(c, hipGetLastError()); }
    else if (p.route == DxRoute::Dx) { if (int rc = launch_dx_train(c, s, a, nb, whole, maxOut, records, hist)) return rc; }
    else if (p.route == DxRoute::DxGrouped) {
        // Each group is the same stage train on s: a block needs only the 64 KiB in front of it, which the finish stage of the group
        // before has laid down in a.window; that, the window's length and one word per chain -- the chain has had a bad block -- are
        // what goes from group to group, in device memory.
        int32_t* const dead = dx_dead(c->dx.d, whole, true);
        HIPCHK(c, hipMemsetAsync(dead, 0, (size_t)nCh * 4, s));
        const int nGroups = (int)groups.size();
        for (int gi = 0; gi < nGroups; ++gi) {
            const DxlGroup& g = groups[gi];
            CodecArgs x = a;                                                        // the group's view of the call
            const int ng = g.g1 - g.g0;
            if (x.recOff) x.recOff += g.g0; else { x.src += (int64_t)g.g0 * x.srcStride; x.srcLen += g.g0; }
            x.dst += (int64_t)g.g0 * x.dstStride; x.result += g.g0; x.status += g.g0; x.nBlocks = ng;
            x.window += (size_t)g.ch0 * 131072; x.windowLen += g.ch0; x.nChains = g.ch1 - g.ch0;
            if (x.chainFirst) x.chainFirst += g.ch0;
            x.dxlDead = dead + g.ch0; x.dxlBlk0 = g.g0; x.dxlGroup = gi; x.dxlGroups = nGroups;
            if (int rc = launch_dx_train(c, s, x, ng, layout_for(ng), maxOut, records, hist)) return rc;
        }
    }
    // the tail: the one-wave kernels answer every block the stages above have not
    a.queue = next_queue(c, s, &e); HIPCHK(c, e);
    const dim3 grid(grid_for(p.tail == DxTail::RecLinked ? a.nChains : nb, c->decWaves));
    switch (p.tail) {
    case DxTail::RecLinked: hipLaunchKernelGGL(k_decode_rec_linked, grid, dim3(64), 0, s, a); break;
    case DxTail::RecDict:   hipLaunchKernelGGL(k_decode_rec_dict, grid, dim3(64), 0, s, a); break;
    case DxTail::RawDict:   hipLaunchKernelGGL(k_decode_raw_dict, grid, dim3(64), 0, s, a); break;
    case DxTail::RecDx:     hipLaunchKernelGGL(k_decode_rec_dx, grid, dim3(64), 0, s, a); break;
    case DxTail::Rec:       launch_rec_verify(s, a); hipLaunchKernelGGL(k_decode_rec, grid, dim3(64), 0, s, a); break;
    case DxTail::Raw:       hipLaunchKernelGGL(k_decode_raw, grid, dim3(64), 0, s, a); break;
    case DxTail::None:      break;
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, job.leave());
    return PLZ4HIP_OK;
}

// What the entry points hand to the launchers.  The record decode of nBlocks records of a frame body ...
CodecArgs rec_decode_args(const void* body, const int64_t* recOff, int nBlocks, int bsz, int blockChecksum, void* dst, int64_t dstStride,
                          int dstCap, int32_t* result, int32_t* status)
{
    CodecArgs a{};
    a.src = (const uint8_t*)body; a.recOff = recOff; a.bsz = bsz;
    a.dst = (uint8_t*)dst; a.dstStride = dstStride; a.dstCapAll = dstCap;
    a.result = result; a.status = status; a.nBlocks = nBlocks; a.blockChecksum = blockChecksum;
    a.dictLen = -1; a.prevTailLen = -1;
    return a;
}
// ... the record encode of srcBytes of plaintext in blocks of bsz, srcStride apart, into a staging area or straight into a frame body
CodecArgs rec_encode_args(const void* src, int64_t srcBytes, int64_t srcStride, int bsz, int blockChecksum, int32_t* recLen, int nBlocks)
{
    CodecArgs a{};
    a.src = (const uint8_t*)src; a.srcStride = srcStride; a.srcBytes = srcBytes; a.bsz = bsz;
    a.result = recLen; a.nBlocks = nBlocks; a.blockChecksum = blockChecksum;
    a.dictLen = -1; a.prevTailLen = -1;
    return a;
}
void into_stage(CodecArgs& a, void* stage, int64_t stride) { a.dst = (uint8_t*)stage; a.dstStride = stride; a.bodyOff = nullptr; a.bodyCap = 0; }
void into_body(CodecArgs& a, void* body, int64_t bodyCap, int64_t* recOff) { a.dst = (uint8_t*)body; a.dstStride = 0; a.bodyOff = recOff; a.bodyCap = bodyCap; }
// ... and a dictionary's level-1 table and, for the HC levels, its context's tables and k_hcx's lists
void dict_args(CodecArgs& a, const plz4hip_dict* dict) { a.dict = dict->d_bytes; a.dictLen = dict->len; a.dictTable = dict->d_table; }
void dict_hc_args(CodecArgs& a, const plz4hip_dict* dict, int level)
{
    const uint8_t* t = dict->d_hc + (level <= 2 ? 0 : (size_t)kHcWorkBytes);
    a.hcDictHash = (const uint32_t*)t; a.hcDictChain = (const uint16_t*)(t + kHcHashEntries * 4);
    a.hcxStart = (const uint32_t*)dict->d_hcx; a.hcxList = (const uint16_t*)(dict->d_hcx + kHcxDictStartBytes);
}

}  // namespace

extern "C" {

int plz4hip_abi_version(void) { return PLZ4HIP_ABI_VERSION; }

#if defined(PLZ4_STATS)
// diagnostics build only: read-and-reset the device counters
int plz4hip_debug_stats(unsigned long long* out24)
{
    unsigned long long zero[24] = {0};
    if (hipDeviceSynchronize() != hipSuccess) return PLZ4HIP_E_DEVICE;
    if (hipMemcpyFromSymbol(out24, HIP_SYMBOL(plz4_stats), sizeof zero) != hipSuccess) return PLZ4HIP_E_DEVICE;
    if (hipMemcpyToSymbol(HIP_SYMBOL(plz4_stats), zero, sizeof zero) != hipSuccess) return PLZ4HIP_E_DEVICE;
    return PLZ4HIP_OK;
}
#endif

int plz4hip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return PLZ4HIP_E_DEVICE;
    return n;
}

int plz4hip_compress_bound(int n) { return ((unsigned)n > 0x7E000000u) ? 0 : n + n / 255 + 16; }

int64_t plz4hip_dev_stage_stride(int bsz) { return (int64_t)round_up((size_t)bsz + 8, 16); }

int plz4hip_ctx_create(int device, plz4hip_ctx** out)
{
    if (!out) return PLZ4HIP_E_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return PLZ4HIP_E_DEVICE;
    plz4hip_ctx* c = new (std::nothrow) plz4hip_ctx();
    if (!c) return PLZ4HIP_E_NOMEM;
    c->device = device;
    DeviceGuard dg(device);
    hipError_t e = dg.err;
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc((void**)&c->d_queues, kQueueSlots * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&c->d_gate, 256);
    // (on the ctx's own stream: a hipMemset would be this process's first use of the NULL stream, which then takes one of the
    // four hardware queues -- the staging slots of the host-buffer calls end up sharing queues and their chunks stop overlapping:
    // 2560 blocks 470 -> 790 ms, found with scripts/host_rate_ab.py)
    if (e == hipSuccess) e = zero_sync(c, c->d_gate, 256);
    if (e == hipSuccess) e = hipMalloc((void**)&c->d_counters, plz4hip_ctx::kCounters * 8);
    if (e == hipSuccess) e = zero_sync(c, c->d_counters, plz4hip_ctx::kCounters * 8);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&c->cus, hipDeviceAttributeMultiprocessorCount, device);
    int encPer = 0, decPer = 0;
    if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&encPer, k_encode_rec<kEncWavesPerWg>, 64 * kEncWavesPerWg, 0);
    if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&decPer, k_decode_rec, 64, 0);
    if (e != hipSuccess) {
        fprintf(stderr, "plz4hip_ctx_create: %s\n", hipGetErrorString(e));
        for (void* p : {(void*)c->d_queues, (void*)c->d_gate, (void*)c->d_counters}) if (p) hipFree(p);
        if (c->stream) hipStreamDestroy(c->stream);
        delete c;
        return PLZ4HIP_E_DEVICE;
    }
    if (encPer < 1) encPer = 1;
    if (decPer < 1) decPer = 1;
    if (encPer > 1) encPer = 1;                      // one 160 KiB workgroup is all of a CU's LDS
    c->encWaves = c->cus * encPer * kEncWavesPerWg;
    c->decWaves = c->cus * decPer;
    *out = c;
    return PLZ4HIP_OK;
}

void plz4hip_ctx_destroy(plz4hip_ctx* c)
{
    if (!c) return;
    DeviceGuard dg(c->device);
    // the jobs still in flight on the callers' streams first: every workspace is freed behind its last job
    for (auto& w : c->owned()) (void)w.buf->release(*w.order);
    for (auto& w : c->owned()) w.order->destroy();
    if (c->stream) { hipStreamSynchronize(c->stream); hipStreamDestroy(c->stream); }
    for (auto& sl : c->slot) {
        if (sl.s) { hipStreamSynchronize(sl.s); hipStreamDestroy(sl.s); }
        if (sl.evData) hipEventDestroy(sl.evData);
        if (sl.evHash) hipEventDestroy(sl.evHash);
        if (sl.h) hipHostFree(sl.h);
        if (sl.d) hipFree(sl.d);
        sl.l1.release();
    }
    for (hipEvent_t ev : {c->evDxFork, c->evDxHash}) if (ev) hipEventDestroy(ev);
    if (c->hashStream) { hipStreamSynchronize(c->hashStream); hipStreamDestroy(c->hashStream); }
    if (c->hcBuildStream) { hipStreamSynchronize(c->hcBuildStream); hipStreamDestroy(c->hcBuildStream); }
    for (void* p : {(void*)c->d_queues, (void*)c->d_gate, (void*)c->d_counters}) if (p) hipFree(p);
    for (hipEvent_t ev : {c->evHcFork, c->evHcHist, c->evHcChain[0], c->evHcChain[1], c->evHcFree[0], c->evHcFree[1]}) if (ev) hipEventDestroy(ev);
    delete c;
}

// Give back what the host-buffer calls and the HC levels keep between calls: pinned host + device staging, HC workspaces.
int plz4hip_ctx_trim(plz4hip_ctx* c)
{
    if (!c) return PLZ4HIP_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    ENTER_DEVICE(c);
    for (auto& sl : c->slot) {
        if (sl.s) HIPCHK(c, hipStreamSynchronize(sl.s));
        if (sl.h) { hipHostFree(sl.h); sl.h = nullptr; sl.hcap = 0; }
        if (sl.d) { hipFree(sl.d); sl.d = nullptr; sl.dcap = 0; }
        sl.l1.release();
    }
    for (auto& w : c->owned()) if (w.trimmed) HIPCHK(c, w.buf->release(*w.order));
    c->hcWaves = 0;
    return PLZ4HIP_OK;
}

int plz4hip_ctx_counters(plz4hip_ctx* c, int64_t* out, int n)
{
    if (!c || n < 0 || (n > 0 && !out)) return PLZ4HIP_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    ENTER_DEVICE(c);
    constexpr int kCounters = plz4hip_ctx::kCounters;
    unsigned long long v[kCounters] = {};
    HIPCHK(c, hipDeviceSynchronize());                                      // (the ctx's work runs on the callers' streams)
    HIPCHK(c, copy_sync(c, v, c->d_counters, sizeof v, hipMemcpyDeviceToHost));
    for (int i = 0; i < n && i < kCounters; ++i) out[i] = (int64_t)v[i];
    return kCounters;
}

const char* plz4hip_last_error(const plz4hip_ctx* c)
{
    if (!c) return "null ctx";
    static thread_local std::string copy;          // the caller's own copy: valid until this thread asks again
    std::lock_guard<std::mutex> g(const_cast<plz4hip_ctx*>(c)->errMu);
    copy = c->err;
    return copy.c_str();
}

int plz4hip_dev_resident_waves(plz4hip_ctx* c, int decode) { return c ? (decode ? c->decWaves : c->encWaves) : PLZ4HIP_E_ARG; }

// ---------------------------------------------------------------------------------------- device-resident API
int plz4hip_dev_compress(plz4hip_ctx* c, int nBlocks, const void* src, int64_t srcStride, const int32_t* srcLen,
                         void* dst, int64_t dstStride, const int32_t* dstCap, int level, int maxLen, int32_t* result, void* stream)
{
    if (!c || nBlocks < 0 || !srcLen || !dstCap || !result) return fail(c, PLZ4HIP_E_ARG, "plz4hip_dev_compress: bad argument");
    if (level != 1 && !is_hc_level(level)) return fail(c, PLZ4HIP_E_UNSUPPORTED, "levels 1..12 are built");
    if (nBlocks == 0) return PLZ4HIP_OK;
    if (is_hc_level(level) && maxLen <= 0) return fail(c, PLZ4HIP_E_ARG, "plz4hip_dev_compress: levels 2..12 need maxLen (the largest srcLen[i]; the lengths are on the device)");
    std::lock_guard<std::mutex> g(c->mu);
    ENTER_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    CodecArgs a{};
    a.src = (const uint8_t*)src; a.srcStride = srcStride; a.srcLen = srcLen;
    a.dst = (uint8_t*)dst; a.dstStride = dstStride; a.dstCap = dstCap;
    a.result = result; a.nBlocks = nBlocks;
    a.dictLen = -1; a.prevTailLen = -1;
    MarkOnExit job;
    if (maxLen > 0) {
        // the kernels index per-block workspaces sized from maxLen: they read lengths that were checked against it
        if ((size_t)nBlocks * 4 > c->lenCopy.bytes) {                     // (grown with room for 256 blocks more)
            // (every reader of the copy was enqueued on its call's stream -- the HC builder's stream joins it -- in front of that
            // call's mark, on whichever way the call ended: the order's own event is enough to free it)
            bool refused = false;  HIPCHK(c, c->lenCopy.reserve((size_t)nBlocks * 4 + 1024, c->lenOrder, &refused));
            if (refused) return fail(c, PLZ4HIP_E_NOMEM, "plz4hip_dev_compress: length copy");
        }
        HIPCHK(c, c->lenOrder.wait(s));                                   // the last job's kernels still read the copy
        job.arm(c->lenOrder, s);                                          // (also after a failed launch: whatever was enqueued reads the copy)
        hipLaunchKernelGGL(k_check_len, dim3((nBlocks + 255) / 256), dim3(256), 0, s, srcLen, maxLen, nBlocks, (int32_t*)c->lenCopy.d, result, 0);
        a.srcLen = (const int32_t*)c->lenCopy.d;
    }
    int rc;
    if (is_hc_level(level)) { a.level = level; rc = launch_hc(c, s, a, nBlocks, maxLen, 1); }
    else rc = launch_l1(c, s, a, nBlocks, maxLen, 1, nullptr);           // (maxLen <= 0: lengths unknown to the host -> fused kernels)
    if (rc == PLZ4HIP_OK && maxLen > 0) {
        hipLaunchKernelGGL(k_check_len, dim3((nBlocks + 255) / 256), dim3(256), 0, s, srcLen, maxLen, nBlocks, (int32_t*)c->lenCopy.d, result, 1);
        HIPCHK(c, hipGetLastError());
    }
    if (rc != PLZ4HIP_OK) return rc;
    HIPCHK(c, job.leave());
    return PLZ4HIP_OK;
}

int plz4hip_dev_decompress(plz4hip_ctx* c, int nBlocks, const void* src, int64_t srcStride, const int32_t* srcLen,
                           void* dst, int64_t dstStride, const int32_t* dstCap, int32_t* result, void* stream)
{
    if (!c || nBlocks < 0 || !srcLen || !dstCap || !result) return fail(c, PLZ4HIP_E_ARG, "plz4hip_dev_decompress: bad argument");
    if (nBlocks == 0) return PLZ4HIP_OK;
    std::lock_guard<std::mutex> g(c->mu);
    ENTER_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    CodecArgs a{};
    a.src = (const uint8_t*)src; a.srcStride = srcStride; a.srcLen = srcLen;
    a.dst = (uint8_t*)dst; a.dstStride = dstStride; a.dstCap = dstCap;
    a.result = result; a.nBlocks = nBlocks;
    a.dictLen = -1; a.prevTailLen = -1;
    // (the lengths live on the device: the strides bound them)
    // (one block: the strides are the bounds where they are above the few-block path's defaults -- a caller with one block above
    // 4 MiB says so by passing strides no smaller than its compressed length and its capacity.  Several blocks: the strides bound
    // them, as ever; an output stride of up to 6 MiB -- 4 MiB blocks with padding -- says nothing of blocks above kDxMaxOut and the
    // call is what it was, a larger one sends it down the big path of launch_decode.)
    const int64_t in1 = srcStride > (int64_t)(6 << 20) ? srcStride : (int64_t)(6 << 20), out1 = dstStride > (int64_t)kDxMaxOut ? dstStride : (int64_t)kDxMaxOut;
    const int64_t outN = dstStride > (int64_t)(6 << 20) || dstStride < (int64_t)kDxMaxOut ? dstStride : (int64_t)kDxMaxOut;
    return launch_decode(c, s, a, nBlocks, nBlocks > 1 ? srcStride : in1, nBlocks > 1 ? outN : out1, false);
}

int plz4hip_dev_encode_records(plz4hip_ctx* c, const void* src, int64_t srcBytes, int bsz, int level,
                               int blockChecksum, void* stage, int32_t* recLen, void* stream)
{
    if (!c || srcBytes < 0 || bsz <= 0 || !stage || !recLen) return fail(c, PLZ4HIP_E_ARG, "plz4hip_dev_encode_records: bad argument");
    if (level != 1 && !is_hc_level(level)) return fail(c, PLZ4HIP_E_UNSUPPORTED, "levels 1..12 are built");
    const int64_t nb64 = (srcBytes + bsz - 1) / bsz;
    if (nb64 > 0x7FFFFFFF) return fail(c, PLZ4HIP_E_ARG, "too many blocks");
    const int nBlocks = (int)nb64;
    if (nBlocks == 0) return PLZ4HIP_OK;
    std::lock_guard<std::mutex> g(c->mu);
    ENTER_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    CodecArgs a = rec_encode_args(src, srcBytes, bsz, bsz, blockChecksum, recLen, nBlocks);
    into_stage(a, stage, plz4hip_dev_stage_stride(bsz));
    if (is_hc_level(level)) {
        a.level = level;
        return launch_hc(c, s, a, nBlocks, bsz, 0);
    }
    return launch_l1(c, s, a, nBlocks, bsz, 0, nullptr);
}

static int move_slices(int maxLen) { const int s = (maxLen + 256 * 16 * 8 - 1) / (256 * 16 * 8); return s < 1 ? 1 : s; }

int plz4hip_dev_compact_records(plz4hip_ctx* c, const void* stage, int64_t stageStride, const int32_t* recLen,
                                int nBlocks, int64_t* recOff, void* body, int64_t bodyCap, void* stream)
{
    if (!c || nBlocks < 0 || !stage || !recLen || !recOff || stageStride <= 0) return fail(c, PLZ4HIP_E_ARG, "plz4hip_dev_compact_records: bad argument");
    if (body && bodyCap <= 0) return fail(c, PLZ4HIP_E_ARG, "plz4hip_dev_compact_records: bodyCap");
    if (nBlocks == 0) return PLZ4HIP_OK;
    std::lock_guard<std::mutex> g(c->mu);
    ENTER_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(64), 0, s, recLen, recOff, nBlocks);
    HIPCHK(c, hipGetLastError());
    if (body) {
        hipLaunchKernelGGL(k_move_records, dim3(nBlocks, move_slices((int)stageStride)), dim3(256), 0, s,
                           (const uint8_t*)stage, (const int64_t*)nullptr, stageStride, recLen, (const int64_t*)recOff, (uint8_t*)body, bodyCap);
        HIPCHK(c, hipGetLastError());
    }
    return PLZ4HIP_OK;
}

int plz4hip_dev_scatter_records(plz4hip_ctx* c, const void* src, const int64_t* srcOff, const int32_t* len,
                                const int64_t* dstOff, int n, int maxLen, void* dst, int64_t dstCap, void* stream)
{
    if (!c || n < 0 || !src || !srcOff || !len || !dstOff || !dst || maxLen < 0 || dstCap < 0) return fail(c, PLZ4HIP_E_ARG, "plz4hip_dev_scatter_records: bad argument");
    if (n == 0) return PLZ4HIP_OK;
    std::lock_guard<std::mutex> g(c->mu);
    ENTER_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_move_records, dim3(n, move_slices(maxLen)), dim3(256), 0, s,
                       (const uint8_t*)src, srcOff, (int64_t)0, len, dstOff, (uint8_t*)dst, dstCap);
    HIPCHK(c, hipGetLastError());
    return PLZ4HIP_OK;
}

int plz4hip_dev_decode_records(plz4hip_ctx* c, const void* body, const int64_t* recOff, int nBlocks,
                               int bsz, int blockChecksum, void* dst, int64_t dstStride, int dstCap,
                               int32_t* result, int32_t* status, void* stream)
{
    if (!c || nBlocks < 0 || !body || !recOff || !dst || !result || !status || bsz <= 0) return fail(c, PLZ4HIP_E_ARG, "plz4hip_dev_decode_records: bad argument");
    if (nBlocks == 0) return PLZ4HIP_OK;
    std::lock_guard<std::mutex> g(c->mu);
    ENTER_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    CodecArgs a = rec_decode_args(body, recOff, nBlocks, bsz, blockChecksum, dst, dstStride, dstCap, result, status);
    return launch_decode(c, s, a, nBlocks, bsz, dstCap, true);
}

int plz4hip_dev_index_body(plz4hip_ctx* c, const void* body, int64_t bodyBytes, int bsz, int blockChecksum,
                           int maxBlocks, int64_t* recOff, plz4hip_body_index* info, void* stream)
{
    if (!c || bodyBytes < 0 || (bodyBytes && !body) || bsz <= 0 || maxBlocks < 0 || maxBlocks > 0x7FFFFFFE || !recOff || !info)
        return fail(c, PLZ4HIP_E_ARG, "plz4hip_dev_index_body: bad argument");
    std::lock_guard<std::mutex> g(c->mu);
    ENTER_DEVICE(c);
    hipLaunchKernelGGL(k_index_body, dim3(1), dim3(64), 0, (hipStream_t)stream, (const uint8_t*)body, bodyBytes, bsz, blockChecksum, maxBlocks,
                       recOff, (BodyIndex*)info);
    HIPCHK(c, hipGetLastError());
    return PLZ4HIP_OK;
}

int plz4hip_dev_index_stream(plz4hip_ctx* c, const void* bytes, int64_t nBytes, int maxFrames, int maxRecs, plz4hip_frame_index* frames,
                             int64_t* recOff, plz4hip_stream_index* info, void* stream)
{
    if (!c || nBytes < 0 || (nBytes && !bytes) || maxFrames < 0 || (maxFrames && !frames) || maxRecs < 0 || maxRecs > 0x7FFFFFFE || !recOff || !info)
        return fail(c, PLZ4HIP_E_ARG, "plz4hip_dev_index_stream: bad argument");
    std::lock_guard<std::mutex> g(c->mu);
    ENTER_DEVICE(c);
    hipLaunchKernelGGL(k_index_stream, dim3(1), dim3(64), 0, (hipStream_t)stream, (const uint8_t*)bytes, nBytes, maxFrames, maxRecs,
                       (FrameIndex*)frames, recOff, (StreamIndex*)info);
    HIPCHK(c, hipGetLastError());
    return PLZ4HIP_OK;
}

// PLZ4HIP_VERIFY_WAVES (read per call): the cap on k_verify_frames' grid, for tests of its stride loop
static int verify_waves_cap(const plz4hip_ctx* c)
{
    int cap = c->decWaves > 0 ? c->decWaves : 1;
    if (const char* v = getenv("PLZ4HIP_VERIFY_WAVES")) { const int w = atoi(v); if (w >= 1 && w <= cap) cap = w; }
    return cap;
}

int plz4hip_dev_verify_frames(plz4hip_ctx* c, const plz4hip_frame_index* frames, const plz4hip_stream_index* info, int maxFrames,
                              const void* dst, int64_t dstStride, int dstCap, const int32_t* result, const int32_t* status, int maxRecs,
                              plz4hip_frame_verdict* verdicts, plz4hip_stream_verdict* sv, void* stream)
{
    if (!c || !info || !sv || !result || !status || maxFrames < 0 || maxRecs < 0 || maxRecs > 0x7FFFFFFE || dstCap < 0 || dstStride < dstCap ||
        (maxFrames && (!frames || !verdicts)) || (maxFrames && maxRecs && !dst))   // (no table or no record: nothing of dst could be read)
        return fail(c, PLZ4HIP_E_ARG, "plz4hip_dev_verify_frames: bad argument");
    std::lock_guard<std::mutex> g(c->mu);
    ENTER_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    if (maxFrames > 0) {
        const int64_t groups = ((int64_t)maxFrames + 15) / 16;
        const int cap = verify_waves_cap(c);
        const int grid = groups < cap ? (int)groups : cap;
        hipLaunchKernelGGL(k_verify_frames, dim3(grid), dim3(64), 0, s, (const FrameIndex*)frames, (const StreamIndex*)info, maxFrames,
                           (const uint8_t*)dst, dstStride, dstCap, result, status, maxRecs, (FrameVerdict*)verdicts);
        HIPCHK(c, hipGetLastError());
    }
    hipLaunchKernelGGL(k_verify_summary, dim3(1), dim3(64), 0, s, (const StreamIndex*)info, maxFrames, (const FrameVerdict*)verdicts, (StreamVerdict*)sv);
    HIPCHK(c, hipGetLastError());
    return PLZ4HIP_OK;
}

// PLZ4HIP_WRITE_WAVES (read per call): the cap on k_frame_edges' grid, for tests of its stride loop
static int write_waves_cap(const plz4hip_ctx* c)
{
    int cap = c->decWaves > 0 ? c->decWaves : 1;
    if (const char* v = getenv("PLZ4HIP_WRITE_WAVES")) { const int w = atoi(v); if (w >= 1 && w <= cap) cap = w; }
    return cap;
}

int plz4hip_dev_write_frames(plz4hip_ctx* c, const plz4hip_frame_opts* o, const void* src, int64_t srcBytes, int64_t srcStride,
                             const void* body, int64_t bodyBytes, const int64_t* recOff, int blocksPerFrame, void* out, int64_t outCap,
                             plz4hip_frame_index* frames, int64_t* outRecOff, plz4hip_write_info* info, void* stream)
{
    constexpr int64_t kMaxBytes = (int64_t)1 << 62;
    if (!c || !o || !recOff || !out || !frames || !outRecOff || !info || srcBytes < 0 || bodyBytes < 0 || bodyBytes > kMaxBytes || outCap < 0 ||
        outCap > kMaxBytes || blocksPerFrame < 0 || o->reserved != 0 || (bodyBytes && !body) || (srcBytes && o->contentChecksum && !src) ||
        (o->linked && blocksPerFrame != 0))
        return fail(c, PLZ4HIP_E_ARG, "plz4hip_dev_write_frames: bad argument");
    const int bsz = o->bsz;
    int id = 0;
    for (int j = 4; j <= 7; ++j) if (bsz == 65536 << 2 * (j - 4)) id = j;
    if (!id) return fail(c, PLZ4HIP_E_ARG, "plz4hip_dev_write_frames: bsz is none of 64 KiB, 256 KiB, 1 MiB, 4 MiB");
    if (srcStride != bsz && srcStride < (int64_t)bsz + 65536) return fail(c, PLZ4HIP_E_ARG, "plz4hip_dev_write_frames: srcStride");
    const int64_t nb64 = srcBytes / bsz + (srcBytes % bsz != 0);
    if (nb64 > 0x7FFFFFFE) return fail(c, PLZ4HIP_E_ARG, "plz4hip_dev_write_frames: too many blocks");
    const FrameWriteGeom g = frame_write_geom(bsz, o->blockChecksum != 0, o->linked != 0, o->contentChecksum != 0, o->contentSize != 0,
                                              o->hasDictId != 0, o->dictId, srcBytes, srcStride, bodyBytes, blocksPerFrame, outCap);
    std::lock_guard<std::mutex> lk(c->mu);
    ENTER_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    const int64_t groups = ((int64_t)g.nFrames + 15) / 16;
    const int cap = write_waves_cap(c);
    hipLaunchKernelGGL(k_frame_edges, dim3(groups < cap ? (int)groups : cap), dim3(64), 0, s, g, (const uint8_t*)src, (const uint8_t*)body, recOff,
                       (uint8_t*)out, (FrameIndex*)frames, outRecOff);
    HIPCHK(c, hipGetLastError());
    if (g.nBlocks > 0) {
        hipLaunchKernelGGL(k_frame_move, dim3(g.nBlocks, move_slices(bsz + 8)), dim3(256), 0, s, g, (const uint8_t*)body, recOff, (uint8_t*)out);
        HIPCHK(c, hipGetLastError());
    }
    hipLaunchKernelGGL(k_frame_summary, dim3(1), dim3(64), 0, s, g, recOff, (const FrameIndex*)frames, (WriteInfo*)info);
    HIPCHK(c, hipGetLastError());
    return PLZ4HIP_OK;
}

// Linked and dictionary records from device memory.  The call's chainFirst goes to the device by value, 64 entries per launch: the
// caller's array is not read after the call returns, and nothing here waits for the device.
namespace {
struct I32x64 { int32_t v[64]; };
__global__ void k_put_i32(int32_t* dst, I32x64 vals, int n) { if ((int)threadIdx.x < n) dst[threadIdx.x] = vals.v[threadIdx.x]; }
}
int plz4hip_dev_decode_records_ex(plz4hip_ctx* c, const void* body, const int64_t* recOff, int nBlocks,
                                  int bsz, int blockChecksum, int linked, const plz4hip_dict* dict,
                                  int nChains, const int32_t* chainFirst, void* windows, int32_t* windowLen,
                                  void* dst, int64_t dstStride, int dstCap, int32_t* result, int32_t* status, void* stream)
{
    if (!c || nBlocks < 0 || !body || !recOff || !dst || !result || !status || bsz <= 0) return fail(c, PLZ4HIP_E_ARG, "plz4hip_dev_decode_records_ex: bad argument");
    if (linked && dict) return fail(c, PLZ4HIP_E_ARG, "plz4hip_dev_decode_records_ex: a linked call takes its dictionary through the window");
    if (!linked && !dict) return fail(c, PLZ4HIP_E_ARG, "plz4hip_dev_decode_records_ex: neither linked nor a dictionary (plz4hip_dev_decode_records)");
    if (linked) {
        if (!windows || !windowLen || nChains < 1) return fail(c, PLZ4HIP_E_ARG, "linked decode needs the window state of its chains");
        if (!chainFirst && nChains != 1) return fail(c, PLZ4HIP_E_ARG, "several chains need chainFirst");
        if (chainFirst) {
            if (chainFirst[0] != 0) return fail(c, PLZ4HIP_E_ARG, "chainFirst[0] must be 0");
            for (int k = 0; k < nChains; ++k) if (chainFirst[k + 1] < chainFirst[k]) return fail(c, PLZ4HIP_E_ARG, "chainFirst must not decrease");
            if (chainFirst[nChains] != nBlocks) return fail(c, PLZ4HIP_E_ARG, "chainFirst must end at nBlocks");
        }
    }
    if (nBlocks == 0) return PLZ4HIP_OK;
    std::lock_guard<std::mutex> g(c->mu);
    ENTER_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    CodecArgs a = rec_decode_args(body, recOff, nBlocks, bsz, blockChecksum, dst, dstStride, dstCap, result, status);
    if (!linked) {
        dict_args(a, dict);
        return launch_decode(c, s, a, nBlocks, bsz, dstCap, true, kHistDict);
    }
    a.linked = 1; a.window = (uint8_t*)windows; a.windowLen = windowLen; a.nChains = nChains;
    MarkOnExit job;
    if (chainFirst) {
        const size_t bytes = (size_t)(nChains + 1) * 4;
        if (bytes > c->chainCopy.bytes) {
            bool refused = false;  HIPCHK(c, c->chainCopy.reserve(bytes + 1024, c->chainOrder, &refused));
            if (refused) return fail(c, PLZ4HIP_E_NOMEM, "plz4hip_dev_decode_records_ex: chain copy");
        }
        HIPCHK(c, c->chainOrder.wait(s));                                   // the last job's kernels still read the copy
        job.arm(c->chainOrder, s);
        for (int k = 0; k <= nChains; k += 64) {
            I32x64 v; const int n = nChains + 1 - k < 64 ? nChains + 1 - k : 64;
            memcpy(v.v, chainFirst + k, (size_t)n * 4);
            hipLaunchKernelGGL(k_put_i32, dim3(1), dim3(64), 0, s, (int32_t*)c->chainCopy.d + k, v, n);
        }
        HIPCHK(c, hipGetLastError());
        a.chainFirst = (const int32_t*)c->chainCopy.d;
    }
    if (int rc = launch_decode(c, s, a, nBlocks, bsz, dstCap, true, kHistLinked, chainFirst)) return rc;
    HIPCHK(c, job.leave());
    return PLZ4HIP_OK;
}

int plz4hip_dev_duplex_records(plz4hip_ctx* c, const void* src, int64_t srcBytes, int bsz, int blockChecksum, void* stage, int32_t* recLen,
                               const void* body, const int64_t* recOff, int nDecBlocks, int decBsz, int decBlockChecksum,
                               void* dst, int64_t dstStride, int dstCap, int32_t* result, int32_t* status, void* stream)
{
    if (!c || srcBytes < 0 || bsz <= 0 || !stage || !recLen) return fail(c, PLZ4HIP_E_ARG, "plz4hip_dev_duplex_records: bad argument (encode side)");
    if (nDecBlocks < 0 || !body || !recOff || !dst || !result || !status || decBsz <= 0) return fail(c, PLZ4HIP_E_ARG, "plz4hip_dev_duplex_records: bad argument (decode side)");
    const int64_t nb64 = (srcBytes + bsz - 1) / bsz;
    if (nb64 > 0x7FFFFFFF) return fail(c, PLZ4HIP_E_ARG, "too many blocks");
    const int nBlocks = (int)nb64;
    if (nBlocks == 0 && nDecBlocks == 0) return PLZ4HIP_OK;
    std::lock_guard<std::mutex> g(c->mu);
    ENTER_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    CodecArgs d = rec_decode_args(body, recOff, nDecBlocks, decBsz, decBlockChecksum, dst, dstStride, dstCap, result, status);
    if (nDecBlocks > 0) { hipError_t e; d.queue = next_queue(c, s, &e); HIPCHK(c, e); }
    if (nBlocks == 0) {
        launch_rec_verify(s, d);
        hipLaunchKernelGGL(k_decode_rec, dim3(grid_for(nDecBlocks, c->decWaves)), dim3(64), 0, s, d);
        HIPCHK(c, hipGetLastError());
        return PLZ4HIP_OK;
    }
    CodecArgs a = rec_encode_args(src, srcBytes, bsz, bsz, blockChecksum, recLen, nBlocks);
    into_stage(a, stage, plz4hip_dev_stage_stride(bsz));
    return launch_l1(c, s, a, nBlocks, bsz, 0, nullptr, nullptr, nDecBlocks > 0 ? &d : nullptr);
}

// plz4hip_dev_encode_records + plz4hip_dev_compact_records in one: the records go straight to their place in the frame body
// (the emit stage knows every record's length before it writes a byte: k_l1_scan, then a scan over the blocks).  No staging
// area, no second pass over the records.  Level 1 and 2 (the staged call); recOff[nBlocks] > bodyCap: the records beyond the
// room were not written.
static int encode_body_args(plz4hip_ctx* c, CodecArgs& a, const void* src, int64_t srcBytes, int bsz, int blockChecksum,
                            void* body, int64_t bodyCap, int64_t* recOff, int32_t* recLen, int* nBlocksOut, const char* who)
{
    if (!c || srcBytes < 0 || bsz <= 0 || bsz > kSeqMaxBlock || !body || bodyCap <= 0 || !recOff || !recLen) return fail(c, PLZ4HIP_E_ARG, who);
    const int64_t nb64 = (srcBytes + bsz - 1) / bsz;
    if (nb64 > 0x7FFFFFFF) return fail(c, PLZ4HIP_E_ARG, "too many blocks");
    *nBlocksOut = (int)nb64;
    a = rec_encode_args(src, srcBytes, bsz, bsz, blockChecksum, recLen, *nBlocksOut);
    into_body(a, body, bodyCap, recOff);
    return PLZ4HIP_OK;
}
int plz4hip_dev_encode_body(plz4hip_ctx* c, const void* src, int64_t srcBytes, int bsz, int level, int blockChecksum,
                            void* body, int64_t bodyCap, int64_t* recOff, int32_t* recLen, void* stream)
{
    if (level != 1 && level != 2) return fail(c, PLZ4HIP_E_UNSUPPORTED, "plz4hip_dev_encode_body: levels 1 and 2 (the others: plz4hip_dev_encode_records + plz4hip_dev_compact_records)");
    CodecArgs a{}; int nBlocks = 0;
    if (int rc = encode_body_args(c, a, src, srcBytes, bsz, blockChecksum, body, bodyCap, recOff, recLen, &nBlocks, "plz4hip_dev_encode_body: bad argument")) return rc;
    std::lock_guard<std::mutex> g(c->mu);
    ENTER_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    if (nBlocks == 0) { HIPCHK(c, hipMemsetAsync(recOff, 0, sizeof(int64_t), s)); return PLZ4HIP_OK; }
    if (level == 2) { a.level = 2; return launch_hc(c, s, a, nBlocks, bsz, 0); }
    return launch_l1(c, s, a, nBlocks, bsz, 0, nullptr);
}
// ... and with the record decode of another batch in the same launch (plz4hip_dev_duplex_records' counterpart)
int plz4hip_dev_duplex_body(plz4hip_ctx* c, const void* src, int64_t srcBytes, int bsz, int blockChecksum,
                            void* body, int64_t bodyCap, int64_t* recOff, int32_t* recLen,
                            const void* decBody, const int64_t* decRecOff, int nDecBlocks, int decBsz, int decBlockChecksum,
                            void* dst, int64_t dstStride, int dstCap, int32_t* result, int32_t* status, void* stream)
{
    CodecArgs a{}; int nBlocks = 0;
    if (int rc = encode_body_args(c, a, src, srcBytes, bsz, blockChecksum, body, bodyCap, recOff, recLen, &nBlocks, "plz4hip_dev_duplex_body: bad argument (encode side)")) return rc;
    if (nDecBlocks < 0 || (nDecBlocks > 0 && (!decBody || !decRecOff || !dst || !result || !status || decBsz <= 0))) return fail(c, PLZ4HIP_E_ARG, "plz4hip_dev_duplex_body: bad argument (decode side)");
    if (nBlocks == 0 && nDecBlocks == 0) return PLZ4HIP_OK;
    std::lock_guard<std::mutex> g(c->mu);
    ENTER_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    CodecArgs d = rec_decode_args(decBody, decRecOff, nDecBlocks, decBsz, decBlockChecksum, dst, dstStride, dstCap, result, status);
    if (nDecBlocks > 0) { hipError_t e; d.queue = next_queue(c, s, &e); HIPCHK(c, e); }
    if (nBlocks == 0) {
        HIPCHK(c, hipMemsetAsync(recOff, 0, sizeof(int64_t), s));
        launch_rec_verify(s, d);
        hipLaunchKernelGGL(k_decode_rec, dim3(grid_for(nDecBlocks, c->decWaves)), dim3(64), 0, s, d);
        HIPCHK(c, hipGetLastError());
        return PLZ4HIP_OK;
    }
    return launch_l1(c, s, a, nBlocks, bsz, 0, nullptr, nullptr, nDecBlocks > 0 ? &d : nullptr);
}

// ---- records of blocks with history outside the block (linked blocks, a dictionary) from device-resident plaintext:
// plz4hip_encode_records_ex for a producer whose plaintext is in device memory.  The kernels' one layout rule -- the external segment
// lies immediately in front of the block -- holds by itself for a linked frame over contiguous plaintext (srcStride == bsz: block i's
// segment is the tail of block i - 1); elsewhere the caller leaves 64 KiB of scratch in front of the block and the kernels lay the
// segment there (block 0 of a contiguous call under a dictionary / after a prevTail that does not end at src; every block of a
// gapped call).
static int encode_ex_args(plz4hip_ctx* c, CodecArgs& a, const void* src, int64_t srcBytes, int64_t srcStride, int bsz, int level,
                          int blockChecksum, int linked, const plz4hip_dict* dict, const void* prevTail, int prevTailLen,
                          int32_t* recLen, int* nBlocksOut, const char* who)
{
    if (!c || srcBytes < 0 || (srcBytes > 0 && !src) || bsz <= 0 || !recLen) return fail(c, PLZ4HIP_E_ARG, who);
    if (!linked && !dict) return fail(c, PLZ4HIP_E_ARG, "independent blocks without a dictionary: plz4hip_dev_encode_records / plz4hip_dev_encode_body");
    if (srcStride != (int64_t)bsz && srcStride < (int64_t)bsz + 65536) return fail(c, PLZ4HIP_E_ARG, "srcStride: bsz (contiguous) or at least bsz + 65536 (64 KiB of scratch in front of every block)");
    if (!linked && srcStride == (int64_t)bsz) return fail(c, PLZ4HIP_E_ARG, "independent blocks under a dictionary need 64 KiB of scratch in front of every block (srcStride >= bsz + 65536)");
    if (prevTailLen > 65536 || (prevTailLen > 0 && !prevTail)) return fail(c, PLZ4HIP_E_ARG, "prevTail: a device pointer and at most 64 KiB");
    if (linked && prevTailLen > 0) {
        // laid at [src - prevTailLen, src) unless it is those bytes already: a tail that overlaps that range otherwise would be copied over itself
        const uintptr_t t0 = (uintptr_t)prevTail, t1 = t0 + (uintptr_t)prevTailLen, s1 = (uintptr_t)src, s0 = s1 - (uintptr_t)prevTailLen;
        if (t1 != s1 && t0 < s1 && t1 > s0) return fail(c, PLZ4HIP_E_ARG, "prevTail must end exactly at src or lie outside the bytes it is laid at, [src - prevTailLen, src)");
    }
    const int64_t nb64 = (srcBytes + bsz - 1) / bsz;
    if (nb64 > 0x7FFFFFFF) return fail(c, PLZ4HIP_E_ARG, "too many blocks");
    *nBlocksOut = (int)nb64;
    a = rec_encode_args(src, srcBytes, srcStride, bsz, blockChecksum, recLen, *nBlocksOut);
    a.linked = linked ? 1 : 0;
    if (dict) dict_args(a, dict);
    if (linked && prevTailLen >= 0) { a.prevTail = (const uint8_t*)prevTail; a.prevTailLen = prevTailLen; }
    if (is_hc_level(level)) {
        a.level = level; a.hcEx = 1;
        if (dict) dict_hc_args(a, dict, level);
    }
    return PLZ4HIP_OK;
}

int plz4hip_dev_encode_records_ex(plz4hip_ctx* c, const void* src, int64_t srcBytes, int64_t srcStride, int bsz, int level,
                                  int blockChecksum, int linked, const plz4hip_dict* dict, const void* prevTail, int prevTailLen,
                                  void* stage, int32_t* recLen, void* stream)
{
    if (level != 1 && !is_hc_level(level)) return fail(c, PLZ4HIP_E_UNSUPPORTED, "levels 1..12 are built");
    CodecArgs a{}; int nBlocks = 0;
    if (int rc = encode_ex_args(c, a, src, srcBytes, srcStride, bsz, level, blockChecksum, linked, dict, prevTail, prevTailLen, recLen, &nBlocks,
                                "plz4hip_dev_encode_records_ex: bad argument")) return rc;
    if (!stage) return fail(c, PLZ4HIP_E_ARG, "plz4hip_dev_encode_records_ex: bad argument");
    if (nBlocks == 0) return PLZ4HIP_OK;
    std::lock_guard<std::mutex> g(c->mu);
    ENTER_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    into_stage(a, stage, plz4hip_dev_stage_stride(bsz));
    if (is_hc_level(level)) return launch_hc(c, s, a, nBlocks, bsz, 0);
    return launch_l1(c, s, a, nBlocks, bsz, 0, nullptr, nullptr, nullptr, true, true);
}

int plz4hip_dev_encode_body_ex(plz4hip_ctx* c, const void* src, int64_t srcBytes, int64_t srcStride, int bsz, int level,
                               int blockChecksum, int linked, const plz4hip_dict* dict, const void* prevTail, int prevTailLen,
                               void* body, int64_t bodyCap, int64_t* recOff, int32_t* recLen, void* stream)
{
    if (level != 1 && level != 2) return fail(c, PLZ4HIP_E_UNSUPPORTED, "plz4hip_dev_encode_body_ex: levels 1 and 2 (the others: plz4hip_dev_encode_records_ex + plz4hip_dev_compact_records)");
    CodecArgs a{}; int nBlocks = 0;
    if (int rc = encode_ex_args(c, a, src, srcBytes, srcStride, bsz, level, blockChecksum, linked, dict, prevTail, prevTailLen, recLen, &nBlocks,
                                "plz4hip_dev_encode_body_ex: bad argument")) return rc;
    if (bsz > kSeqMaxBlock || !body || bodyCap <= 0 || !recOff) return fail(c, PLZ4HIP_E_ARG, "plz4hip_dev_encode_body_ex: bad argument");
    std::lock_guard<std::mutex> g(c->mu);
    ENTER_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    if (nBlocks == 0) { HIPCHK(c, hipMemsetAsync(recOff, 0, sizeof(int64_t), s)); return PLZ4HIP_OK; }
    into_body(a, body, bodyCap, recOff);
    if (level == 2) {
        // (a block <= 4 KiB under a dictionary context is written by the one-thread parser behind the emit stage, into a staged record)
        const int lastLen = (int)(srcBytes - (int64_t)(nBlocks - 1) * bsz);
        // (hc_prime: under ANY attached dictionary, whatever its length)
        const bool ctxSmall = dict && (linked ? (a.prevTailLen < 0 && (nBlocks == 1 ? lastLen : bsz) <= kCtxMaxBlock) : (lastLen <= kCtxMaxBlock || bsz <= kCtxMaxBlock));
        if (ctxSmall) return fail(c, PLZ4HIP_E_UNSUPPORTED, "plz4hip_dev_encode_body_ex: level 2 with a block <= 4 KiB under a dictionary context (plz4hip_dev_encode_records_ex + plz4hip_dev_compact_records)");
        return launch_hc(c, s, a, nBlocks, bsz, 0);
    }
    const L1Shape shape{nBlocks, bsz, false, false, false, true, true, true, a.dictLen >= 8};
    const L1Switches sw = read_l1_switches();                                   // (once per call: launch_l1 is handed these)
    if (!l1_want(shape, sw).staged) {
        // the one-kernel encoder writes staged records: a staging area of the ctx's, then the compaction of plz4hip_dev_compact_records
        const int64_t stride = plz4hip_dev_stage_stride(bsz);
        HIPCHK(c, c->xstageOrder.wait(s));
        bool refused = false;  HIPCHK(c, c->xstage.reserve((size_t)nBlocks * (size_t)stride, c->xstageOrder, &refused));
        if (refused) return fail(c, PLZ4HIP_E_NOMEM, "plz4hip_dev_encode_body_ex: the one-kernel encoder's staging area");
        MarkOnExit job;  job.arm(c->xstageOrder, s);
        into_stage(a, c->xstage.d, stride);
        if (int rc = launch_l1(c, s, a, nBlocks, bsz, 0, nullptr, nullptr, nullptr, true, true, &sw)) return rc;
        hipLaunchKernelGGL(k_scan, dim3(1), dim3(64), 0, s, (const int32_t*)recLen, recOff, nBlocks);
        hipLaunchKernelGGL(k_move_records, dim3(nBlocks, move_slices((int)stride)), dim3(256), 0, s,
                           (const uint8_t*)c->xstage.d, (const int64_t*)nullptr, stride, (const int32_t*)recLen, (const int64_t*)recOff, (uint8_t*)body, bodyCap);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, job.leave());
        return PLZ4HIP_OK;
    }
    return launch_l1(c, s, a, nBlocks, bsz, 0, nullptr, nullptr, nullptr, true, true, &sw);
}

// ---------------------------------------------------------------------------------------- host-buffer API
// The layout of one chunk in a slot, the same in the pinned host buffer and in the device buffer: Staging (ws_layout.h)
struct DictJob {                       // optional dictionary / linked parameters of a host call
    const plz4hip_dict* dict = nullptr;
    int   linked = 0;
    const void* prevTail = nullptr; int prevTailLen = -1;
    uint8_t* window = nullptr; int* windowLen = nullptr;      // host buffers (64 KiB, one length) per linked decode chain
    int   nChains = 1; const int32_t* chainFirst = nullptr;   // several chains in one call (plz4hip_decode_records_chains)
    bool  any = false;
    int   level = 1;
};

// Host-buffer entry points.  A call is cut into chunks of at most kChunkBytes (6 GiB; PLZ4HIP_HOST_CHUNK_MB) of staging; up to kSlots chunks are in flight,
// each on its own stream: while the GPU works on one, the host threads fill the next and empty the previous, H2D / kernel /
// D2H of different chunks overlap, and kernels of several chunks share the GPU.  Only the bytes produced travel back
// (outputs are compacted on the device first).  A linked chain (block i needs block i-1) stays one chunk.
static int host_codec(plz4hip_ctx* c, int mode /*0 enc raw,1 dec raw,2 enc rec,3 dec rec,4 xxh*/, int nBlocks,
                      const void* const* src, const int32_t* srcLen, void* const* dst, const int32_t* dstCap,
                      int bsz, int blockChecksum, int32_t* result, int32_t* status, const DictJob* dj = nullptr)
{
    if (nBlocks == 0) return PLZ4HIP_OK;
    int maxIn = 0, maxOut = 0;
    for (int i = 0; i < nBlocks; ++i) {
        if (srcLen[i] < 0 || (srcLen[i] > 0 && !src[i])) return fail(c, PLZ4HIP_E_ARG, "bad source block");
        if (srcLen[i] > maxIn) maxIn = srcLen[i];
        const int oc = (mode == 0 || mode == 1) ? dstCap[i] : (mode == 4 ? 4 : bsz + 8);
        if (oc < 0) return fail(c, PLZ4HIP_E_ARG, "negative capacity");
        if (oc > maxOut) maxOut = oc;
    }
    std::lock_guard<std::mutex> g(c->mu);
    ENTER_DEVICE(c);
    const bool dictMode = dj && dj->any;
    const bool hcMode = dj && is_hc_level(dj->level);
    plz4hip_xxh32_stream* const hash = (mode == 2 || (mode == 3 && !(dj && dj->nChains > 1))) ? c->contentHash : nullptr;
    if (hash && !c->hashStream) HIPCHK(c, hipStreamCreateWithFlags(&c->hashStream, hipStreamNonBlocking));
    // a linked DECODE is one serial chain (block i needs block i-1's output): one chunk.  A linked ENCODE needs only the
    // previous block's source tail, which the caller's buffers hold: it is cut into chunks like any other call, the first
    // block of a later chunk getting the tail of the block before it as its prevTail.
    const bool chained = dictMode && dj->linked && mode == 3;
    if (dictMode && dj->prevTail && dj->prevTailLen > 65536) return fail(c, PLZ4HIP_E_ARG, "prevTail longer than 64 KiB");

    size_t kChunkBytes = (size_t)4 << 30;      // x kSlots in flight (smaller chunks starve the encoder's wave slots); pinned host + device staging stay allocated until plz4hip_ctx_trim / destroy
    // the HC levels run one chunk at a time (below) and live on the number of blocks in flight: one chunk of three times the
    // size (4 MiB blocks: 1024 instead of 341 per chunk) for the same staging memory
    if (hcMode) kChunkBytes *= plz4hip_ctx::kSlots;
    if (const char* v = getenv("PLZ4HIP_HOST_CHUNK_MB")) { const long mb = atol(v); if (mb > 0) kChunkBytes = (size_t)mb << 20; }   // tests: force many chunks
    const size_t gap = (dictMode && (mode == 0 || mode == 2)) ? 65536 : 0;     // encoders with a dictionary / linked blocks: room for the external segment
    int cb = nBlocks;
    {
        const Staging one = staging_layout(1, maxIn, maxOut, gap, false, 1);
        const size_t per = (size_t)one.inStride + 2 * (size_t)one.outStride;
        if (!chained && per * (size_t)nBlocks > kChunkBytes) { cb = (int)(kChunkBytes / per); if (cb < 1) cb = 1; }
    }
    const int nChunks = (nBlocks + cb - 1) / cb;
    // HC kernels index one shared workspace by workgroup: never two of them at once
    const int nSlots = hcMode ? 1 : (nChunks < plz4hip_ctx::kSlots ? nChunks : plz4hip_ctx::kSlots);
    const int    nCh = (dictMode && dj->window) ? dj->nChains : 1;
    const Staging st = staging_layout(cb, maxIn, maxOut, gap, dictMode, nCh);
    for (int i = 0; i < nSlots; ++i) if (int rc = ensure_slot(c, i, st.total, st.total)) return rc;

    auto submit = [&](int k) -> int {
        plz4hip_ctx::HostSlot& sl = c->slot[k % nSlots];
        const int b0 = k * cb, nb = (nBlocks - b0 < cb) ? nBlocks - b0 : cb;
        hipStream_t s = sl.s;
        int32_t* hA = (int32_t*)(sl.h + st.offA);
        int32_t* hB = (int32_t*)(sl.h + st.offB);
        size_t inBytes = 0;
        for (int i = 0; i < nb; ++i) { hA[i] = srcLen[b0 + i]; hB[i] = (mode == 0 || mode == 1) ? dstCap[b0 + i] : 0; inBytes += (size_t)srcLen[b0 + i]; }
        parallel_blocks(nb, inBytes, [&](int i) {
            if (srcLen[b0 + i]) memcpy(sl.h + st.offIn + st.gap + (size_t)i * st.inStride, src[b0 + i], (size_t)srcLen[b0 + i]);
        });
        HIPCHK(c, hipMemcpyAsync(sl.d, sl.h, st.offRes, hipMemcpyHostToDevice, s));                                   // srcLen, dstCap
        HIPCHK(c, hipMemcpyAsync(sl.d + st.offIn, sl.h + st.offIn, (size_t)nb * st.inStride, hipMemcpyHostToDevice, s));
        if (hash && mode == 2) {
            if (!sl.evData) HIPCHK(c, hipEventCreateWithFlags(&sl.evData, hipEventDisableTiming));
            HIPCHK(c, hipEventRecord(sl.evData, s));
        }
        hipError_t e; uint32_t* q = next_queue(c, s, &e); HIPCHK(c, e);
        CodecArgs a{};
        a.src = sl.d + st.offIn + st.gap; a.srcStride = st.inStride; a.srcLen = (const int32_t*)(sl.d + st.offA);
        a.dst = sl.d + st.offOut; a.dstStride = st.outStride; a.dstCap = (const int32_t*)(sl.d + st.offB);
        a.result = (int32_t*)(sl.d + st.offRes); a.status = (int32_t*)(sl.d + st.offSt);
        a.queue = q; a.nBlocks = nb; a.bsz = bsz; a.blockChecksum = blockChecksum; a.dstCapAll = bsz + 8;
        a.dictLen = -1; a.prevTailLen = -1;
        if (hcMode) a.level = dj->level;
        if (dictMode) {
            if (dj->dict) dict_args(a, dj->dict);
            if (hcMode) { a.hcEx = 1; if (dj->dict) dict_hc_args(a, dj->dict, dj->level); }
            a.linked = dj->linked;
            const void* pt = dj->prevTail; int ptLen = (dj->prevTail && dj->prevTailLen >= 0) ? dj->prevTailLen : -1;
            if (dj->linked && b0 > 0) {                                   // a later chunk of a linked encode
                const int pl = srcLen[b0 - 1]; ptLen = tail_len(pl);
                pt = (const uint8_t*)src[b0 - 1] + (pl - ptLen);
            }
            if (ptLen >= 0) {
                if (ptLen) memcpy(sl.h + st.offExtra, pt, (size_t)ptLen);
                HIPCHK(c, hipMemcpyAsync(sl.d + st.offExtra, sl.h + st.offExtra, (size_t)ptLen + 16, hipMemcpyHostToDevice, s));
                a.prevTail = sl.d + st.offExtra; a.prevTailLen = ptLen;
            }
            if (dj->window) {
                for (int ch = 0; ch < nCh; ++ch) memcpy(sl.h + st.offWin + (size_t)ch * 131072, dj->window + (size_t)ch * 65536, 65536);
                memcpy(sl.h + st.offWinLen, dj->windowLen, (size_t)nCh * sizeof(int));
                if (dj->chainFirst) memcpy(sl.h + st.offFirst, dj->chainFirst, (size_t)(nCh + 1) * sizeof(int32_t));
                HIPCHK(c, hipMemcpyAsync(sl.d + st.offWin, sl.h + st.offWin, st.winBytes, hipMemcpyHostToDevice, s));
                a.window = sl.d + st.offWin; a.windowLen = (int*)(sl.d + st.offWinLen);
                a.nChains = nCh; a.chainFirst = dj->chainFirst ? (const int32_t*)(sl.d + st.offFirst) : nullptr;
            }
        }
        switch (mode) {
        case 0: if (hcMode) { if (int rc = launch_hc(c, s, a, nb, maxIn, 1)) return rc; }
                else { if (int rc = launch_l1(c, s, a, nb, maxIn, 1, &sl.l1, nullptr, nullptr, dictMode)) return rc; } break;
        case 1: if (int rc = launch_decode(c, s, a, nb, maxIn, maxOut, false, dictMode ? kHistDict : kHistNone)) return rc;
                break;
        case 2: a.dstCap = nullptr;
                if (hcMode) { if (int rc = launch_hc(c, s, a, nb, maxIn, 0)) return rc; }
                else { if (int rc = launch_l1(c, s, a, nb, maxIn, 0, &sl.l1, nullptr, nullptr, dictMode)) return rc; } break;
        case 3: a.dstCap = nullptr;
                if (int rc = launch_decode(c, s, a, nb, bsz, bsz + 8, true, !dictMode ? kHistNone : (dj->linked ? kHistLinked : kHistDict),
                                           dictMode ? dj->chainFirst : nullptr)) return rc;    // (a linked decode is one chunk: the call's chains)
                break;
        case 4: hipLaunchKernelGGL(k_xxh32, dim3(grid_for(nb, c->decWaves)), dim3(64), 0, s,
                                   (const uint8_t*)a.src, a.srcStride, a.srcLen, (uint32_t*)a.result, nb, q); break;
        }
        HIPCHK(c, hipGetLastError());
        if (hash && (mode == 2 || mode == 3)) {
            // The content checksum of this chunk's plaintext, in block order, on the ctx's hash stream: it starts once the
            // chunk's plaintext is on the device (encode: the copy in; decode: the decode kernel) and runs beside whatever the
            // slot's stream does next; chunks follow each other on the hash stream.
            if (!sl.evData) HIPCHK(c, hipEventCreateWithFlags(&sl.evData, hipEventDisableTiming));
            if (!sl.evHash) HIPCHK(c, hipEventCreateWithFlags(&sl.evHash, hipEventDisableTiming));
            if (mode == 3) HIPCHK(c, hipEventRecord(sl.evData, s));             // (encode: recorded right behind the copy in)
            HIPCHK(c, hipStreamWaitEvent(c->hashStream, sl.evData, 0));
            if (mode == 2) hipLaunchKernelGGL(k_xxh32_stream, dim3(1), dim3(64), 0, c->hashStream, hash->d_state, (const uint8_t*)a.src, a.srcStride, a.srcLen, nb, (int64_t)0, 0);
            else           hipLaunchKernelGGL(k_xxh32_stream, dim3(1), dim3(64), 0, c->hashStream, hash->d_state, (const uint8_t*)a.dst, a.dstStride, (const int32_t*)a.result, nb, (int64_t)0, 0);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipEventRecord(sl.evHash, c->hashStream));
            HIPCHK(c, hipEventRecord(hash->done, c->hashStream));
            sl.hashBusy = true;
        }
        if (mode != 4) {                                       // pack the outputs: sizes -> offsets -> back to back
            int32_t* dLen = (int32_t*)(sl.d + st.offLen); int64_t* dOff = (int64_t*)(sl.d + st.offOff);
            hipLaunchKernelGGL(k_out_len, dim3((nb + 255) / 256), dim3(256), 0, s, (const int32_t*)a.result, dLen, nb);
            hipLaunchKernelGGL(k_scan, dim3(1), dim3(64), 0, s, (const int32_t*)dLen, dOff, nb);
            hipLaunchKernelGGL(k_move_records, dim3(nb, move_slices((int)st.outStride)), dim3(256), 0, s,
                               (const uint8_t*)(sl.d + st.offOut), (const int64_t*)nullptr, st.outStride, (const int32_t*)dLen,
                               (const int64_t*)dOff, sl.d + st.offPack, (int64_t)nb * st.outStride);
            HIPCHK(c, hipGetLastError());
        }
        // results, status, sizes and offsets now; the packed bytes once their total is known (retire)
        HIPCHK(c, hipMemcpyAsync(sl.h + st.offRes, sl.d + st.offRes, st.offIn - st.offRes, hipMemcpyDeviceToHost, s));
        if (dictMode && dj->window)
            HIPCHK(c, hipMemcpyAsync(sl.h + st.offWin, sl.d + st.offWin, st.offFirst - st.offWin, hipMemcpyDeviceToHost, s));
        return PLZ4HIP_OK;
    };
    auto retire = [&](int k) -> int {
        plz4hip_ctx::HostSlot& sl = c->slot[k % nSlots];
        const int b0 = k * cb, nb = (nBlocks - b0 < cb) ? nBlocks - b0 : cb;
        HIPCHK(c, hipStreamSynchronize(sl.s));
        if (sl.hashBusy) { HIPCHK(c, hipEventSynchronize(sl.evHash)); sl.hashBusy = false; }     // the slot's buffers are free again
        const int32_t* hRes = (const int32_t*)(sl.h + st.offRes);
        const int32_t* hSt  = (const int32_t*)(sl.h + st.offSt);
        const int32_t* hLen = (const int32_t*)(sl.h + st.offLen);
        const int64_t* hOff = (const int64_t*)(sl.h + st.offOff);
        if (mode != 4 && hOff[nb] > 0) {
            HIPCHK(c, hipMemcpyAsync(sl.h + st.offOut, sl.d + st.offPack, (size_t)hOff[nb], hipMemcpyDeviceToHost, sl.s));
            HIPCHK(c, hipStreamSynchronize(sl.s));
        }
        if (dictMode && dj->window) {
            for (int ch = 0; ch < nCh; ++ch) memcpy(dj->window + (size_t)ch * 65536, sl.h + st.offWin + (size_t)ch * 131072, 65536);
            memcpy(dj->windowLen, sl.h + st.offWinLen, (size_t)nCh * sizeof(int));
        }
        for (int i = 0; i < nb; ++i) { result[b0 + i] = hRes[i]; if (status) status[b0 + i] = hSt[i]; }
        if (mode != 4)
            parallel_blocks(nb, (size_t)hOff[nb], [&](int i) {
                if (hLen[i] > 0 && dst[b0 + i]) memcpy(dst[b0 + i], sl.h + st.offOut + (size_t)hOff[i], (size_t)hLen[i]);
            });
        return PLZ4HIP_OK;
    };
    int rc = PLZ4HIP_OK;
    int retired = 0;
    for (int k = 0; k < nChunks && rc == PLZ4HIP_OK; ++k) {
        if (k >= nSlots) { rc = retire(retired++); if (rc) break; }       // its slot is the one chunk k needs
        rc = submit(k);
    }
    for (; retired < nChunks && rc == PLZ4HIP_OK; ++retired) rc = retire(retired);
    if (rc != PLZ4HIP_OK) for (int i = 0; i < nSlots; ++i) if (c->slot[i].s) hipStreamSynchronize(c->slot[i].s);   // nothing left in flight
    if (rc == PLZ4HIP_OK && hcMode && c->h12.d && dj->level >= 12) {
        // the level-12 search kernel bounds its spins and raises this flag if it ever gives up (never seen): an engine failure,
        // not a result
        int32_t flag = 0;
        HIPCHK(c, copy_sync(c, &flag, c->h12.d + c->h12ErrOff, 4, hipMemcpyDeviceToHost));
        if (flag) return fail(c, PLZ4HIP_E_DEVICE, "level-12 search kernel gave up (spin guard)");
    }
    return rc;
}

int plz4hip_compress_batch(plz4hip_ctx* c, int nBlocks, const void* const* src, const int32_t* srcLen,
                           void* const* dst, const int32_t* dstCap, int level, int32_t* result)
{
    if (!c || nBlocks < 0 || (nBlocks && (!src || !srcLen || !dst || !dstCap || !result))) return fail(c, PLZ4HIP_E_ARG, "plz4hip_compress_batch: bad argument");
    if (is_hc_level(level)) { DictJob j; j.level = level; return host_codec(c, 0, nBlocks, src, srcLen, dst, dstCap, 0, 0, result, nullptr, &j); }
    if (level != 1) return fail(c, PLZ4HIP_E_UNSUPPORTED, "levels 1..12 are built");
    return host_codec(c, 0, nBlocks, src, srcLen, dst, dstCap, 0, 0, result, nullptr);
}

int plz4hip_decompress_batch(plz4hip_ctx* c, int nBlocks, const void* const* src, const int32_t* srcLen,
                             void* const* dst, const int32_t* dstCap, int32_t* result)
{
    if (!c || nBlocks < 0 || (nBlocks && (!src || !srcLen || !dst || !dstCap || !result))) return fail(c, PLZ4HIP_E_ARG, "plz4hip_decompress_batch: bad argument");
    return host_codec(c, 1, nBlocks, src, srcLen, dst, dstCap, 0, 0, result, nullptr);
}

int plz4hip_xxh32_batch(plz4hip_ctx* c, int n, const void* const* buf, const int32_t* len, uint32_t* out)
{
    if (!c || n < 0 || (n && (!buf || !len || !out))) return fail(c, PLZ4HIP_E_ARG, "plz4hip_xxh32_batch: bad argument");
    return host_codec(c, 4, n, buf, len, nullptr, nullptr, 0, 0, (int32_t*)out, nullptr);
}

int plz4hip_encode_records(plz4hip_ctx* c, int nBlocks, const void* const* src, const int32_t* srcLen,
                           int bsz, int level, int blockChecksum, void* const* rec, int32_t* recLen)
{
    if (!c || nBlocks < 0 || bsz <= 0 || (nBlocks && (!src || !srcLen || !rec || !recLen))) return fail(c, PLZ4HIP_E_ARG, "plz4hip_encode_records: bad argument");
    for (int i = 0; i < nBlocks; ++i) if (srcLen[i] > bsz) return fail(c, PLZ4HIP_E_ARG, "source block larger than block size");
    if (is_hc_level(level)) { DictJob j; j.level = level; return host_codec(c, 2, nBlocks, src, srcLen, rec, nullptr, bsz, blockChecksum, recLen, nullptr, &j); }
    if (level != 1) return fail(c, PLZ4HIP_E_UNSUPPORTED, "levels 1..12 are built");
    return host_codec(c, 2, nBlocks, src, srcLen, rec, nullptr, bsz, blockChecksum, recLen, nullptr);
}

int plz4hip_decode_records(plz4hip_ctx* c, int nBlocks, const void* const* rec, const int32_t* recLen,
                           int bsz, int blockChecksum, void* const* dst, int32_t* result, int32_t* status)
{
    if (!c || nBlocks < 0 || bsz <= 0 || (nBlocks && (!rec || !recLen || !dst || !result || !status))) return fail(c, PLZ4HIP_E_ARG, "plz4hip_decode_records: bad argument");
    for (int i = 0; i < nBlocks; ++i) if (recLen[i] < 4) return fail(c, PLZ4HIP_E_ARG, "record shorter than its size word");
    return host_codec(c, 3, nBlocks, rec, recLen, dst, nullptr, bsz, blockChecksum, result, status);
}


// ---------------------------------------------------------------------------------------- streaming content checksum
int plz4hip_xxh32_stream_create(plz4hip_ctx* c, plz4hip_xxh32_stream** out)
{
    if (!c || !out) return fail(c, PLZ4HIP_E_ARG, "plz4hip_xxh32_stream_create: bad argument");
    std::lock_guard<std::mutex> g(c->mu);
    ENTER_DEVICE(c);
    if (!c->hashStream) HIPCHK(c, hipStreamCreateWithFlags(&c->hashStream, hipStreamNonBlocking));
    plz4hip_xxh32_stream* h = new (std::nothrow) plz4hip_xxh32_stream();
    if (!h) return fail(c, PLZ4HIP_E_NOMEM, "plz4hip_xxh32_stream");
    hipError_t e = hipMalloc((void**)&h->d_state, sizeof(XxhStream));
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->done, hipEventDisableTiming);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_xxh32_stream, dim3(1), dim3(64), 0, c->hashStream, h->d_state, (const uint8_t*)nullptr, (int64_t)0, (const int32_t*)nullptr, 0, (int64_t)0, 1);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipEventRecord(h->done, c->hashStream);
    }
    if (e != hipSuccess) { if (h->d_state) hipFree(h->d_state); if (h->done) hipEventDestroy(h->done); delete h; return fail(c, PLZ4HIP_E_DEVICE, "plz4hip_xxh32_stream_create", e); }
    *out = h;
    return PLZ4HIP_OK;
}

void plz4hip_xxh32_stream_destroy(plz4hip_ctx* c, plz4hip_xxh32_stream* h)
{
    if (!h) return;
    DeviceGuard dg(c ? c->device : 0);
    if (c) { std::lock_guard<std::mutex> g(c->mu); if (c->contentHash == h) c->contentHash = nullptr; }
    if (h->done) { hipEventSynchronize(h->done); hipEventDestroy(h->done); }
    if (h->d_state) hipFree(h->d_state);
    delete h;
}

int plz4hip_xxh32_stream_reset(plz4hip_ctx* c, plz4hip_xxh32_stream* h)
{
    if (!c || !h) return fail(c, PLZ4HIP_E_ARG, "plz4hip_xxh32_stream_reset: bad argument");
    std::lock_guard<std::mutex> g(c->mu);
    ENTER_DEVICE(c);
    hipLaunchKernelGGL(k_xxh32_stream, dim3(1), dim3(64), 0, c->hashStream, h->d_state, (const uint8_t*)nullptr, (int64_t)0, (const int32_t*)nullptr, 0, (int64_t)0, 1);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(h->done, c->hashStream));
    return PLZ4HIP_OK;
}

int plz4hip_dev_xxh32_stream_update(plz4hip_ctx* c, plz4hip_xxh32_stream* h, const void* data, int64_t n, void* stream)
{
    if (!c || !h || n < 0 || (n && !data)) return fail(c, PLZ4HIP_E_ARG, "plz4hip_dev_xxh32_stream_update: bad argument");
    if (n == 0) return PLZ4HIP_OK;
    std::lock_guard<std::mutex> g(c->mu);
    ENTER_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(c, hipStreamWaitEvent(s, h->done, 0));                       // behind the last update, whichever stream it ran on
    hipLaunchKernelGGL(k_xxh32_stream, dim3(1), dim3(64), 0, s, h->d_state, (const uint8_t*)data, (int64_t)0, (const int32_t*)nullptr, 0, n, 0);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(h->done, s));
    return PLZ4HIP_OK;
}

int plz4hip_xxh32_stream_update(plz4hip_ctx* c, plz4hip_xxh32_stream* h, const void* data, int64_t n)
{
    if (!c || !h || n < 0 || (n && !data)) return fail(c, PLZ4HIP_E_ARG, "plz4hip_xxh32_stream_update: bad argument");
    if (n == 0) return PLZ4HIP_OK;
    std::lock_guard<std::mutex> g(c->mu);
    ENTER_DEVICE(c);
    const size_t piece = (size_t)64 << 20;
    uint8_t* d = nullptr;
    HIPCHK(c, hipMalloc((void**)&d, (size_t)n < piece ? (size_t)n : piece));
    int rc = PLZ4HIP_OK;
    for (int64_t o = 0; o < n && rc == PLZ4HIP_OK; o += (int64_t)piece) {
        const size_t k = (size_t)(n - o) < piece ? (size_t)(n - o) : piece;
        hipError_t e = hipMemcpyAsync(d, (const uint8_t*)data + o, k, hipMemcpyHostToDevice, c->hashStream);
        if (e == hipSuccess) { hipLaunchKernelGGL(k_xxh32_stream, dim3(1), dim3(64), 0, c->hashStream, h->d_state, (const uint8_t*)d, (int64_t)0, (const int32_t*)nullptr, 0, (int64_t)k, 0); e = hipGetLastError(); }
        if (e == hipSuccess) e = hipStreamSynchronize(c->hashStream);
        if (e != hipSuccess) rc = fail(c, PLZ4HIP_E_DEVICE, "plz4hip_xxh32_stream_update", e);
    }
    hipFree(d);
    if (rc == PLZ4HIP_OK) HIPCHK(c, hipEventRecord(h->done, c->hashStream));
    return rc;
}

int plz4hip_xxh32_stream_sum(plz4hip_ctx* c, plz4hip_xxh32_stream* h, uint32_t* out)
{
    if (!c || !h || !out) return fail(c, PLZ4HIP_E_ARG, "plz4hip_xxh32_stream_sum: bad argument");
    std::lock_guard<std::mutex> g(c->mu);
    ENTER_DEVICE(c);
    HIPCHK(c, hipEventSynchronize(h->done));
    XxhStream st;
    HIPCHK(c, copy_sync(c, &st, h->d_state, sizeof st, hipMemcpyDeviceToHost));
    *out = xxh32_stream_sum(st);
    return PLZ4HIP_OK;
}

int plz4hip_ctx_set_content_hash(plz4hip_ctx* c, plz4hip_xxh32_stream* h)
{
    if (!c) return PLZ4HIP_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    c->contentHash = h;
    return PLZ4HIP_OK;
}

// ---------------------------------------------------------------------------------------- dictionaries / linked blocks
int plz4hip_dict_create(plz4hip_ctx* c, const void* dict, int dictLen, plz4hip_dict** out)
{
    if (!c || !out || dictLen < 0 || (dictLen && !dict)) return fail(c, PLZ4HIP_E_ARG, "plz4hip_dict_create: bad argument");
    std::lock_guard<std::mutex> g(c->mu);
    ENTER_DEVICE(c);
    plz4hip_dict* d = new (std::nothrow) plz4hip_dict();
    if (!d) return fail(c, PLZ4HIP_E_NOMEM, "plz4hip_dict");
    const uint8_t* p = (const uint8_t*)dict;
    if (dictLen > 65536) { p += dictLen - 65536; dictLen = 65536; }             // compress/dict.go:43-56, lz4.c:1617
    d->h_bytes.assign(p, p + dictLen);
    d->len = dictLen;
    std::vector<uint32_t> tab(4096);
    build_dict_table_slow(d->h_bytes.data(), dictLen, tab.data());
    hipError_t e = hipMalloc((void**)&d->d_bytes, 65536 + 64);
    if (e == hipSuccess) e = hipMalloc((void**)&d->d_table, 4096 * sizeof(uint32_t));
    if (e == hipSuccess && dictLen) e = copy_sync(c, d->d_bytes, d->h_bytes.data(), (size_t)dictLen, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = copy_sync(c, d->d_table, tab.data(), 4096 * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void**)&d->d_hc, 2 * (size_t)kHcWorkBytes);
    if (e == hipSuccess) e = hipMalloc((void**)&d->d_hcx, (size_t)kHcxDictBytes);
    if (e == hipSuccess) {                                                       // ... and the hash chain as lists, for k_hcx
        std::vector<uint8_t> lists((size_t)kHcxDictBytes, 0);
        hcx_dict_build(d->h_bytes.data(), dictLen, (uint32_t*)lists.data(), (uint16_t*)(lists.data() + kHcxDictStartBytes));
        e = copy_sync(c, d->d_hcx, lists.data(), lists.size(), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) {                                                       // clz4.NewDictCtxHC for both table strategies
        hipLaunchKernelGGL(k_hc_dict_prime, dim3(2), dim3(64), 0, c->stream, (const uint8_t*)d->d_bytes, dictLen, d->d_hc);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    }
    if (e != hipSuccess) { if (d->d_bytes) hipFree(d->d_bytes); if (d->d_table) hipFree(d->d_table); if (d->d_hc) hipFree(d->d_hc); if (d->d_hcx) hipFree(d->d_hcx); delete d; return fail(c, PLZ4HIP_E_DEVICE, "plz4hip_dict_create", e); }
    *out = d;
    return PLZ4HIP_OK;
}

void plz4hip_dict_destroy(plz4hip_ctx* c, plz4hip_dict* d)
{
    if (!d) return;
    DeviceGuard dg(c ? c->device : 0);
    if (d->d_bytes) hipFree(d->d_bytes);
    if (d->d_table) hipFree(d->d_table);
    if (d->d_hc) hipFree(d->d_hc);
    if (d->d_hcx) hipFree(d->d_hcx);
    delete d;
}

int plz4hip_compress_batch_dict(plz4hip_ctx* c, int nBlocks, const void* const* src, const int32_t* srcLen,
                                void* const* dst, const int32_t* dstCap, int level, const plz4hip_dict* dict, int32_t* result)
{
    if (!c || !dict || nBlocks < 0 || (nBlocks && (!src || !srcLen || !dst || !dstCap || !result))) return fail(c, PLZ4HIP_E_ARG, "plz4hip_compress_batch_dict: bad argument");
    if (level != 1 && !is_hc_level(level)) return fail(c, PLZ4HIP_E_UNSUPPORTED, "levels 1..12 are built");
    DictJob j; j.dict = dict; j.any = true; j.level = level;
    return host_codec(c, 0, nBlocks, src, srcLen, dst, dstCap, 0, 0, result, nullptr, &j);
}

int plz4hip_decompress_batch_dict(plz4hip_ctx* c, int nBlocks, const void* const* src, const int32_t* srcLen,
                                  void* const* dst, const int32_t* dstCap, const plz4hip_dict* dict, int32_t* result)
{
    if (!c || !dict || nBlocks < 0 || (nBlocks && (!src || !srcLen || !dst || !dstCap || !result))) return fail(c, PLZ4HIP_E_ARG, "plz4hip_decompress_batch_dict: bad argument");
    DictJob j; j.dict = dict; j.any = true;
    return host_codec(c, 1, nBlocks, src, srcLen, dst, dstCap, 0, 0, result, nullptr, &j);
}

int plz4hip_encode_records_ex(plz4hip_ctx* c, int nBlocks, const void* const* src, const int32_t* srcLen,
                              int bsz, int level, int blockChecksum, int linked, const plz4hip_dict* dict,
                              const void* prevTail, int prevTailLen, void* const* rec, int32_t* recLen)
{
    if (!c || nBlocks < 0 || bsz <= 0 || (nBlocks && (!src || !srcLen || !rec || !recLen))) return fail(c, PLZ4HIP_E_ARG, "plz4hip_encode_records_ex: bad argument");
    if (level != 1 && !is_hc_level(level)) return fail(c, PLZ4HIP_E_UNSUPPORTED, "levels 1..12 are built");
    for (int i = 0; i < nBlocks; ++i) if (srcLen[i] > bsz) return fail(c, PLZ4HIP_E_ARG, "source block larger than block size");
    if (!linked && !dict) {
        if (is_hc_level(level)) { DictJob j; j.level = level; return host_codec(c, 2, nBlocks, src, srcLen, rec, nullptr, bsz, blockChecksum, recLen, nullptr, &j); }
        return host_codec(c, 2, nBlocks, src, srcLen, rec, nullptr, bsz, blockChecksum, recLen, nullptr);
    }
    DictJob j; j.dict = dict; j.linked = linked; j.prevTail = prevTail; j.prevTailLen = (linked && prevTail) ? prevTailLen : -1; j.any = true; j.level = level;
    return host_codec(c, 2, nBlocks, src, srcLen, rec, nullptr, bsz, blockChecksum, recLen, nullptr, &j);
}

int plz4hip_decode_records_ex(plz4hip_ctx* c, int nBlocks, const void* const* rec, const int32_t* recLen,
                              int bsz, int blockChecksum, int linked, const plz4hip_dict* dict,
                              void* window, int* windowLen, void* const* dst, int32_t* result, int32_t* status)
{
    if (!c || nBlocks < 0 || bsz <= 0 || (nBlocks && (!rec || !recLen || !dst || !result || !status))) return fail(c, PLZ4HIP_E_ARG, "plz4hip_decode_records_ex: bad argument");
    for (int i = 0; i < nBlocks; ++i) if (recLen[i] < 4) return fail(c, PLZ4HIP_E_ARG, "record shorter than its size word");
    if (!linked && !dict) return host_codec(c, 3, nBlocks, rec, recLen, dst, nullptr, bsz, blockChecksum, result, status);
    if (linked && (!window || !windowLen || *windowLen < 0 || *windowLen > 65536)) return fail(c, PLZ4HIP_E_ARG, "linked decode needs the 64 KiB window state");
    DictJob j; j.dict = dict; j.linked = linked; j.any = true;
    if (linked) { j.window = (uint8_t*)window; j.windowLen = windowLen; j.dict = nullptr; }
    return host_codec(c, 3, nBlocks, rec, recLen, dst, nullptr, bsz, blockChecksum, result, status, &j);
}

int plz4hip_decode_records_chains(plz4hip_ctx* c, int nChains, const int32_t* chainFirst, const void* const* rec, const int32_t* recLen,
                                  int bsz, int blockChecksum, void* windows, int32_t* windowLen,
                                  void* const* dst, int32_t* result, int32_t* status)
{
    if (!c || nChains < 0 || bsz <= 0 || (nChains && (!chainFirst || !windows || !windowLen))) return fail(c, PLZ4HIP_E_ARG, "plz4hip_decode_records_chains: bad argument");
    if (nChains == 0) return PLZ4HIP_OK;
    if (chainFirst[0] != 0) return fail(c, PLZ4HIP_E_ARG, "chainFirst[0] must be 0");
    for (int k = 0; k < nChains; ++k) {
        if (chainFirst[k + 1] < chainFirst[k]) return fail(c, PLZ4HIP_E_ARG, "chainFirst must not decrease");
        if (windowLen[k] < 0 || windowLen[k] > 65536) return fail(c, PLZ4HIP_E_ARG, "window length out of range");
    }
    const int nBlocks = chainFirst[nChains];
    if (nBlocks && (!rec || !recLen || !dst || !result || !status)) return fail(c, PLZ4HIP_E_ARG, "plz4hip_decode_records_chains: bad argument");
    if (nBlocks == 0) return PLZ4HIP_OK;
    for (int i = 0; i < nBlocks; ++i) if (recLen[i] < 4) return fail(c, PLZ4HIP_E_ARG, "record shorter than its size word");
    DictJob j; j.linked = 1; j.any = true; j.window = (uint8_t*)windows; j.windowLen = windowLen; j.nChains = nChains; j.chainFirst = chainFirst;
    return host_codec(c, 3, nBlocks, rec, recLen, dst, nullptr, bsz, blockChecksum, result, status, &j);
}

}  // extern "C"
