// lz4_block_io.inl -- what every block encoder kernel does around its encoder: how block i of a call is primed, and how one wave
// turns an encoder's return value into a frame record.  Both are byte-exact frame-format rules; they live here once, on plain
// pointers, so that the lane emulation (g++ -DPLZ4_EMU, tests/test_block_io.py) holds them to the reference without a GPU.
//
// Priming.  plz4 primes a block's stream with one of: the previous block's last <= 64 KiB (linked frames: async/writer.go:412-437
// _genDict, clz4.go:224-248 StreamLinkedCtx, :250-283 StreamLinkedCtxHC), the call's dictionary context (clz4.go:160-179
// StreamIndieCtx, :181-209 StreamCtxHC; lz4hc.c:1438-1461), or nothing.  hist_of answers which, and copies nothing; l1_prime and
// hc_prime map the answer to what the level-1 and the HC encoders take.  A dictionary context serves a block of at most
// kCtxMaxBlock bytes by lookup (usingDictCtx); above that liblz4 copies its state in, which is the same as an external segment.
// In the dictionary / linked modes every input block has 64 KiB of scratch in front of it (host_codec lays the staging out that
// way; device-resident plaintext is contiguous): lay_segment puts an external segment there, right before the block, which is
// what wave_encode_block_ext and hc_compress(kHcExt) read.
//
// Records.  blk.CompressToBlk (blk/blk.go:69-109): [LE32 size | stored bit][payload][LE32 xxh32 of the payload as stored?], the
// plaintext stored when the encoder returned 0 (ErrCompress, blk.go:78-92).  The staged emit stage (l1_sizes_body / l1_write_body /
// k_l1_finish, plz4hip.hip) writes the same words one lane per sequence and is not this writer's business.
#pragma once
#include "lz4_device.inl"
#include "lz4hc_device.inl"

#if defined(PLZ4_EMU)
#define BIO_HD static inline
#else
#define BIO_HD __host__ __device__ __forceinline__
#endif

namespace plz4 {

// the largest block a dictionary context serves by lookup (lz4.c:1738-1745, lz4hc.c:1449: 4 KiB)
enum : int { kCtxMaxBlock = 4096 };

// what the rule reads of a call: CodecArgs' fields of the same names (hist_view, plz4hip.hip)
struct HistView {
    const uint8_t* src;  int64_t srcStride;  const int32_t* srcLen;  int64_t srcBytes;  int bsz;
    int            linked;
    const uint8_t* prevTail;  int prevTailLen;      // linked: the window of block 0 (-1: block 0 starts a frame)
    const uint8_t* dict;      int dictLen;          // the dictionary context's last <= 64 KiB; (null, -1): none attached
};
BIO_HD int view_block_len(const HistView& v, int i)
{
    if (v.srcLen) return v.srcLen[i];
    const int64_t rem = v.srcBytes - (int64_t)i * v.bsz;
    return (int)(rem < v.bsz ? rem : v.bsz);
}
// how much of a previous block of pl bytes the next linked block sees (_genDict: its last <= 64 KiB)
BIO_HD int tail_len(int pl) { return pl < 65536 ? pl : 65536; }

enum : int { kSeesNothing = 0, kSeesTail = 1, kSeesDict = 2 };
struct Hist {
    int            kind;
    const uint8_t* bytes;   // kSeesTail: the tail; kSeesDict: the dictionary (null when it is empty)
    int            len;     // kSeesTail: >= 0; kSeesDict: the context's dictLen as attached (<= 0: an empty one)
    bool           small;   // kSeesDict: the block is one the context serves by lookup
};
// the two questions the answer is made of: does a linked call put a block or a window in front of block i (the block API has no
// linked mode), and is a dictionary context attached (possibly an empty one)
BIO_HD bool follows_linked(const HistView& v, int i, bool rawApi) { return !rawApi && v.linked && (i > 0 || v.prevTailLen >= 0); }
BIO_HD bool ctx_attached(const HistView& v) { return v.dict != nullptr || v.dictLen >= 0; }
// Which history block i (n bytes) of the call sees.
BIO_HD Hist hist_of(const HistView& v, int i, int n, bool rawApi)
{
    if (follows_linked(v, i, rawApi)) {
        if (i == 0) return Hist{kSeesTail, v.prevTail, v.prevTailLen, false};
        const int pl = view_block_len(v, i - 1), tl = tail_len(pl);
        if (tl >= 0) return Hist{kSeesTail, v.src + (int64_t)(i - 1) * v.srcStride + (pl - tl), tl, false};   // (< 0, a bad length: no tail)
    }
    if (ctx_attached(v)) return Hist{kSeesDict, v.dict, v.dictLen, n <= kCtxMaxBlock};
    return Hist{kSeesNothing, nullptr, 0, false};
}
// Whether block i is one the context serves by lookup -- hist_of(...) being kSeesDict and small -- without reading the block
// before it: what a kernel asks per block to pass the block over or take it (k_hcx and the one-thread HC kernels).  A linked
// block behind a block of a bad (negative) length counts as linked here, as it always did: the one-thread kernels encode it.
BIO_HD bool ctx_small(const HistView& v, int i, int n, bool rawApi) { return n <= kCtxMaxBlock && !follows_linked(v, i, rawApi) && ctx_attached(v); }

// Level 1 (LZ4_compress_fast_continue).  LZ4_loadDict drops a tail or dictionary shorter than 8 bytes: the stream keeps its
// 64 KiB index offset and no history (kDictNonePrefix).  Unattached is a linked frame's first block (a fresh stream,
// kDictFreshPrefix); the block API always runs as under a context, an empty one when there is none.  table: the context's.
BIO_HD DictEnc l1_prime(const Hist& h, bool rawApi, const uint32_t* table = nullptr)
{
    if (h.kind == kSeesNothing) return DictEnc{nullptr, 0, rawApi ? kDictNonePrefix : kDictFreshPrefix, nullptr};
    if (h.len < 8) return DictEnc{nullptr, 0, kDictNonePrefix, nullptr};
    if (h.kind == kSeesTail) return DictEnc{h.bytes, h.len, kDictLoad, nullptr};
    return DictEnc{h.bytes, h.len, h.small ? kDictCtxLookup : kDictCtxCopy, table};
}
// HC (LZ4_compress_HC_continue): a tail or a copied-in dictionary of ANY length, 0 included, is an external segment (kHcExt, its
// bytes: h.bytes, to be laid in front of the block); hash / chain: the context's tables (hc_prime_dict), used by kHcCtx only.
BIO_HD HcDict hc_prime(const Hist& h, const uint32_t* hash = nullptr, const uint16_t* chain = nullptr)
{
    HcDict d; d.mode = kHcNone; d.len = 0; d.bytes = nullptr; d.hash = nullptr; d.chain = nullptr;
    if (h.kind == kSeesNothing) return d;
    d.len = h.len > 0 ? h.len : 0;
    if (h.kind == kSeesDict && h.small) { d.mode = kHcCtx; d.bytes = h.bytes; d.hash = hash; d.chain = chain; }
    else d.mode = kHcExt;
    return d;
}
// what the list path notes per block (CodecArgs::hcPfx): the bytes of the segment in front of it, -1: a block under a context
BIO_HD int hc_pfx(const HcDict& d) { return d.mode == kHcCtx ? -1 : (d.mode == kHcExt ? d.len : 0); }

// The external segment seg[0, len) right before the block at s -- unless it lies there already (the tail of the block before in
// contiguous plaintext stays: its neighbours read it).
DEV void lay_segment(const uint8_t* s, const uint8_t* seg, int len)
{
    if (len > 0 && seg != s - len) { wave_copy(const_cast<uint8_t*>(s) - len, seg, len); WAVE_FENCE(); }
}

// One level-1 block primed as l1_prime says: an external segment laid right before the block and the full encoder in its
// external-segment mode (wave_encode_block_ext).  Only the dictionary-context lookup keeps the one-sequence-per-batch encoder.
DEV int encode_block_primed(const uint8_t* s, int n, uint8_t* out, int cap, const DictEnc& dc, uint32_t* lds)
{
    if (dc.mode == kDictCtxLookup) return wave_encode_block_dict(s, n, out, cap, dc, lds);
    const int segLen = (dc.mode == kDictLoad || dc.mode == kDictCtxCopy) ? dc.dictSize : 0;
    lay_segment(s, dc.dict, segLen);
    return wave_encode_block_ext(s, n, out, cap, dc.mode, segLen, dc.dictTable, lds);
}

// The record of block s[0, n) whose encoder wrote c bytes at rec + 4 (0: they do not fit in the capacity, the block is stored).
// Returns the record's length.  One wave.  The fences are wavefront-scope: they keep the compiler from moving the fallback copy
// in front of the encoder's last stores to the same bytes, and the checksum's loads in front of the payload's stores.  The
// level-1 encoders used to go without the first one; it is a wait, no cache action (WAVE_FENCE, wave.h; the kernels' s_waitcnt counts before
// and after: profiles/block_io_resources.txt) and changes no byte: every caller has the HC kernels' order now, on purpose.
DEV int wave_finish_record(uint8_t* rec, const uint8_t* s, int n, int c, bool blockChecksum)
{
    uint32_t word = (uint32_t)c & 0x7FFFFFFFu;
    WAVE_FENCE();
    if (c == 0) { wave_copy(rec + 4, s, n); c = n; word = 0x80000000u | ((uint32_t)n & 0x7FFFFFFFu); }
    int len = c + 4;
    if (blockChecksum) {                                                     // over the payload as stored (blk.go:98-102)
        WAVE_FENCE();
        const uint32_t x = wave_xxh32(rec + 4, c);
        LANES({ if (LANE == 0) st32u(rec + 4 + c, x); })
        len += 4;
    }
    LANES({ if (LANE == 0) st32u(rec, word); })
    return len;
}

}  // namespace plz4
