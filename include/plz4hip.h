/*
 * plz4hip.h -- C ABI of the MI355X (gfx950) LZ4 block engine that replaces plz4's cgo -> liblz4 engine.
 *
 * Drop-in boundary.  Today plz4 crosses from Go into C once per block through
 * internal/pkg/clz4/clz4.go (CompressFast :31-45, DecompressSafe :47-60, CompressBound :27-29) underneath
 * compress.Compressor / compress.Decompressor (internal/pkg/compress/compress.go:7-13, decompress.go:14-16),
 * called from blk.CompressToBlk (internal/pkg/blk/blk.go:69-109), BlkT.Decompress (blk.go:50-61) and the
 * raw block API (plz4_block.go:96-172); the per-block checksum is xxh32.ChecksumZero (blk.go:98-102,
 * blk/frame.go:114-127).  One cgo call per 4 MiB block cannot feed a GPU, so this ABI is the same contract
 * in BATCH form and sits where the reference's worker loops sit (async/writer.go:232-282 compressLoop,
 * async/reader.go:192-221 _decompressLoop): N independent blocks in, N per-block results out.
 * A one-block batch behaves exactly like the per-block call it replaces.
 *
 * Value semantics are liblz4's: encode result > 0 = bytes written, 0 = "cannot compress within dst"
 * (clz4.ErrLz4Compress -> zerr.ErrCompress -> the caller stores the block raw, blk.go:78-92);
 * decode result >= 0 = bytes, < 0 = liblz4's error code (clz4.ErrLz4Decompress -> zerr.ErrCorrupted).
 * The function return value is separate and reports engine/runtime failures (PLZ4HIP_E_*); those must NOT be
 * turned into stored blocks by the caller.
 *
 * Plain C, pointers and sizes only.  Host-pointer entry points never retain caller memory after return.
 * Thread-safety: a ctx serialises its own calls with an internal mutex; every entry point runs on the ctx's device and
 * puts the calling thread's current HIP device back before it returns (goroutines migrate between OS threads); use one
 * ctx per writer/reader for concurrency, one per device for several GPUs (section D).  plz4hip_last_error returns the
 * calling thread's own copy of the text (valid until that thread asks again).
 * Memory: the host-buffer calls keep their pinned host + device staging (up to 3 chunks of <= 4 GiB; one of <= 12 GiB at the HC
 * levels, which run a chunk at a time), level 1 its sequence records (2.25 bytes per input byte of the largest group of blocks
 * in one call, at most half of what is free: PLZ4HIP_L1_BUDGET_GIB; a second such workspace when calls arrive on a second stream
 * while the first one is busy, so that the two need not wait for each other -- PLZ4HIP_L1_WORKSPACES=1: never) and the HC levels
 * their workspaces between calls;
 * plz4hip_ctx_trim gives them back.  The HC workspaces are sized by the call: on independent blocks levels 3..11 keep 14.5 bytes
 * per input byte of the blocks in flight (chain, per-hash lists, sequence records of the segments), level 12 22.5 (the search results as well), level 2 2.25, out
 * of a quarter of the device memory that is free when the call arrives, at most 64 GiB; a call whose blocks do not fit runs in
 * groups.  A caller that owns the GPU raises the budget with PLZ4HIP_HC_BUDGET_GIB (these kernels live on blocks in flight).
 * With a dictionary and / or linked blocks the HC levels run the same designs over segment + block (strides for 4 MiB + 64 KiB).
 * A block of at most 4 KiB under an attached dictionary (compress_batch_dict, encode_records_ex, dev_encode_records_ex, the host
 * layer's Writer with a dictionary: a short payload or a short last block) keeps its own empty tables and searches the dictionary
 * context's behind them (lz4hc.c:1442-1463).  At levels 2..12 such a block is one wavefront's: its chain as lists in 17 KiB of LDS
 * (level 2: its two direct-mapped tables, compacted to the hashes the block has, in 21 KiB),
 * the dictionary's chain as lists built once by plz4hip_dict_create (256 KiB per dictionary), one candidate per lane, no workspace
 * in device memory at levels 3..9 (levels 10..12: a price table, level 2: the sequence records, per wave out of the HC workspace); all such blocks of a call are
 * one launch off the block queue.  PLZ4HIP_HCX=0 (read per call) keeps the one-thread parsers.  Bytes and results are the same
 * either way.
 * A DECODE call of few blocks (decompress_batch, decode_records and their dev_ forms, up to PLZ4HIP_DX_MAX_BLOCKS = 128 blocks of up
 * to 4 MiB + 8 of output; 0 turns it off) is cut across the whole chip and keeps 8 bytes per input byte + 4 per output byte of
 * the call's blocks (about 50 MiB per 4 MiB block) until plz4hip_ctx_trim; results and error codes are LZ4_decompress_safe's
 * either way (a block that path will not answer for is decoded by the one-wavefront decoder inside the call).
 * RAW blocks above 4 MiB + 8 of capacity without history outside the block (decompress_batch, dev_decompress, the host layer's
 * DecompressBlock; a frame's block stops at 4 MiB) take the path as well: a call of up to PLZ4HIP_DX_MAX_BLOCKS blocks whose largest
 * capacity is above 4 MiB + 8 and at most PLZ4HIP_DX_BIG_MAX_MIB MiB + 8 (default and ceiling 1024; read per call) runs every block
 * of the call, the small ones beside the large, through the stages cut once more -- the stitch in groups of segments, length bytes
 * 64 a step, literal runs and matches of 64 KiB or more by the whole grid, ceil(log2(capacity)) + 1 jump rounds.  PLZ4HIP_DX_BIG=0
 * keeps every block above 4 MiB + 8 on the one-wavefront decoder (for tests and A/B runs).  The workspace is 8 bytes per input byte
 * + 4 per output byte of the call's largest block per block, and some 3 % of that for the groups and the run list: ONE 1 GiB BLOCK
 * OF TEXT KEEPS ABOUT 7 GiB (4 GiB of pointers, 8 B x its compressed length), an incompressible one 12 GiB, until plz4hip_ctx_trim;
 * a workspace that cannot be had leaves the call to one wavefront per block.  Left to the one-wavefront decoder: blocks above the
 * limit, blocks above 4 MiB under a dictionary (decompress_batch_dict: their pointer space tags bit 31), and every block the path
 * finds less than plainly valid -- an output beyond the capacity among them.  Records stay at 4 MiB, and so do all encoders.
 * Blocks with history outside the block take the same path under the same conditions (decompress_batch_dict, decode_records_ex
 * with a dictionary and / or linked = 1, decode_records_chains): the call has one pointer space, a match that starts in front of
 * its block points into an earlier block's output, the window the call came in with or the dictionary, and the jump rounds follow
 * the call's total output (up to 32).  A chain is answered up to its first block that is not plainly good; the one-wavefront chain
 * walk goes on from there inside the call, from the window the good blocks leave.  The blocks of a chain behind a record that
 * fails the frame reader's checks (PLZ4HIP_BLK_SIZE_OVERFLOW) are not decoded on this path either: their output stays as it was,
 * as on the walk.  PLZ4HIP_DX_LINKED=0 keeps such calls on the
 * one-wavefront kernels (a switch for tests and A/B runs; PLZ4HIP_DX_MAX_BLOCKS=0 does so too).
 * A LINKED call of more blocks than that (decode_records_ex with linked = 1, decode_records_chains, dev_decode_records_ex) is cut
 * into groups of PLZ4HIP_DXL_GROUP_BLOCKS consecutive blocks (default 128; read per call), each group the same path across the whole
 * chip, one behind the other on the call's stream: a block needs only the 64 KiB in front of it, so the window, its length and one
 * word per chain (the chain has had a bad block: its later blocks are PLZ4HIP_BLK_CORRUPT with result 0) go from group to group in
 * device memory and the host never waits in between.  The workspace is that of one group.  Results, status, bytes and windows are
 * those of the one-wavefront walk.  Groups are taken when blocks x 0.33 ms <= longest chain x 59 ms -- few long chains; many short
 * chains keep one wavefront per chain -- and PLZ4HIP_DXL_GROUP_BLOCKS=0 keeps every call beyond PLZ4HIP_DX_MAX_BLOCKS on the walk
 * (set to a number, it also cuts calls that would fit one pass: a switch for tests and measurements).
 * An ENCODE call of few blocks at level 1 (compress_batch, encode_records, dev_compress with maxLen > 0, dev_encode_records,
 * dev_encode_body; up to PLZ4HIP_FX_MAX_BLOCKS = 128 blocks, 0 turns it off) whose largest block is 65 547 bytes .. 4 MiB (liblz4's
 * byU32 tables) has its parse cut across the whole chip: pieces of PLZ4HIP_FX_PIECE_KIB (64) parsed by a wave each, in rounds
 * until every piece starts from the exact state its predecessor ends in; a guessed start begins PLZ4HIP_FX_WARMUP_KIB (64) early.
 * Output, results and error codes are exactly those of the one-wave parse; smaller blocks of such a call are parsed whole.
 * A level-1 call with a dictionary and/or linked blocks through host buffers (compress_batch_dict, encode_records_ex, and the
 * multi-GPU / host-layer routes that end there) takes the same path under the same limits, per staging chunk: the segment -- the
 * previous block's tail or the dictionary -- is laid in front of every block and the table liblz4 starts the block with is the
 * first piece's entry state; every block of such a call may be shorter than a piece, only blocks <= 4 KiB under a dictionary
 * context keep their two-table encoder.  PLZ4HIP_FX_LINKED=0 (read per call) keeps such calls on one wavefront per block.
 * The device-resident calls with history outside the block (dev_encode_records_ex, dev_encode_body_ex) take it likewise; a call of
 * more blocks there runs the staged level-1 design with one wavefront per block and holds the level-1 workspace above (2.25 bytes
 * per input byte of a group of blocks), PLZ4HIP_L1X=0 the one-kernel encoder (see section C).
 * Duplex calls keep their kernels.  It keeps about 3 bytes per input byte of the call's blocks (the pieces' tables
 * and records) until plz4hip_ctx_trim.  plz4hip_ctx_counters reports what these few-block paths did.
 * A level-2 call (LZ4MID) of at most PLZ4HIP_MX_MAX_BLOCKS (512; 0: off) independent blocks, the largest above one piece and at most 4 MiB, without
 * a dictionary, linked blocks or a rider, has its walk cut across the chip the same way: pieces of PLZ4HIP_MX_PIECE_KIB (128), a
 * guessed start PLZ4HIP_MX_WARMUP_KIB (256) early -- level 2's tables have one slot per four positions of the window, so a wrong
 * entry lives for a whole window.  Blocks of at most one piece are one piece of the same call.  Output, results, error codes and
 * capacity verdicts are exactly those of one wavefront per block; a call the path does not take, or whose workspace is refused
 * (about 5 bytes per input byte: three 128 KiB states and the records per piece, kept until plz4hip_ctx_trim), runs that launch.
 * A level-2 call with a dictionary and/or linked blocks (compress_batch_dict, encode_records_ex, dev_encode_records_ex,
 * dev_encode_body_ex and the multi-GPU / host-layer routes that end there; host buffers: per staging chunk) of at most
 * PLZ4HIP_MXL_MAX_BLOCKS (512; 0: off; read per call) blocks, the largest above one piece and at most 4 MiB, without a rider, takes the same
 * walk in pieces behind every block's external segment -- the previous block's tail or the dictionary -- under the same
 * PLZ4HIP_MX_PIECE_KIB / PLZ4HIP_MX_WARMUP_KIB and with the same workspace (about 5 bytes per input byte, kept until
 * plz4hip_ctx_trim); blocks of at most 4 KiB under a dictionary context keep their wave-wide parser.  Same bytes, results and
 * capacity verdicts; a call the path does not take, or whose workspace is refused, runs one wavefront per block.
 * A call at levels 3..12 of at most PLZ4HIP_HB_MAX_BLOCKS (64; 0: off; read per call) blocks of at most 4 MiB -- independent ones, or blocks
 * behind a dictionary / linked blocks on the list path (compress_batch, compress_batch_dict, encode_records, encode_records_ex,
 * dev_compress, dev_encode_records, dev_encode_records_ex and the routes that end there; host buffers: per staging chunk) -- whose
 * largest segment + block is above one piece has the chains and per-hash lists in front of its walk built in pieces of
 * PLZ4HIP_HB_PIECE_KIB (64, clamped to 1..4096) KiB of positions by many workgroups per block (count, scan, fill, chain: four launches, nobody waits for
 * anybody) instead of one wavefront per block.  The arrays are the same, and so are the searches and walks behind them: output,
 * results and capacity verdicts are unchanged.  The workspace is two 128 KiB tables per piece (16 MiB per 4 MiB block at 64 KiB
 * pieces), kept until plz4hip_ctx_trim; a call the path does not take -- more blocks, raw blocks above 4 MiB, the calls of 2048
 * blocks and more that build the next group's lists beside a walk -- or whose workspace is refused keeps one wavefront per block.
 * plz4hip_ctx_counters [17] and [18] report what the path did.
 * Other environment switches, for tests and experiments only: PLZ4HIP_HC_EXT_OFF (the one-thread HC parsers for dictionary / linked
 * calls, rounds 1-3), PLZ4HIP_HC12_LAZY (level 12 with its searches made on demand), PLZ4HIP_HC_OVERLAP_OFF / _MIN / _GROUPS (levels 3..11: a call of 2048
 * blocks or more runs in four or more groups, the list builder of the next group on a second stream of the ctx beside the walk
 * of the current one), PLZ4HIP_DUPLEX=P,D / PLZ4HIP_DUPLEX_PRIO (parser + decoder waves per workgroup of the duplex call),
 * PLZ4HIP_HC_SEGS / PLZ4HIP_HC_MIN_SEG (segments a block is walked
 * in at levels 3..11, default up to 512 of at least 8 KiB), PLZ4HIP_HC_LAZY_OFF / PLZ4HIP_HC_MID_OFF / PLZ4HIP_HC12_OFF / PLZ4HIP_L1_FUSED
 * (the one-kernel paths of rounds 1-2 instead), PLZ4HIP_HOST_CHUNK_MB, PLZ4HIP_VERBOSE.
 */
#ifndef PLZ4HIP_H
#define PLZ4HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PLZ4HIP_ABI_VERSION 2

enum {
    PLZ4HIP_OK            =  0,
    PLZ4HIP_E_ARG         = -1,   /* bad argument */
    PLZ4HIP_E_DEVICE      = -2,   /* HIP runtime / kernel failure (see plz4hip_last_error) */
    PLZ4HIP_E_NOMEM       = -3,   /* host or device allocation failed */
    PLZ4HIP_E_UNSUPPORTED = -4    /* level / mode not built yet */
};

/* Per-block status of the record-level decode (plz4hip_decode_records, plz4hip_dev_decode_records). */
enum {
    PLZ4HIP_BLK_OK            = 0,
    PLZ4HIP_BLK_HASH_MISMATCH = 1,   /* zerr.ErrBlockHash        (blk/frame.go:114-127) */
    PLZ4HIP_BLK_SIZE_OVERFLOW = 2,   /* zerr.ErrBlockSizeOverflow (blk/frame.go:79-81)  */
    PLZ4HIP_BLK_CORRUPT       = 3    /* zerr.ErrDecompress: liblz4 returned < 0 (compress/decompress.go:32-38) */
};

typedef struct plz4hip_ctx plz4hip_ctx;

int         plz4hip_abi_version(void);
int         plz4hip_device_count(void);                       /* <0: PLZ4HIP_E_DEVICE */
int         plz4hip_ctx_create(int device, plz4hip_ctx** out);
void        plz4hip_ctx_destroy(plz4hip_ctx* ctx);            /* waits for the ctx's jobs still in flight on the callers' streams */
const char* plz4hip_last_error(const plz4hip_ctx* ctx);       /* text of the last PLZ4HIP_E_* on this ctx */
int         plz4hip_ctx_trim(plz4hip_ctx* ctx);                /* release staging buffers and HC workspaces (waits for work in flight) */
/* Waits for the ctx's work, then writes up to n counters to out: [0] blocks encoded by the few-block level-1 path, [1] its rounds
 * in the last such call, [2] pieces it parsed more than once, [3] blocks answered by the few-block decoder, [4] blocks with history
 * outside the block (dictionary, linked) answered by it, [5] its jump rounds in the last such call (the maximum over the groups of
 * a call cut into groups), [6] the groups of the last call that was cut into groups, [7] blocks with history outside the block encoded by
 * the few-block level-1 path (a subset of [0]), [8] blocks with history outside the block parsed by the staged one-wavefront-per-block
 * route of plz4hip_dev_encode_records_ex / _body_ex (not those the one-kernel encoder took), [9] blocks of at most 4 KiB under a
 * dictionary context encoded by the wave-wide HC parser (levels 2..12), [10] raw blocks above 4 MiB + 8 of capacity answered by the
 * few-block decoder (they count in [3] as well), [11] the jump rounds launched for the last call with such a block, [12] the literal
 * runs and matches that call handed to its grid-wide stage, [13] blocks encoded by the few-block level-2 path, [14] its rounds that
 * parsed something in the last such call, [15] pieces it parsed more than once ([14] and [15]: with or without history outside the block), [16] blocks with history outside
 * the block encoded by the few-block level-2 path (a subset of [13]), [17] blocks of levels 3..12 whose chains and lists were built
 * in pieces across the chip, [18] the pieces per block of the last such call (its largest segment + block, cut).  Returns how
 * many counters there are (19), or PLZ4HIP_E_*. */
int         plz4hip_ctx_counters(plz4hip_ctx* ctx, int64_t* out, int n);

/* == clz4.CompressBound (clz4.go:27-29) -> LZ4_compressBound (lz4.h:215).  Pure host arithmetic. */
int plz4hip_compress_bound(int n);

/* ---------------------------------------------------------------------------------------------------------
 * A. Batched Compressor / Decompressor over HOST buffers (what the cgo shim calls).
 *    Replaces clz4.CompressFast (clz4.go:31-45) / clz4.DecompressSafe (clz4.go:47-60) x nBlocks.
 *    level: 1 (== LZ4_compress_fast(accel 1), compress/indie.go:66-74) and 2..12 (== LZ4_compress_HC(level),
 *           compress/indie.go:80-88 -> clz4.CompressHC clz4.go:80-94 -> lz4hc.c:1519: lz4mid at 2, hash chain at 3..9,
 *           optimal parser at 10..12); anything else is PLZ4HIP_E_UNSUPPORTED.  encode_records / dev_encode_records
 *           take the same levels.
 *    result[i]: encode  > 0 bytes written into dst[i], 0 = liblz4 "does not fit dstCap[i]";
 *               decode >= 0 bytes written, < 0 liblz4 error code.
 *    Decode, whatever the input holds: a call reads no byte outside the srcLen[i] bytes of src[i] and the dictionary, and it
 *    writes no byte outside the dstCap[i] bytes of dst[i].
 *    Encode, whatever its verdict: a call writes no byte outside the dstCap[i] bytes of dst[i] -- a block that does not fit
 *    (result 0) may leave anything inside them, nothing behind them.
 * ------------------------------------------------------------------------------------------------------- */
int plz4hip_compress_batch(plz4hip_ctx* ctx, int nBlocks,
                           const void* const* src, const int32_t* srcLen,
                           void* const* dst, const int32_t* dstCap,
                           int level, int32_t* result);

int plz4hip_decompress_batch(plz4hip_ctx* ctx, int nBlocks,
                             const void* const* src, const int32_t* srcLen,
                             void* const* dst, const int32_t* dstCap,
                             int32_t* result);

/* == xxh32.ChecksumZero (xxh32zero.go:238-280) x n. */
int plz4hip_xxh32_batch(plz4hip_ctx* ctx, int n, const void* const* buf, const int32_t* len, uint32_t* out);

/* ---------------------------------------------------------------------------------------------------------
 * B. Frame records over HOST buffers: blk.CompressToBlk (blk.go:69-109) / FrameReader._read + BlkT.Decompress
 *    (blk/frame.go:54-127, blk.go:50-61) fused on the device.
 *    encode: rec[i] (>= bsz+8 bytes) receives [LE32 size | 0x80000000 if stored][payload][LE32 xxh32(payload)?];
 *            encoder capacity is bsz (NOT the bound); stored raw iff the encoder returns 0.  recLen[i] = bytes.
 *    decode: rec[i]/recLen[i] is one such record (size word included); dst[i] has bsz+8 bytes like the
 *            reference's pooled block (blk/pool.go:23-26); status[i] = PLZ4HIP_BLK_*, result[i] = plaintext bytes
 *            (or liblz4's negative code when status is PLZ4HIP_BLK_CORRUPT).
 *            Whatever the record holds -- a size word that lies, fewer bytes than a size word -- a decode call reads no byte
 *            outside rec[i]'s recLen[i] bytes and the dictionary or window, and writes no byte outside dst[i]'s bsz+8 bytes.
 * ------------------------------------------------------------------------------------------------------- */
int plz4hip_encode_records(plz4hip_ctx* ctx, int nBlocks,
                           const void* const* src, const int32_t* srcLen,
                           int bsz, int level, int blockChecksum,
                           void* const* rec, int32_t* recLen);

int plz4hip_decode_records(plz4hip_ctx* ctx, int nBlocks,
                           const void* const* rec, const int32_t* recLen,
                           int bsz, int blockChecksum,
                           void* const* dst, int32_t* result, int32_t* status);

/* ---------------------------------------------------------------------------------------------------------
 * B'. Dictionaries and linked blocks (levels 1..12; SURVEY.md §8a-11, BASELINE config 5).
 *    plz4hip_dict == clz4.DictCtx + clz4.DictCtxHC (clz4.go:96-147: private copy of the last 64 KiB, the LZ4_loadDictSlow
 *                   table for level 1, the LZ4_loadDictHC tables for level 2 (lz4mid) and for levels 3..12 (hash chain)),
 *                   and the hash chain's positions once more as ascending runs per hash (256 KiB, built on the host by
 *                   plz4hip_dict_create, freed by plz4hip_dict_destroy): what the wave-wide parser of small blocks reads
 *                   one candidate per lane.  About 900 KiB of device memory per dictionary in all.
 *    *_batch_dict : level 1: clz4.StreamIndieCtx.Compress (clz4.go:160-179); levels 2..12: clz4.StreamCtxHC.Compress
 *                   (clz4.go:191-209 -> LZ4_compress_HC_continue under an attached dictionary, lz4hc.c:1438-1461);
 *                   clz4.DecompressSafeWithDict (clz4.go:62-78) per block -- i.e. CompressBlock/DecompressBlock with
 *                   WithBlockDictionary (plz4_block.go:48-53).
 *                   HC levels: a block of at most 4 KiB keeps its own empty tables and searches the dictionary context's
 *                   behind them (usingDictCtxHc, lz4hc.c:1442-1463).  Every such block of a call -- here, in
 *                   encode_records_ex and in dev_encode_records_ex (block 0 of a linked frame without prevTail included) --
 *                   is one wavefront's, all of them one launch off the block queue; a call of nothing but such blocks is
 *                   that launch alone.  Levels 3..12: chain as lists in 17 KiB of LDS; level 2: its two tables in 21 KiB.
 *                   PLZ4HIP_HCX=0 (read per call): the one-thread parsers; same bytes.  Counter [9] counts them.
 *    encode_records_ex: `dict` = WithDictionary; `linked` = WithBlockLinked: block i>0 is primed with the last <= 64 KiB of
 *                   src[i-1] (async/writer.go:412-437 -> LZ4_loadDict, clz4.go:224-241; levels 2..12: LZ4_loadDictHC,
 *                   clz4.go:262-283); block 0 with prevTail when the batch continues a frame (prevTail == NULL: block 0
 *                   starts the frame and uses `dict`, if any).  As everywhere, a block the encoder cannot fit into bsz
 *                   bytes comes back as a stored record; NOTE that the reference's linked HC compressor does not: it
 *                   fails the write instead (compress/linked.go:47-49 returns the error without zerr.ErrCompress, so
 *                   blk.CompressToBlk takes no fallback) -- a drop-in caller checks the stored bit of rec[i] for
 *                   linked && level > 1 and reports the error (the host layer and the Go shim do).
 *                   At level 1 a call of few blocks (see ENCODE above) has every block's parse cut across the chip: for
 *                   the encoder linked blocks are no chain -- block i needs the PLAINTEXT tail of block i-1, which the
 *                   call's input holds -- so every block and every piece starts at once.  Same records, byte for byte.
 *    decode_records_ex: independent blocks + dict: every block against `dict` (compress/decompress.go:42-58);
 *                   linked: the batch is one chain; `window` (64 KiB, caller-owned) / `*windowLen` carry
 *                   compress.DictT (compress/dict.go:5-56) across calls: initialise with the dictionary's last 64 KiB
 *                   (or length 0).  As in the reference, a stored block does not update the window.
 *                   A call of few blocks (see DECODE above) decodes all of them at once across the chip -- a block's
 *                   history is the output of the blocks before it -- and hands back the same results, status and
 *                   window as the walk of one wavefront that calls of many blocks run.
 * ------------------------------------------------------------------------------------------------------- */
typedef struct plz4hip_dict plz4hip_dict;
int  plz4hip_dict_create(plz4hip_ctx* ctx, const void* dict, int dictLen, plz4hip_dict** out);
void plz4hip_dict_destroy(plz4hip_ctx* ctx, plz4hip_dict* dict);

int plz4hip_compress_batch_dict(plz4hip_ctx* ctx, int nBlocks, const void* const* src, const int32_t* srcLen,
                                void* const* dst, const int32_t* dstCap, int level, const plz4hip_dict* dict, int32_t* result);
int plz4hip_decompress_batch_dict(plz4hip_ctx* ctx, int nBlocks, const void* const* src, const int32_t* srcLen,
                                  void* const* dst, const int32_t* dstCap, const plz4hip_dict* dict, int32_t* result);

int plz4hip_encode_records_ex(plz4hip_ctx* ctx, int nBlocks, const void* const* src, const int32_t* srcLen,
                              int bsz, int level, int blockChecksum, int linked, const plz4hip_dict* dict,
                              const void* prevTail, int prevTailLen, void* const* rec, int32_t* recLen);
int plz4hip_decode_records_ex(plz4hip_ctx* ctx, int nBlocks, const void* const* rec, const int32_t* recLen,
                              int bsz, int blockChecksum, int linked, const plz4hip_dict* dict,
                              void* window, int* windowLen, void* const* dst, int32_t* result, int32_t* status);
/* Linked decode of SEVERAL frames in one call.  The blocks of one linked frame are a serial chain ("replicas
 * only"), chains of different frames share nothing: chain k = records [chainFirst[k], chainFirst[k+1]) (chainFirst[0] == 0,
 * nChains + 1 entries): the few-block path over all chains at once, or (many blocks) one wavefront per chain.  windows = nChains x 64 KiB, windowLen[nChains]: the compress.DictT state of every
 * chain, in/out, exactly as `window` / `windowLen` of plz4hip_decode_records_ex(linked = 1); per-block result / status likewise
 * (a chain stops at its first bad block, the other chains go on).  No counterpart in the reference: a server that decodes
 * many linked frames (rdr.go:339-341 runs each one on a single goroutine) hands them over together. */
int plz4hip_decode_records_chains(plz4hip_ctx* ctx, int nChains, const int32_t* chainFirst,
                                  const void* const* rec, const int32_t* recLen, int bsz, int blockChecksum,
                                  void* windows, int32_t* windowLen, void* const* dst, int32_t* result, int32_t* status);

/* ---------------------------------------------------------------------------------------------------------
 * B''. Streaming content checksum on the device: xxh32.XXHZero (internal/pkg/xxh32/xxh32zero.go:58-86 Write, :204-235 Sum32)
 *    as the reference feeds it, block after block (async/hash.go:99-111, sync/writer.go:267-271, sync/reader.go:56).
 *    XXH32 has no combine operator: the stream is one serial chain, so this is ONE wavefront that runs beside the codec kernels
 *    (it is there to take the hash off the host's critical path, not to be fast: see DESIGN.md for its rate).
 *    create / reset: empty stream, seed 0.  sum: Sum32 of what was written so far (the stream goes on after it).
 *    update (host bytes) / dev_update (device bytes, enqueued on `stream` behind the stream's previous update).
 *    plz4hip_ctx_set_content_hash(ctx, h): while set (NULL clears it), every plz4hip_encode_records[_ex] call also writes the
 *    plaintext of its blocks, in block order, into h, and every plz4hip_decode_records[_ex] call the plaintext it produced
 *    (blocks whose result is <= 0 contribute nothing; the caller stops at the first bad block anyway) -- without the
 *    plaintext passing through the host again.  A stream is fed from one place at a time.
 * ------------------------------------------------------------------------------------------------------- */
typedef struct plz4hip_xxh32_stream plz4hip_xxh32_stream;
int  plz4hip_xxh32_stream_create(plz4hip_ctx* ctx, plz4hip_xxh32_stream** out);
void plz4hip_xxh32_stream_destroy(plz4hip_ctx* ctx, plz4hip_xxh32_stream* h);
int  plz4hip_xxh32_stream_reset(plz4hip_ctx* ctx, plz4hip_xxh32_stream* h);
int  plz4hip_xxh32_stream_update(plz4hip_ctx* ctx, plz4hip_xxh32_stream* h, const void* data, int64_t n);
int  plz4hip_dev_xxh32_stream_update(plz4hip_ctx* ctx, plz4hip_xxh32_stream* h, const void* devData, int64_t n, void* stream);
int  plz4hip_xxh32_stream_sum(plz4hip_ctx* ctx, plz4hip_xxh32_stream* h, uint32_t* out);
int  plz4hip_ctx_set_content_hash(plz4hip_ctx* ctx, plz4hip_xxh32_stream* h);

/* ---------------------------------------------------------------------------------------------------------
 * C. Device-resident pipeline (bench.py, GPU-to-GPU producers).  Every pointer below is a DEVICE pointer
 *    on ctx's device; work is enqueued on `stream` (a hipStream_t; NULL is HIP's default/null stream, as for any
 *    hip*Async call) and the call returns without synchronising.  Layout:
 *      src     plaintext, block i = src[i*bsz, min((i+1)*bsz, srcBytes))          nBlocks = ceil(srcBytes/bsz)
 *      stage   nBlocks records at stride plz4hip_dev_stage_stride(bsz)             (scratch)
 *      recLen  int32[nBlocks]   record i length (4 + payload + 4 if checksums)
 *      recOff  int64[nBlocks+1] exclusive prefix sum of recLen (recOff[nBlocks] = body bytes); the encoders write it, and
 *              plz4hip_dev_index_body reads it off a body that came from elsewhere
 *      body    the records, compacted back to back: exactly the frame's block section
 *    Decode (dev_decompress, dev_decode_records*, the decode side of dev_duplex_*), whatever the input holds: a call reads no
 *    byte outside the srcLen[i] bytes of a block / the recOff[i+1] - recOff[i] bytes of a record and the dictionary or the
 *    chain's window, and it writes no byte outside the dstCap bytes of that block's output (and the window).
 *    plz4hip_dev_decompress does not know the blocks' sizes on the host: the strides bound them.  With nBlocks == 1 strides of zero
 *    (or small ones) mean a block of at most 6 MiB in and 4 MiB + 8 out, as ever; a caller with ONE block above that passes
 *    srcStride >= its compressed length and dstStride >= its capacity, which send the call down the few-block path for large blocks
 *    (see DECODE above).  With several blocks a dstStride above 6 MiB does the same; up to there the call is what it was (4 MiB
 *    blocks at a padded stride), and a block above 4 MiB + 8 of capacity in it is one wavefront's.
 *    plz4hip_dev_encode_records  : the encode kernel; fills stage + recLen.
 *    plz4hip_dev_compact_records : exclusive scan of recLen -> recOff, then moves every record to body+recOff[i];
 *                                  records that would end past bodyCap are skipped (recOff[nBlocks] > bodyCap tells).
 *    plz4hip_dev_scatter_records : generic record mover, dst+dstOff[k] <- src+srcOff[k] (len[k] bytes); used by the
 *                                  multi-GPU frame assembly, where the owner rank interleaves the bodies it
 *                                  received from the other ranks (block i lives on rank i mod G).
 *    plz4hip_dev_decode_records reads records at body+recOff[i] and writes block i at dst + i*dstStride
 *    (capacity dstCap, bsz+8 in the reference); result/status as in B.
 * ------------------------------------------------------------------------------------------------------- */
int64_t plz4hip_dev_stage_stride(int bsz);

int plz4hip_dev_encode_records(plz4hip_ctx* ctx, const void* src, int64_t srcBytes, int bsz, int level,
                               int blockChecksum, void* stage, int32_t* recLen, void* stream);

int plz4hip_dev_compact_records(plz4hip_ctx* ctx, const void* stage, int64_t stageStride, const int32_t* recLen,
                                int nBlocks, int64_t* recOff, void* body, int64_t bodyCap, void* stream);

int plz4hip_dev_scatter_records(plz4hip_ctx* ctx, const void* src, const int64_t* srcOff, const int32_t* len,
                                const int64_t* dstOff, int n, int maxLen, void* dst, int64_t dstCap, void* stream);

int plz4hip_dev_decode_records(plz4hip_ctx* ctx, const void* body, const int64_t* recOff, int nBlocks,
                               int bsz, int blockChecksum, void* dst, int64_t dstStride, int dstCap,
                               int32_t* result, int32_t* status, void* stream);

/* plz4hip_dev_decode_records_ex: plz4hip_dev_decode_records for records with history outside the block -- what
 * plz4hip_decode_records_ex / plz4hip_decode_records_chains do over host buffers, for a consumer whose frame body is on the device.
 * linked = 0 with `dict`: independent blocks, every one against the dictionary, at any block count.  linked = 1 (dict NULL): the
 * call's blocks are the chains of chainFirst (a HOST array of nChains + 1 entries, chainFirst[0] == 0, non-decreasing, the last one
 * == nBlocks; it is not read after the call returns; NULL: one chain); windows / windowLen are DEVICE memory, in/out: 128 KiB per
 * chain -- the live window (compress.DictT) in the first 64 KiB, the rest scratch -- and int32[nChains]; as with
 * plz4hip_decode_records_ex the caller seeds a chain's window with the dictionary's last 64 KiB (or length 0).  Few blocks go
 * across the chip at once, a long chain in groups (see DECODE above).  Enqueued on `stream`, no synchronisation; it does not feed
 * plz4hip_ctx_set_content_hash (plz4hip_dev_xxh32_stream_update takes the plaintext where it lies). */
int plz4hip_dev_decode_records_ex(plz4hip_ctx* ctx, const void* body, const int64_t* recOff, int nBlocks,
                                  int bsz, int blockChecksum, int linked, const plz4hip_dict* dict,
                                  int nChains, const int32_t* chainFirst, void* windows, int32_t* windowLen,
                                  void* dst, int64_t dstStride, int dstCap, int32_t* result, int32_t* status, void* stream);

/* plz4hip_dev_index_body: recOff of a frame body that is ALREADY in device memory -- a file read there, a body received from
 * another GPU or node, the output of any other LZ4 writer -- for the record decoders above, which until here only this engine's own
 * encoders could feed.  It is the size-word walk of FrameReader._read (blk/frame.go:54-98) with that reader's checks, in place of a
 * host that chases the chain four bytes and one device-to-host copy per record.  The chain is serial, so the kernel is ONE wavefront
 * (no LDS, no workspace of the ctx; it runs beside any other launch, like the streaming checksum).  At every step, in this order:
 *     off == bodyBytes                                   PLZ4HIP_BODY_END_OF_BYTES   end = off   (a bare block section, as plz4hip_dev_encode_body writes it)
 *     bodyBytes - off < 4                                PLZ4HIP_BODY_TRUNCATED_WORD end = off   (zerr.ErrBlockSizeRead, frame.go:57-61)
 *     word == 0                                          PLZ4HIP_BODY_END_MARK       end = off + 4 (frame.go:71: where a content checksum or the next frame starts)
 *     i == maxBlocks                                     PLZ4HIP_BODY_FULL           end = off   (more records than the caller has room for)
 *     (word & 0x7FFFFFFF) > bsz                          PLZ4HIP_BODY_SIZE_OVERFLOW  end = off   (zerr.ErrBlockSizeOverflow, frame.go:79-81)
 *     4 + size + (blockChecksum ? 4 : 0) > bodyBytes-off PLZ4HIP_BODY_TRUNCATED_BLOCK end = off  (zerr.ErrBlockRead, frame.go:91-98)
 *     otherwise                                          recOff[i] = off; off += 4 + size (+ 4); ++i
 * 0x80000000 is a stored record of size 0 (descriptor/data.go:12), not an end mark: it is listed.  info->nBlocks = the records listed,
 * info->status = why the walk stopped, info->end as above; on EVERY exit recOff[nBlocks] is the end of the last listed record and
 * recOff[nBlocks + 1 .. maxBlocks] hold the same value.
 * Reads: the four bytes of a size word, and only where bodyBytes - off >= 4; never a payload byte, nothing outside
 * [body, body + bodyBytes).  Offsets are 64 bits wide and no size word overflows a test.  At most maxBlocks + 1 words are read.
 * Without a host synchronisation: the padded tail of recOff reads as zero-length records, which the record decoders answer with
 * PLZ4HIP_BLK_SIZE_OVERFLOW, result 0, and no byte written (in a linked chain the first of them does, and the chain's later records
 * are PLZ4HIP_BLK_CORRUPT, result 0, nothing written, as behind any bad block of a chain).  A caller that knows only an upper bound of the block count -- from the
 * header's content size, or bodyBytes / 5 + 1 -- enqueues this call and plz4hip_dev_decode_records[_ex] of maxBlocks records one
 * behind the other on one stream and reads info->nBlocks afterwards.
 * Enqueued on `stream`, no synchronisation.  body, recOff (maxBlocks + 1 entries) and info are device pointers.  PLZ4HIP_E_ARG: a null
 * pointer (body may be null when bodyBytes == 0), bodyBytes < 0, bsz <= 0, maxBlocks < 0 or > 0x7FFFFFFE.  Headers and trailers stay
 * on the host: `body` starts at the first record (plz4hip_dev_index_stream below takes headers, trailers and several frames). */
enum {
    PLZ4HIP_BODY_END_MARK        = 0,
    PLZ4HIP_BODY_END_OF_BYTES    = 1,
    PLZ4HIP_BODY_FULL            = 2,
    PLZ4HIP_BODY_SIZE_OVERFLOW   = 3,
    PLZ4HIP_BODY_TRUNCATED_WORD  = 4,
    PLZ4HIP_BODY_TRUNCATED_BLOCK = 5
};
typedef struct { int64_t end; int32_t nBlocks; int32_t status; } plz4hip_body_index;

int plz4hip_dev_index_body(plz4hip_ctx* ctx, const void* body, int64_t bodyBytes, int bsz, int blockChecksum,
                           int maxBlocks, int64_t* recOff /* device, maxBlocks + 1 */,
                           plz4hip_body_index* info /* device */, void* stream);

/* plz4hip_dev_index_stream: the index of a WHOLE LZ4 stream that is already in device memory -- any number of frames back to back,
 * skippable frames among them: an appended log, the output of `cat a.lz4 b.lz4`, a file with a seek table.  It is the reader's whole
 * header-mode / body-mode walk (rdr/rdr.go:242-296, header/read.go:26-119, header/skip.go:38-76, blk/frame.go:54-139) as ONE
 * wavefront (no LDS, no workspace of the ctx), in place of a host that copies every header back, calls plz4hip_dev_index_body, waits
 * for its end and copies the trailer back, frame after frame.  It writes a table of frames with their descriptors (skippable frames
 * listed with where their payload lies -- what the reference offers its skip callback), and ONE recOff for every record of the stream,
 * as offsets from `bytes`.  At every frame start `off`, in this order (hdr[k]: the byte at off + k):
 *     off == nBytes                                      PLZ4HIP_STREAM_END               end = off   (the reader's clean io.EOF)
 *     nFrames == maxFrames                               PLZ4HIP_STREAM_FRAMES_FULL       end = off   (something follows, and the table is full)
 *     nBytes - off < 7                                   PLZ4HIP_STREAM_HEADER_READ       end = off   (zerr.ErrHeaderRead)
 *     LE32 hdr[0..3] is 0x184D2A50 .. 0x184D2A5F         a skippable frame, size = LE32 hdr[4..7]:
 *         nBytes - off < 8                               PLZ4HIP_STREAM_HEADER_READ       end = off
 *         size > nBytes - off - 8                        PLZ4HIP_STREAM_SKIP              end = off   (zerr.ErrSkip)
 *         otherwise                                      list it: kind 1, nibble = magic & 15, bodyOff = off + 8, contentSz = size,
 *                                                        end = off + 8 + size, firstRec = the records listed so far, nRecs 0, bsz 0,
 *                                                        status PLZ4HIP_BODY_END_MARK; off = end; next frame
 *     hdr[0..3] is not 04 22 4D 18                       PLZ4HIP_STREAM_MAGIC             end = off   (zerr.ErrMagic)
 *     FLG = hdr[4]: (FLG >> 6) != 1                      PLZ4HIP_STREAM_VERSION           end = off   (zerr.ErrVersion)
 *     FLG & 2                                            PLZ4HIP_STREAM_RESERVED_BIT      end = off   (zerr.ErrReserveBitSet)
 *     BD = hdr[5]: id = (BD >> 4) & 7 < 4, BD & 0x80 or BD & 0x0F
 *                                                        PLZ4HIP_STREAM_BLOCK_DESCRIPTOR  end = off   (zerr.ErrBlockDescriptor)
 *     len = 7 + (FLG & 8 ? 8 : 0) + (FLG & 1 ? 4 : 0) > nBytes - off
 *                                                        PLZ4HIP_STREAM_HEADER_READ       end = off
 *     hdr[len - 1] != (xxh32 of hdr[4 .. len - 2], seed 0) >> 8 & 0xFF
 *                                                        PLZ4HIP_STREAM_HEADER_HASH       end = off   (zerr.ErrHeaderHash)
 *     otherwise                                          list the frame: hdrOff = off, bodyOff = off + len, flags = FLG, blockDesc = BD,
 *                                                        bsz = 64 KiB << 2 * (id - 4), contentSz = LE64 hdr[6..13] with FLG & 8,
 *                                                        dictId = LE32 hdr[len - 5 .. len - 2] with FLG & 1, firstRec = the records
 *                                                        listed so far; then the walk of plz4hip_dev_index_body from bodyOff, with that
 *                                                        bsz, block checksums = FLG & 16 and the stream's end as the body's, its checks
 *                                                        in its order, but off == nBytes inside a frame is PLZ4HIP_BODY_TRUNCATED_WORD
 *                                                        (the reference: zerr.ErrBlockSizeRead; a stream has no bare block section),
 *                                                        and `full` is the stream-wide count of records reaching maxRecs.
 *                                                        The entry's status is the walk's, its end the walk's, nRecs what it listed.
 *       the walk stopped with PLZ4HIP_BODY_END_MARK      FLG & 4: fewer than 4 bytes behind the end mark is
 *                                                        PLZ4HIP_STREAM_CONTENT_HASH_READ (zerr.ErrContentHashRead; the frame stays listed,
 *                                                        status PLZ4HIP_BODY_END_MARK, end behind the end mark), end = the entry's end;
 *                                                        else contentSum = that LE32 and the entry's end is behind it.
 *                                                        off = the entry's end; next frame
 *       with PLZ4HIP_BODY_FULL                           PLZ4HIP_STREAM_RECORDS_FULL      end = the entry's end (the record that found no room)
 *       with any other status                            PLZ4HIP_STREAM_BODY              end = the entry's end
 * On EVERY exit info is written (nFrames counts the skippable entries too, nSkippable those alone; maxBsz, flagsAnd and flagsOr run
 * over the LZ4 frames listed, all 0 when there is none; pad is 0); frames[0 .. nFrames) are written and the entries behind them are
 * not touched; recOff[0 .. nRecs) are the records' offsets from `bytes` and recOff[nRecs .. maxRecs] hold the end of the last listed
 * record (0 if there is none): the padding the record decoders answer with PLZ4HIP_BLK_SIZE_OVERFLOW, result 0, nothing written.
 * Reads: header bytes, size words and content-checksum words, each only where the remaining length holds it; never a payload byte
 * (a skippable frame's included), nothing outside [bytes, bytes + nBytes).  Every comparison is `need > nBytes - off` in 64 bits.
 * Without a host synchronisation: the record decoders take a record's payload size from its size word and recOff[i + 1] - recOff[i]
 * only as an upper bound, so the global recOff decodes although a frame's last record is followed by the end mark, the trailer and the
 * next header before the next entry.  A caller that knows the stream's options (bsz, block checksums) passes upper bounds --
 * nBytes / 5 + 1 records; nBytes / 7 + 1 table entries (7: the shortest header; nBytes / 8 + 1 where only skippable frames are
 * short) -- and enqueues this call and ONE plz4hip_dev_decode_records over bytes, recOff and maxRecs records for all frames on the
 * same stream, and reads info afterwards: flagsAnd, flagsOr and maxBsz tell whether the options it assumed held for every frame.
 * Linked frames (FLG bit 5 clear) need the entries' firstRec on the host, as chainFirst of plz4hip_dev_decode_records_ex; a dictionary
 * id is the caller's to resolve.  Content size and content checksum are listed, not verified: plz4hip_dev_verify_frames below does
 * that for all frames at once, behind the decode.
 * Enqueued on `stream`, no synchronisation.  bytes, frames (maxFrames entries), recOff (maxRecs + 1 entries) and info are device
 * pointers.  PLZ4HIP_E_ARG: a null pointer (bytes may be null when nBytes == 0, frames when maxFrames == 0), nBytes < 0,
 * maxFrames < 0, maxRecs < 0 or > 0x7FFFFFFE. */
enum {                                   /* why the stream walk stopped */
    PLZ4HIP_STREAM_END               = 0,
    PLZ4HIP_STREAM_FRAMES_FULL       = 1,
    PLZ4HIP_STREAM_RECORDS_FULL      = 2,  /* the frame is listed, status PLZ4HIP_BODY_FULL */
    PLZ4HIP_STREAM_HEADER_READ       = 3,
    PLZ4HIP_STREAM_MAGIC             = 4,
    PLZ4HIP_STREAM_VERSION           = 5,
    PLZ4HIP_STREAM_RESERVED_BIT      = 6,
    PLZ4HIP_STREAM_BLOCK_DESCRIPTOR  = 7,
    PLZ4HIP_STREAM_HEADER_HASH       = 8,
    PLZ4HIP_STREAM_SKIP              = 9,
    PLZ4HIP_STREAM_BODY              = 10, /* the last listed frame's walk did not reach an end mark: its status says why */
    PLZ4HIP_STREAM_CONTENT_HASH_READ = 11
};
typedef struct {                         /* 64 bytes */
    int64_t  hdrOff;      /* the magic */
    int64_t  bodyOff;     /* the first record; skippable: the payload */
    int64_t  end;         /* complete frame: first byte behind end mark and content checksum; else where its walk stopped; skippable: behind the payload */
    uint64_t contentSz;   /* FLG bit 3, else 0; skippable: the payload's size */
    uint32_t dictId;      /* FLG bit 0, else 0 */
    uint32_t contentSum;  /* the stored content checksum, FLG bit 2, else 0 */
    int32_t  firstRec;    /* index of its first record in recOff */
    int32_t  nRecs;
    int32_t  bsz;         /* 64 KiB << 2 * (BD id - 4); skippable: 0 */
    uint8_t  flags, blockDesc, kind /* 0 LZ4 frame, 1 skippable */, nibble /* skippable: magic & 15 */;
    int32_t  status;      /* PLZ4HIP_BODY_* of its walk; PLZ4HIP_BODY_END_MARK: complete (skippable: always that) */
    int32_t  reserved;    /* 0 */
} plz4hip_frame_index;
typedef struct {                         /* 32 bytes */
    int64_t end; int32_t nFrames /* table entries, skippable included */; int32_t nRecs; int32_t status; int32_t nSkippable;
    int32_t maxBsz; uint8_t flagsAnd, flagsOr /* over the LZ4 frames listed; both 0 when there is none */; uint8_t pad[2];
} plz4hip_stream_index;

int plz4hip_dev_index_stream(plz4hip_ctx* ctx, const void* bytes, int64_t nBytes, int maxFrames, int maxRecs,
                             plz4hip_frame_index* frames /* device, maxFrames */, int64_t* recOff /* device, maxRecs + 1 */,
                             plz4hip_stream_index* info /* device */, void* stream);

/* plz4hip_dev_verify_frames: the verdict on EVERY frame of a stream that plz4hip_dev_index_stream listed and one
 * plz4hip_dev_decode_records[_ex] over the global recOff decoded -- what the reference's reader checks before it reads the next header:
 * every block decoded, the plaintext hashes to the stored content checksum (zerr.ErrContentHash, async/reader.go:236-241,
 * sync/reader.go:56-67), and there is as much of it as the header promised (zerr.ErrContentSize, rdr/rdr.go:91-101).  It completes
 * index -> decode -> verify on one stream without a host in between: the host reads info, sv and, where sv names a bad frame, that
 * frame's verdict.  dst, dstStride, dstCap, result, status and maxRecs are those of the ONE record decode (record i left result[i] bytes
 * at dst + i * dstStride); which decoder ran does not matter.  nFrames = info->nFrames, read on the device and clamped to
 * [0, maxFrames].  For every frame f < nFrames, in this order:
 *     kind == 1                                          PLZ4HIP_FRAME_SKIPPABLE     all other fields 0, nothing read
 *     firstRec < 0, nRecs < 0 or firstRec + nRecs > maxRecs (64 bits)
 *                                                        PLZ4HIP_FRAME_RANGE         firstBad = -1, nothing read
 *     records i = firstRec .. firstRec + nRecs - 1, in order:
 *         status[i] != PLZ4HIP_BLK_OK                    PLZ4HIP_FRAME_BLOCK         firstBad = i, blockStatus = status[i]; stop
 *         result[i] < 0 or > dstCap                      PLZ4HIP_FRAME_RANGE         firstBad = i; stop
 *         otherwise                                      contentSz += result[i]; where the entry's status is PLZ4HIP_BODY_END_MARK and
 *                                                        FLG & 4, those bytes go into the frame's hash
 *     the entry's status != PLZ4HIP_BODY_END_MARK        PLZ4HIP_FRAME_INCOMPLETE    (the index stopped inside this frame)
 *     FLG & 4 and the sum differs from the entry's contentSum
 *                                                        PLZ4HIP_FRAME_CONTENT_HASH
 *     FLG & 8 and contentSz differs from the entry's contentSz
 *                                                        PLZ4HIP_FRAME_CONTENT_SIZE
 *     otherwise                                          PLZ4HIP_FRAME_OK
 * Hash before size is the reference's order (NextBlock turns the end mark into ErrContentHash before handleEndMark runs).
 * contentSz is always the bytes counted before the walk stopped; contentSum is the xxh32 (seed 0) of exactly those bytes whenever
 * the entry is an LZ4 frame that is complete and stores a checksum (status PLZ4HIP_BODY_END_MARK, FLG & 4), whatever the verdict
 * -- of no bytes where the walk never started -- and 0 otherwise; firstBad = -1 and blockStatus = 0 where no record stopped the
 * walk; reserved is 0.  verdicts[nFrames .. maxFrames) are not touched.
 * Reads: info->nFrames; frames[0 .. nFrames); status[i] and result[i] of the listed records up to the first bad one; the first
 * result[i] bytes at dst + i * dstStride, only for frames that are hashed and only after that result[i] passed its range check.
 * Nothing else.
 * The stream verdict sv is written on every exit: nFrames = the clamped count; nSkippable and nOk count over the table;
 * firstBadFrame = the lowest f whose verdict is neither OK nor SKIPPABLE, or -1, and status = that frame's (or 0); contentBytes = the
 * sum of contentSz over the frames before it plus its own -- the plaintext a reader delivers before it errors -- and with no bad frame
 * the sum over all frames.  info->status of the index stays the caller's to read: a walk that stopped at a bad header is not this
 * call's business.
 * The kernels: sixteen frames per wavefront, four lanes a frame (a frame's xxh32 is four serial chains: there is no combine
 * operator), one-wave workgroups that stride over the table -- at most ceil(maxFrames / 16) of them and at most
 * plz4hip_dev_resident_waves(ctx, 1), so a loose maxFrames such as nBytes / 7 + 1 costs no empty launch -- then one wavefront that
 * folds the verdicts into sv.  No LDS, no workspace of the ctx, no atomics.  Known limit: one frame is one chain, so a stream of few
 * huge frames is verified at one chain's rate per frame, and the sixteen frames of a wave finish with its longest.
 * Enqueued on `stream`, no synchronisation.  Every pointer is a device pointer.  PLZ4HIP_E_ARG: a null pointer (frames and verdicts
 * may be null when maxFrames == 0, dst when maxFrames == 0 or maxRecs == 0), maxFrames < 0, maxRecs < 0 or > 0x7FFFFFFE, dstCap < 0,
 * dstStride < dstCap. */
enum {
    PLZ4HIP_FRAME_OK           = 0,
    PLZ4HIP_FRAME_SKIPPABLE    = 1,
    PLZ4HIP_FRAME_RANGE        = 2,  /* the table or a result points outside the decode's arrays */
    PLZ4HIP_FRAME_BLOCK        = 3,  /* a block did not decode: blockStatus is its PLZ4HIP_BLK_* */
    PLZ4HIP_FRAME_INCOMPLETE   = 4,
    PLZ4HIP_FRAME_CONTENT_HASH = 5,  /* zerr.ErrContentHash */
    PLZ4HIP_FRAME_CONTENT_SIZE = 6   /* zerr.ErrContentSize */
};
typedef struct {                         /* 32 bytes */
    uint64_t contentSz;   /* plaintext bytes counted */
    uint32_t contentSum;  /* their xxh32 where the frame is complete and stores one, else 0 */
    int32_t  status;      /* PLZ4HIP_FRAME_* */
    int32_t  firstBad;    /* stream-wide index of the record that stopped the walk, or -1 */
    int32_t  blockStatus; /* PLZ4HIP_FRAME_BLOCK: that record's status, else 0 */
    int32_t  reserved[2]; /* 0 */
} plz4hip_frame_verdict;
typedef struct {                         /* 32 bytes */
    int64_t contentBytes; int32_t firstBadFrame; int32_t status; int32_t nFrames; int32_t nOk; int32_t nSkippable; int32_t reserved;
} plz4hip_stream_verdict;

int plz4hip_dev_verify_frames(plz4hip_ctx* ctx, const plz4hip_frame_index* frames, const plz4hip_stream_index* info,
                              int maxFrames, const void* dst, int64_t dstStride, int dstCap,
                              const int32_t* result, const int32_t* status, int maxRecs,
                              plz4hip_frame_verdict* verdicts /* device, maxFrames */,
                              plz4hip_stream_verdict* sv /* device */, void* stream);

/* plz4hip_dev_write_frames: whole LZ4 frames around the block section an encode left in device memory -- the magic, FLG / BD, content
 * size, dictionary id and header checksum in front (header/write.go:23-73), the end mark and the content checksum behind
 * (trailer/trailer.go, blk/frame.go): bytes that any LZ4 reader and plz4hip_dev_index_stream open.  The dual of
 * plz4hip_dev_verify_frames.  Enqueued behind plz4hip_dev_encode_body[_ex], or behind plz4hip_dev_encode_records[_ex] +
 * plz4hip_dev_compact_records (levels 3..12), on the same stream: no host reads recOff in between.  One call writes a STREAM of frames
 * of blocksPerFrame blocks each: XXH32 has no combine operator, so a frame's content checksum is one serial chain, and the caller
 * trades checksum parallelism against header bytes with k = blocksPerFrame.
 * GEOMETRY (host arithmetic, 64 bits).  nBlocks = ceil(srcBytes / bsz) (above 0x7FFFFFFE: PLZ4HIP_E_ARG); block i is the
 * min(bsz, srcBytes - i * bsz) bytes at src + i * srcStride, the layout of plz4hip_dev_encode_records_ex.  nFrames = k ?
 * max(1, ceil(nBlocks / k)) : 1; frame f owns records [f * k, min((f + 1) * k, nBlocks)) (k == 0: all of them).  srcBytes == 0 is ONE
 * empty frame: header, end mark, the checksum of no bytes (0x02CC5D05) -- what the reference's synchronous writer emits on Close
 * (sync/writer.go:133-186); recOff is then not read and counts as recOff[0] = 0.
 * BYTES.  H = 7 + 8 * contentSize + 4 * hasDictId, T = 4 + 4 * contentChecksum.  Frame f starts at F(f) = f * (H + T) + recOff[f * k]:
 *     04 22 4D 18 | FLG = 0x40 | !linked << 5 | blockChecksum << 4 | contentSize << 3 | contentChecksum << 2 | hasDictId
 *     | BD = id << 4 (bsz 64 KiB << 2 * (id - 4)) | LE64 the FRAME's plaintext length | LE32 dictId | (xxh32(FLG .. dictId, seed 0) >> 8) & 0xFF
 *   then the frame's records unchanged, record i at outRecOff[i] = recOff[i] + (i / k + 1) * H + (i / k) * T (i / k = 0 when k == 0),
 *   then four zero bytes, then LE32 of the xxh32 (seed 0) of the frame's plaintext where contentChecksum is set.
 *   The stream's end E = nFrames * (H + T) + recOff[nBlocks].
 * CHECKS (on the device; every one is `need > have` in 64 bits).  In this order:
 *     recOff[nBlocks] outside [0, bodyBytes]                E is unknown: info.end = -1, no byte of `out` is written; the record
 *                                                           tests below run and name a record (the last one at least is bad)
 *     E > outCap                                            PLZ4HIP_WRITE_NO_ROOM: info.end = E, firstBadRec = -1; NO byte of out, frames
 *                                                           or outRecOff is written and nothing but recOff[nBlocks] is read
 *     record i, with a = recOff[i], b = recOff[i + 1]:
 *         a < 0, b < a or b > bodyBytes                     bad
 *         b - a < 4 + 4 * blockChecksum                     bad (a block the engine failed on takes no room; an overflowed body)
 *         w = the size word at body + a:
 *         (w & 0x7FFFFFFF) > bsz, or
 *         4 + (w & 0x7FFFFFFF) + 4 * blockChecksum != b - a bad
 *     any bad record                                        PLZ4HIP_WRITE_RECORD, firstBadRec = the lowest such i
 *     otherwise                                             PLZ4HIP_WRITE_OK: out[0 .. E) is the stream
 *   With PLZ4HIP_WRITE_RECORD the bytes inside [out, out + outCap) are unspecified (frames without a bad record that fit are written).
 * TABLES, so that the reader calls need no index pass: frames[f] is, field by field, what plz4hip_dev_index_stream lists for that
 * frame -- hdrOff = F(f), bodyOff = F(f) + H, end = F(f + 1); contentSz, dictId, contentSum each 0 where its flag is clear; firstRec,
 * nRecs, bsz, flags, blockDesc; kind 0, nibble 0, status PLZ4HIP_BODY_END_MARK, reserved 0.  A frame that holds a bad record has
 * status = -1 - (the index of its first bad record) instead (no PLZ4HIP_BODY_* is negative; plz4hip_dev_verify_frames answers it with
 * PLZ4HIP_FRAME_INCOMPLETE) and contentSum 0.  outRecOff[i] as above for every i < nBlocks, whatever record i is;
 * outRecOff[nBlocks] = the end of the last record, E - T (0 if there is none): the index's padding convention.
 * info is written on EVERY exit: end, nFrames and nRecs = nBlocks of the geometry, status, firstBadRec or -1, reserved 0.  Its end,
 * nFrames and nRecs lie where plz4hip_stream_index has them, so info serves as the `info` of plz4hip_dev_verify_frames (which reads
 * nFrames alone) behind ONE plz4hip_dev_decode_records over out, outRecOff and nBlocks records.  recOff[0] need not be 0: the stream
 * then starts at out + recOff[0], every offset above counts from `out`, and the bytes in front of it are not written.
 * Whatever the inputs hold, the call READS only recOff[0 .. nBlocks], size words of records that passed the range tests, record bytes
 * inside [body, body + bodyBytes) and, only when contentChecksum is set, plaintext bytes of blocks inside the srcBytes geometry (a
 * frame's blocks up to its first bad record); it WRITES nothing outside [out, out + outCap), frames[0 .. nFrames),
 * outRecOff[0 .. nBlocks] and info.
 * The call frames whatever records it is given: that a linked HC frame's records obey the stored-bit rule of B' stays the caller's
 * business, as does passing the blockChecksum, bsz and `linked` the records were encoded with.
 * The kernels: k_frame_edges, sixteen frames per wavefront and four lanes a frame as in plz4hip_dev_verify_frames, one-wave workgroups
 * that stride over the frames -- at most ceil(nFrames / 16) and at most plz4hip_dev_resident_waves(ctx, 1) of them; k_frame_move, one
 * pass over the records' bytes into their places; k_frame_summary, one wavefront that writes info.  No synchronisation, no
 * allocation, no workspace of the ctx, no LDS, no atomics, nothing on the NULL stream.  Known limit: one frame is one chain of about
 * 1 GB/s; k = 0 with contentChecksum over a large input is that chain alone.
 * Every pointer but opts is a device pointer.  PLZ4HIP_E_ARG: a null pointer (src may be null when contentChecksum == 0 or
 * srcBytes == 0, body when bodyBytes == 0), a negative size, bodyBytes or outCap above 2^62, a bsz that is not one of the four, a
 * srcStride that is neither bsz nor >= bsz + 65536, blocksPerFrame < 0, linked with blocksPerFrame != 0, reserved != 0. */
typedef struct {                         /* host, by value: what every frame of the call has in common */
    int32_t  bsz;             /* 65536, 262144, 1048576 or 4194304 (BD id 4 .. 7) */
    int32_t  blockChecksum;   /* FLG bit 4: what the records were encoded with */
    int32_t  linked;          /* FLG bit 5 CLEAR; only with blocksPerFrame == 0 */
    int32_t  contentChecksum; /* FLG bit 2 */
    int32_t  contentSize;     /* FLG bit 3: every header carries its own frame's plaintext length */
    int32_t  hasDictId;       /* FLG bit 0 */
    uint32_t dictId;
    int32_t  reserved;        /* 0 */
} plz4hip_frame_opts;
enum { PLZ4HIP_WRITE_OK = 0, PLZ4HIP_WRITE_NO_ROOM = 1, PLZ4HIP_WRITE_RECORD = 2 };
typedef struct {                         /* 32 bytes */
    int64_t end;              /* bytes of the stream: what `out` needs; -1 where recOff[nBlocks] lies outside the body */
    int32_t nFrames; int32_t nRecs; int32_t status /* PLZ4HIP_WRITE_* */; int32_t firstBadRec /* or -1 */;
    int32_t reserved[2];      /* 0 */
} plz4hip_write_info;

int plz4hip_dev_write_frames(plz4hip_ctx* ctx, const plz4hip_frame_opts* opts,
                             const void* src, int64_t srcBytes, int64_t srcStride,
                             const void* body, int64_t bodyBytes, const int64_t* recOff /* device, nBlocks + 1 */,
                             int blocksPerFrame, void* out, int64_t outCap,
                             plz4hip_frame_index* frames /* device, nFrames */, int64_t* outRecOff /* device, nBlocks + 1 */,
                             plz4hip_write_info* info /* device */, void* stream);

/* plz4hip_dev_duplex_records: plz4hip_dev_encode_records (level 1) of one batch AND plz4hip_dev_decode_records of another --
 * a writer's next batch and a reader's -- enqueued as one call, with results identical to the two calls made one after the
 * other; the operands of the two sides must not overlap.  The reference runs its compress and decompress workers side by side
 * on the host's cores (async/writer.go:232-282, async/reader.go:192-221); here the decoder's waves share every CU with the
 * level-1 parser's (k_l1_duplex): the parser is a serial chain per block that leaves about half of the vector issue slots
 * idle, the decoder is bound by those slots, so the decode costs the pair little more than the parse alone.  Either side may be
 * empty (srcBytes == 0 / nDecBlocks == 0). */
int plz4hip_dev_duplex_records(plz4hip_ctx* ctx, const void* src, int64_t srcBytes, int bsz, int blockChecksum, void* stage, int32_t* recLen,
                               const void* body, const int64_t* recOff, int nDecBlocks, int decBsz, int decBlockChecksum,
                               void* dst, int64_t dstStride, int dstCap, int32_t* result, int32_t* status, void* stream);

/* plz4hip_dev_encode_body: plz4hip_dev_encode_records + plz4hip_dev_compact_records in one call, without the staging area and
 * without the second pass over the records -- blk.CompressToBlk (blk/blk.go:69-109) for every block and the writer's in-order
 * emission (async/writer.go:284-381) as ONE contiguous frame body: record i lands at body + recOff[i], recOff[nBlocks] = the body's
 * length, recLen[i] = record i's bytes (a negative PLZ4HIP_E_* for a block the engine failed on; it takes no room).  The emit stage
 * knows every record's length before it writes a byte, so the records' places come from a scan between its passes.  Levels 1
 * and 2, blocks up to 4 MiB (the staged call; PLZ4HIP_E_NOMEM if its workspace cannot be had).  recOff[nBlocks] > bodyCap: the
 * records beyond the room were not written.  plz4hip_dev_duplex_body: the same with the record decode of another batch in the
 * same launch, as plz4hip_dev_duplex_records. */
int plz4hip_dev_encode_body(plz4hip_ctx* ctx, const void* src, int64_t srcBytes, int bsz, int level, int blockChecksum,
                            void* body, int64_t bodyCap, int64_t* recOff, int32_t* recLen, void* stream);
int plz4hip_dev_duplex_body(plz4hip_ctx* ctx, const void* src, int64_t srcBytes, int bsz, int blockChecksum,
                            void* body, int64_t bodyCap, int64_t* recOff, int32_t* recLen,
                            const void* decBody, const int64_t* decRecOff, int nDecBlocks, int decBsz, int decBlockChecksum,
                            void* dst, int64_t dstStride, int dstCap, int32_t* result, int32_t* status, void* stream);

/* plz4hip_dev_encode_records_ex / plz4hip_dev_encode_body_ex: plz4hip_dev_encode_records / plz4hip_dev_encode_body for blocks with
 * history outside the block -- what plz4hip_encode_records_ex does over host buffers (WithBlockLinked, WithDictionary; BASELINE
 * config 5), for a producer whose plaintext is on the device.  Enqueued on `stream`, no synchronisation; every pointer is a device
 * pointer.  Block i = src + i*srcStride, nBlocks = ceil(srcBytes / bsz), the last block is short.  srcStride == bsz: contiguous
 * plaintext; srcStride >= bsz + 65536: gapped, 64 KiB of caller-owned scratch in front of every block; anything else: PLZ4HIP_E_ARG.
 * `linked`, `dict`, prevTail / prevTailLen mean what they mean in plz4hip_encode_records_ex and prime a block exactly as there
 * (prevTail is a device pointer; prevTailLen < 0: none, block 0 starts the frame; > 65536: PLZ4HIP_E_ARG).  prevTail either ends
 * exactly at src or does not overlap [src - prevTailLen, src), where it is laid; anything else: PLZ4HIP_E_ARG.
 * THE SEGMENT RULE.  The kernels read a block's external segment -- the previous block's last <= 64 KiB, prevTail, or the dictionary --
 * immediately in front of the block.  Where the segment a block needs is not already the bytes lying there, the 64 KiB in front of
 * that block must be writable scratch of the caller, and the engine lays the segment there:
 *   linked = 1, contiguous : block i > 0 finds block i-1's tail in front of it: nothing is copied.  Only block 0 can need the
 *                            scratch (src - 65536 .. src), for the dictionary or prevTail; when prevTail == src - prevTailLen -- a
 *                            later call that continues one big buffer -- nothing is copied and nothing is written.
 *   linked = 1, gapped     : every block's tail is copied from its predecessor into the block's gap.
 *   linked = 0 with dict   : every block is against the dictionary; needs the gapped stride (contiguous: PLZ4HIP_E_ARG).
 *   linked = 0, no dict    : PLZ4HIP_E_ARG (plz4hip_dev_encode_records / plz4hip_dev_encode_body).
 * Outside those scratch regions the call writes no byte of src.
 * Levels 1..12 (records_ex; levels 2..12 are the HC designs over segment + block, as in B'); body_ex takes levels 1 and 2 like
 * plz4hip_dev_encode_body (level 2 with a block <= 4 KiB that starts under an attached dictionary of any length, which the
 * one-thread parser writes as a staged record: PLZ4HIP_E_UNSUPPORTED, use records_ex + plz4hip_dev_compact_records).    A block that does not fit comes back as a stored record; the note in B' about the reference's
 * linked HC writer applies unchanged.  These calls do not feed plz4hip_ctx_set_content_hash (plz4hip_dev_xxh32_stream_update takes
 * the plaintext where it lies).
 * Level 1: a call of few blocks (see ENCODE above) is cut across the chip like the host-buffer call.  A call of more blocks runs the
 * staged design with one wavefront per block -- each block one exact run of the parser behind its segment, the table liblz4 starts
 * the block with built in the wavefront's own LDS table, then the data-parallel emit stage; it keeps the level-1 workspace (2.25
 * bytes per input byte of a group of blocks, like the independent call).  PLZ4HIP_L1X=0 (read per call), PLZ4HIP_L1_FUSED or a
 * workspace that cannot be had: the one-kernel encoder of plz4hip_encode_records_ex instead (body_ex then stages its records in a
 * buffer of the ctx's, nBlocks x plz4hip_dev_stage_stride(bsz), until plz4hip_ctx_trim; a refused workspace there: PLZ4HIP_E_NOMEM).
 * The staged design is the default for many blocks: on linked 4 MiB blocks of text behind a 64 KiB dictionary body_ex takes 77 ms
 * at 512 blocks and 256 ms at 6144 (94 GiB/s), the one-kernel encoder 154 and 461 ms, plz4hip_dev_encode_body on the same bytes as
 * independent blocks 76 and 250 ms (profiles/l1x_rate.json, scripts/l1x_rate.py). */
int plz4hip_dev_encode_records_ex(plz4hip_ctx* ctx, const void* src, int64_t srcBytes, int64_t srcStride, int bsz, int level,
                                  int blockChecksum, int linked, const plz4hip_dict* dict, const void* prevTail, int prevTailLen,
                                  void* stage, int32_t* recLen, void* stream);
int plz4hip_dev_encode_body_ex(plz4hip_ctx* ctx, const void* src, int64_t srcBytes, int64_t srcStride, int bsz, int level,
                               int blockChecksum, int linked, const plz4hip_dict* dict, const void* prevTail, int prevTailLen,
                               void* body, int64_t bodyCap, int64_t* recOff, int32_t* recLen, void* stream);

/* Raw LZ4 blocks on the device (no record framing): block i = src + i*srcStride (srcLen[i] bytes) ->
 * dst + i*dstStride (capacity dstCap[i]); result[i] as in A, levels 1..12.  srcLen/dstCap/result are device arrays.
 * Whatever result[i] is, the call writes no byte of dst outside the dstCap[i] bytes at dst + i*dstStride (the rest of a stride
 * wider than the capacity is left as it was), and none of src.
 * maxLen is a host value the per-block workspaces are sized from, at EVERY level: it must be >= every srcLen[i]; a block whose
 * device-side length is outside [0, maxLen] is not touched and gets result[i] = PLZ4HIP_E_ARG (its neighbours are unaffected).
 * maxLen <= 0 means "unknown to the host": allowed at level 1 only, where it selects the one-kernel encoder that needs no
 * workspace (levels 2..12 return PLZ4HIP_E_ARG for the call).  A level-1 caller with a loose or stale positive maxLen therefore
 * gets per-block errors, not slower output: pass 0 rather than a guess.
 * The staged level-1 call and the HC levels (here and in plz4hip_dev_encode_records) work in per-ctx workspaces and read a
 * per-ctx sanitised copy of srcLen: jobs enqueued on different streams of one ctx are ordered behind each other on the device
 * (an event wait, no host block); they never overlap.  The exception is the staged level-1 call on device-resident records
 * (plz4hip_dev_encode_records / _encode_body / _duplex_records / _duplex_body): a ctx keeps two record workspaces, so calls that
 * alternate over two streams overlap -- behind a call that fills the chip (>= 8 blocks per CU) the parse launch of the later call
 * waits on the device until the earlier one has handed out its last block, then moves in as that one's workgroups leave, and the
 * earlier call's emit kernels run beside it (bench.py --pipelines: + 10 % over one stream).
 * The library never issues work on the NULL stream (its own small copies and memsets run on a stream of the ctx): a process that
 * does not use the NULL stream itself keeps all four hardware queues for the streams it passes in and the staging slots. */
int plz4hip_dev_compress(plz4hip_ctx* ctx, int nBlocks, const void* src, int64_t srcStride, const int32_t* srcLen,
                         void* dst, int64_t dstStride, const int32_t* dstCap, int level, int maxLen, int32_t* result, void* stream);
int plz4hip_dev_decompress(plz4hip_ctx* ctx, int nBlocks, const void* src, int64_t srcStride, const int32_t* srcLen,
                           void* dst, int64_t dstStride, const int32_t* dstCap, int32_t* result, void* stream);

/* Number of waves the encode / decode kernels keep resident on ctx's device (for sizing batches). */
int plz4hip_dev_resident_waves(plz4hip_ctx* ctx, int decode);

/* ---------------------------------------------------------------------------------------------------------
 * D. Several GPUs of one node behind one handle (BASELINE.json north_star: independent blocks shard round-robin).
 *    The reference spreads the blocks of a stream over NParallel worker goroutines and emits their records in order
 *    (async/writer.go:232-282 compressLoop, :284-381 writeLoop, :439-467 kickoffAsync); here the workers are the GPUs:
 *    block i of a call belongs to device i mod G, G = the number of entries passed to plz4hip_mgpu_create (one plz4hip_ctx
 *    each; the same device may be listed more than once).  Results come back in block order; value semantics as in A / B.
 *    Host buffers (what the cgo shim binds): one host thread per device drives that device's ctx.
 *    Device-resident shards (GPU producers, bench): shard k is ONE buffer on device k holding blocks k, k+G, ... back to back.
 *      dev_encode_frame: every device encodes + compacts its shard; record sizes go to the host, one prefix sum gives the
 *        frame offsets (recOff, host, nBlocks+1 entries), and the frame body is assembled on device `owner` (an index into
 *        the handle's devices): the other devices' records arrive peer to peer in pieces of <= 256 MiB through two scratch
 *        buffers and are moved to their place while the next piece travels -- the owner holds the body + two pieces.
 *      dev_decode_frame: the reverse: records are dealt from `owner` to the devices, each decodes its shard into shardDst[k]
 *        (block j of shard k at shardDst[k] + j*dstStride).
 *    Linked decode does not shard (one serial chain per frame): use plz4hip_decode_records_chains per device.
 * ------------------------------------------------------------------------------------------------------- */
typedef struct plz4hip_mgpu plz4hip_mgpu;
int          plz4hip_mgpu_create(const int* devices, int nDevices, plz4hip_mgpu** out);
void         plz4hip_mgpu_destroy(plz4hip_mgpu* m);
int          plz4hip_mgpu_count(const plz4hip_mgpu* m);
plz4hip_ctx* plz4hip_mgpu_ctx(plz4hip_mgpu* m, int k);                /* the k-th device's ctx (dictionaries, trims, ...) */
const char*  plz4hip_mgpu_last_error(const plz4hip_mgpu* m);

int plz4hip_mgpu_compress_batch(plz4hip_mgpu* m, int nBlocks, const void* const* src, const int32_t* srcLen,
                                void* const* dst, const int32_t* dstCap, int level, int32_t* result);
int plz4hip_mgpu_decompress_batch(plz4hip_mgpu* m, int nBlocks, const void* const* src, const int32_t* srcLen,
                                  void* const* dst, const int32_t* dstCap, int32_t* result);
int plz4hip_mgpu_encode_records(plz4hip_mgpu* m, int nBlocks, const void* const* src, const int32_t* srcLen,
                                int bsz, int level, int blockChecksum, void* const* rec, int32_t* recLen);
int plz4hip_mgpu_decode_records(plz4hip_mgpu* m, int nBlocks, const void* const* rec, const int32_t* recLen,
                                int bsz, int blockChecksum, void* const* dst, int32_t* result, int32_t* status);

int plz4hip_mgpu_dev_encode_frame(plz4hip_mgpu* m, int nBlocks, const void* const* shardSrc, const int64_t* shardBytes,
                                  int bsz, int level, int blockChecksum, int owner, void* body, int64_t bodyCap,
                                  int64_t* recOff, int64_t* bodyBytes);
int plz4hip_mgpu_dev_decode_frame(plz4hip_mgpu* m, int nBlocks, int owner, const void* body, const int64_t* recOff,
                                  int bsz, int blockChecksum, void* const* shardDst, int64_t dstStride, int dstCap,
                                  int32_t* result, int32_t* status);
/* plz4hip_mgpu_dev_index_frame: plz4hip_dev_index_body of a frame body on device `owner`, for a caller that holds only the body's
 * bytes: the walk of FrameReader._read (blk/frame.go:54-98) on the owner's ctx and stream, then one copy back each for recOff
 * (HOST, maxBlocks + 1 entries) and info (HOST).  Synchronous.  The caller hands info->nBlocks and recOff to
 * plz4hip_mgpu_dev_decode_frame, whose own check of every record's length stays as it is.  A damaged size word is a status in
 * info, not an error of the call. */
int plz4hip_mgpu_dev_index_frame(plz4hip_mgpu* m, int owner, const void* body, int64_t bodyBytes, int bsz, int blockChecksum,
                                 int maxBlocks, int64_t* recOff /* host, maxBlocks + 1 */, plz4hip_body_index* info /* host */);

#ifdef __cplusplus
}
#endif
#endif /* PLZ4HIP_H */
