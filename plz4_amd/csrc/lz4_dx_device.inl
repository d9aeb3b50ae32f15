// lz4_dx_device.inl -- LZ4_decompress_safe (/root/reference/internal/pkg/clz4/lz4.c:2022-2445) for a FEW blocks, cut across the
// whole chip.  The record decoder of lz4_device.inl is one wavefront per block: a 4 MiB block is 75 ms of one wave whatever else
// the chip does, which is what plz4.DecompressBlock (plz4_block.go:131-172) or a reader with a handful of blocks in flight would
// pay.  A block's decode is a chain twice over -- the token chain (where a sequence starts is only known once the one before it is
// parsed) and the copy chain (a match copies bytes an earlier match produced) -- and both are cut here the way a GPU cuts chains:
// by pointer jumping.
//
//   A  dx_segment_table  one wave per 8 KiB of INPUT: for every byte position p of the segment, as if a sequence started there,
//                        where the token chain from p leaves the segment and how many output bytes it passes (64 positions at a
//                        time, from the segment's end backwards: five doubling rounds inside the batch, one table lookup behind it).
//   B  dx_stitch         one wave per block: the true chain's entry into every segment and the output position there, one table
//                        lookup per segment (a sequence the tables could not tell -- length bytes without end -- is parsed here).
//   C  wave_dx_fill      one wave per segment again, now on the TRUE chain: literals go to their place in the output; a match
//                        is not copied -- its source may not exist yet -- but written down as pointers, ptr[o + i] = o + i - offset,
//                        into a table that starts as the identity.  The reference's accept / reject rules are walked as they are
//                        (fast loop in the middle of a block; the last two segments as one unit with the safe loop's rules): whatever
//                        they would not let pass flags the block, and a flagged block is decoded again by the one-wave decoder,
//                        whose result and error code are the reference's by construction.
//   D  dx_jump           ptr[p] <- ptr[ptr[p]] over every output byte, in place, until nothing moves (log2 of the deepest copy
//                        chain: 8-12 rounds on text, 22 on a 4 MiB run of one byte): every byte then points at the literal it is.
//   E  dx_gather         out[p] <- out[ptr[p]].
//
// Raw blocks above kDxMaxOut (up to 1 GiB) take the same stages with B cut once more, long runs handed to the whole grid and more
// jump rounds: dxb_* below.  Blocks with history outside the block share one pointer space: dxl_* below.
//
// THE STAGE TRAIN, stated once (the dx_stage_* bodies at the end of this file; the kernels of plz4hip.hip are shells over them and
// tests/emu/dx_train.h runs the same bodies on the CPU).  A call of nb blocks, its workspace laid out for blocks of up to maxIn input
// and maxOut output bytes (ws_layout.h: per block a row of T, of pointers, of maxSeg units, a DxInfo); DxBlk is one block's view.
//
//   stage     grid                              body               a flagged block (DxInfo::bad)
//   tables    (maxSeg, nb) waves                dx_stage_tables    -- (not known yet; a block longer than its row of T gets no table)
//   stitch    nb waves                          dx_stage_stitch    set here: a misfit (dx_misfit: larger than the rows were sized
//             [dxb: compose / hop / units]      dxb_stage_*          for), or a chain the stitch cannot follow; DxInfo starts here
//   fill      (maxSeg, nb) waves                dx_stage_fill      skipped; a unit that fails, or that does not stop where the next
//                                                                    one starts, flags its block -- the block's OTHER units still run
//   jump      (chunks of 1024 bytes, nb) x 4    dx_stage_jump      skipped; one launch per round, dx_rounds_for(span) of them; a
//             waves, once per round                                  block sits a round out once its row of moved[] says it is at rest
//   gather    as jump, once                     dx_stage_gather    skipped: its output is the one-wave decoder's, which runs behind
//
// A flavour (DxF: blocks up to kDxMaxOut; DxbF: raw blocks above; DxlF: history outside the block) supplies what differs: the fill's
// <kHist, kBig> and whether it lists runs, where the block's row of moved[] is, the jump and the gather (the block's own pointer row,
// or the call's pointer space), the rounds a call launches.  The verdict and the counters behind the gather are the kernels'.
//
// Compiled for the CPU as-is by tests/emu (dx_train.h) and checked there against the oracle on valid and corrupt blocks.
#pragma once
#include "lz4_device.inl"

namespace plz4 {

enum : int { kDxSeg = 8192,                 // input bytes per table segment / fill unit
             kDxExt = 32,                   // length bytes a table entry looks through (longer: the stitch parses that sequence itself)
             kDxMaxOut = (4 << 20) + 8,     // the path is taken for outputs up to here (blk/pool.go:23-26: bsz + 8)
             kDxRounds = 24 };              // jump rounds launched: dx_rounds_for(kDxMaxOut) below (a block stops taking part once nothing moves)

struct DxUnit { int32_t ip, op, stop, pad; };               // where the true chain enters a segment (ip < 0: it does not), the output position there, where the unit ends
struct DxInfo { int32_t bad, outLen, tailFrom, pad; uint32_t moved[kDxRounds + 1]; };

DEV uint64_t dx_ent(uint32_t exitPos, uint32_t sum, bool slow) { return (uint64_t)exitPos | ((uint64_t)(slow ? 1u : 0u) << 31) | ((uint64_t)sum << 32); }
DEV uint32_t dx_exit(uint64_t e) { return (uint32_t)e & 0x7FFFFFFFu; }
DEV bool     dx_slow(uint64_t e) { return (((uint32_t)e) >> 31) != 0u; }
DEV uint32_t dx_sum(uint64_t e) { return (uint32_t)(e >> 32); }
DEV int dx_segments(int n) { return n > 0 ? (n + kDxSeg - 1) / kDxSeg : 1; }
DEV int dx_tail_from(int nseg) { return nseg >= 2 ? nseg - 2 : 0; }           // the last two segments are one unit (the block's end rules)
// What a call reserves per block (launch_decode; the bounds program of tests/emu allocates exactly this): table entries for blocks
// of up to maxIn input bytes, pointer entries for outputs of up to maxOut bytes, units.
static inline size_t dx_t_stride(const int64_t maxIn) { return ((size_t)maxIn + 64 + 63) / 64 * 64; }
static inline size_t dx_ptr_stride(const int64_t maxOut) { return ((size_t)(maxOut < kDxMaxOut ? maxOut : (int64_t)kDxMaxOut) + 64 + 1023) / 1024 * 1024; }
static inline int    dx_max_seg(const int64_t maxIn) { return (int)((maxIn + kDxSeg - 1) / kDxSeg); }

// One lane: the sequence that would start at input position p.  *next = where the one behind it starts, *outLen = the bytes it
// produces.  false: not to be told here (too close to the input's end -- the tail unit walks there itself -- or more than kDxExt
// length bytes).  Any byte string parses as SOMETHING: whether p is a real sequence start is the stitch's business.
DEV bool dx_parse_at(const uint8_t* __restrict__ in, const int n, const int p, int* next, int* outLen)
{
    if (p + 24 > n) return false;
    const uint32_t t = in[p];
    int l = (int)(t >> 4), q = p + 1;
    if (l == 15) {
        uint32_t b; int k = 0;
        do { if (q + 24 > n || k == kDxExt) return false; b = in[q++]; l += (int)b; ++k; } while (b == 255u);
    }
    q += l;
    if (q + 24 > n) return false;
    int m = (int)(t & 15u) + kMinMatch;
    q += 2;
    if ((t & 15u) == 15u) {
        uint32_t b; int k = 0;
        do { if (q + 24 > n || k == kDxExt) return false; b = in[q++]; m += (int)b; ++k; } while (b == 255u);
    }
    *next = q; *outLen = l + m;
    return true;
}

// A.  T[p] for the positions of segment j (T has one entry per input byte).
DEV void dx_segment_table(const uint8_t* __restrict__ in, const int n, const int j, uint64_t* __restrict__ T)
{
    const int s0 = j * kDxSeg, s1 = min_(s0 + kDxSeg, n);
    if (s0 >= s1) return;
    for (int base = (s1 - 1) & ~63; base >= s0; base -= 64) {
        LV(int, tgt); LV(int, acc); LV(int, slow);
        LANES({
            const int p = base + LANE;
            int nx = p, ol = 0;
            const bool ok = p < s1 && dx_parse_at(in, n, p, &nx, &ol);
            tgt[I_] = ok ? nx : p; acc[I_] = ok ? ol : 0; slow[I_] = (p < s1 && !ok) ? 1 : 0;
        })
        // inside the batch: a chain advances at least 3 bytes per sequence, so five doublings reach past its 64 positions
        for (int r = 0; r < 5; ++r) {
            LV(int, t2); LV(int, a2); LV(int, s2);
            LANES({ const int sl = (tgt[I_] - base) & 63; t2[I_] = SHFL(tgt, sl); a2[I_] = SHFL(acc, sl); s2[I_] = SHFL(slow, sl); })
            LANES({
                const int p = base + LANE;
                if (!slow[I_] && tgt[I_] > p && tgt[I_] < base + 64) { tgt[I_] = t2[I_]; acc[I_] += a2[I_]; slow[I_] = s2[I_]; }
            })
        }
        // behind the batch: the table of the positions above it (written by the steps before this one)
        LANES({
            const int p = base + LANE;
            uint32_t ex = (uint32_t)tgt[I_], sm = (uint32_t)acc[I_]; bool sl = slow[I_] != 0;
            if (p < s1 && !sl && tgt[I_] >= base + 64 && tgt[I_] < s1) { const uint64_t e = T[tgt[I_]]; ex = dx_exit(e); sm += dx_sum(e); sl = dx_slow(e); }
            if (p < s1) T[p] = dx_ent(ex, sm, sl);
        })
        WAVE_FENCE();
    }
}

// one sequence at position e, whatever its length bytes (uniform code: every lane reads the same bytes); false: it runs into the
// last 24 bytes of the input
DEV bool dx_parse_uniform(const uint8_t* __restrict__ in, const int n, const int e, int* next, int64_t* outLen)
{
    if (e + 24 > n) return false;
    const uint32_t t = UNI((uint32_t)in[e]);
    int64_t l = (int64_t)(t >> 4); int q = e + 1;
    if (l == 15) { uint32_t b; do { if (q + 24 > n) return false; b = UNI((uint32_t)in[q]); ++q; l += b; } while (b == 255u); }
    if ((int64_t)q + l + 24 > (int64_t)n) return false;
    q += (int)l;
    int64_t m = (int64_t)(t & 15u) + kMinMatch;
    q += 2;
    if ((t & 15u) == 15u) { uint32_t b; do { if (q + 24 > n) return false; b = UNI((uint32_t)in[q]); ++q; m += b; } while (b == 255u); }
    *next = q; *outLen = l + m;
    return true;
}

// B.  units[0 .. tailFrom]: the true chain's entries.  Returns 0, or 1 when the block is left to the one-wave decoder.
DEV int dx_stitch(const uint8_t* __restrict__ in, const int n, const int cap, const uint64_t* __restrict__ T, DxUnit* units, const int nseg)
{
    if (n <= 0 || cap <= 0 || cap > kDxMaxOut) return 1;
    const int jt = dx_tail_from(nseg);
    int e = 0; int64_t O = 0;
    bool early = false;                                                  // the tail unit starts before its segments (a sequence that reaches the block's end)
    for (int j = 0; j < jt; ++j) {
        const int s1 = (j + 1) * kDxSeg;
        DxUnit u; u.ip = -1; u.op = 0; u.stop = s1; u.pad = 0;
        if (!early && e < s1) {
            u.ip = e; u.op = (int)O;
            while (e < s1) {
                const uint64_t x = UNI(T[e]);
                O += dx_sum(x); e = (int)dx_exit(x);
                if (dx_slow(x)) {                                       // the chain stands at a sequence the tables could not tell
                    int nx = 0; int64_t ol = 0;
                    if (!dx_parse_uniform(in, n, e, &nx, &ol)) {        // ... and it runs into the block's end: everything from here on is the tail unit's
                        early = true; u.stop = e;
                        if (u.ip >= e) u.ip = -1;
                        break;
                    }
                    O += ol; e = nx;
                }
                if (O > (int64_t)cap) return 1;
            }
        }
        LANES({ if (LANE == 0) units[j] = u; })
    }
    if (e >= n) return 1;                                                // (the last sequence is the tail unit's: it cannot start at the end)
    DxUnit u; u.ip = e; u.op = (int)O; u.stop = n; u.pad = 0;
    LANES({ if (LANE == 0) units[jt] = u; })
    return 0;
}

// ---- Blocks above kDxMaxOut (the big path, dxb_* below): what the fill must not do by itself there.  A literal run or a match of
// `thr` bytes or more is not executed by the unit that meets it but written down -- kind 0: literals, from = input position;
// kind 1: a match, from = offset -- and a grid-wide stage behind the fill copies the literals and writes the pointers (dxb_run_piece).
// A run of L bytes consumes L input or L output bytes, so a block has at most in / thr + out / thr of them: `room` is sized from
// that, and a unit that finds the list full flags its block.  Length bytes are scanned 64 a step.
struct DxRun  { uint32_t op, from, len, kind; };
struct DxRuns { DxRun* list; uint32_t* count; int room; int thr; };
#if defined(PLZ4_EMU)
DEV uint32_t dx_count_up(uint32_t* p) { return (*p)++; }
DEV void     dx_flag(int32_t* p) { *p |= 1; }
#else
DEV uint32_t dx_count_up(uint32_t* p) { return atomicAdd(p, 1u); }
DEV void     dx_flag(int32_t* p) { atomicOr(p, 1); }
#endif
DEV bool dxb_note(const DxRuns* r, const uint32_t kind, const int64_t op, const int64_t from, const int64_t len)
{
    uint32_t at = 0;
    LANES({ if (LANE == 0) at = dx_count_up(r->count); })
    at = UNI(at);
    if (at >= (uint32_t)r->room) return false;
    DxRun x; x.op = (uint32_t)op; x.from = (uint32_t)from; x.len = (uint32_t)len; x.kind = kind;
    LANES({ if (LANE == 0) r->list[at] = x; })
    return true;
}
// read_more_len (lz4_device.inl) 64 length bytes a step: the first byte that is not 255 ends the length.  No byte at or behind
// src + n is read; a length that runs there fails as read_more_len's does (its ip has then passed ilimit <= n).
DEV int64_t dxb_more_len(const uint8_t* __restrict__ src, const int n, int* ip, const int ilimit, const bool initialCheck)
{
    int64_t len = 0;
    if (initialCheck && *ip >= ilimit) return -1;
    for (;;) {
        const int q = *ip;
        LV(uint32_t, b);
        LANES({ b[I_] = (q + LANE < n) ? (uint32_t)src[q + LANE] : 0u; })
        const uint64_t ends = BALLOT(b[I_] != 255u);
        if (!ends) { len += 255 * 64; *ip = q + 64; if (*ip > ilimit) return -1; continue; }
        const int k = ctz64(ends);
        len += (int64_t)255 * k + (int64_t)RL(b, k);
        *ip = q + k + 1;
        return *ip > ilimit ? -1 : len;
    }
}

// a match as pointers: ptr[op + i] = op + i - offset.  An overlapping match (offset < len) points into itself, which is what
// its bytes are (lz4.c:2406-2414).
// kHist (blocks with history outside the block, see dxl_* below): a source before the block's start is written down as the distance
// in front of the block, tagged -- kDxlTag | (distance - 1) -- and resolved once every block's output length is known (dxl_resolve).
enum : uint32_t { kDxlTag = 0x80000000u };
template <bool kHist = false>
DEV void dx_fill_match(uint32_t* __restrict__ ptr, const int64_t op, const int offset, const int len)
{
    LANES({
        for (int i = LANE; i < len; i += 64) {
            const int sp = (int)op + i - offset;                             // (sp < 0: tag | (-sp - 1), which is sp with its low 31 bits flipped)
            ptr[op + i] = kHist ? (uint32_t)(sp ^ ((sp >> 31) & 0x7FFFFFFF)) : (uint32_t)sp;
        }
    })
}

// a literal run / a match of the big path's fill: executed here, or (thr bytes or more) written down; false: the list is full
DEV bool dxb_put_literals(const DxRuns* runs, uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, const int64_t op, const int ip, const int64_t ll)
{
    if (ll >= (int64_t)runs->thr) return dxb_note(runs, 0u, op, ip, ll);
    wave_copy(dst + op, src + ip, (int)ll);
    return true;
}
DEV bool dxb_put_match(const DxRuns* runs, uint32_t* __restrict__ ptr, const int64_t op, const int offset, const int64_t ml)
{
    if (ml >= (int64_t)runs->thr) return dxb_note(runs, 1u, op, offset, ml);
    dx_fill_match<false>(ptr, op, offset, (int)ml);
    return true;
}

// The vector path of the one-wave decoder (wave_decode_plain_batch, lz4_device.inl) with the copies taken out: 64 lanes look at
// the next 64 input bytes as 64 hypothetical sequence starts, a scalar hop follows the real chain while the sequences are plain,
// a prefix sum places them; literals are written, matches become pointers.  Sequences that start at or behind ipStop are the next
// unit's.  Returns the sequences taken (0: the sequential step's turn).
DEV int dx_plain_batch(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, uint32_t* __restrict__ ptr, int* ipp, int64_t* opp,
                       LVREF(v16u_t, win), int* winIp, const int ipStop)
{
    const int ip0 = *ipp; const int64_t op0 = *opp;
    if (*winIp != ip0) { LANES({ win[I_] = *(const v16u_t*)(src + ip0 + LANE); }) }
    LV(uint32_t, b0); LV(int, ll); LV(int, ml); LV(int, off); LV(int, nxt); LV(int, outLen); LV(int, plain); LV(int, coop);
    LANES({
        const uint64_t w0 = (uint64_t)win[I_].w[0] | ((uint64_t)win[I_].w[1] << 32);
        const uint64_t w1 = (uint64_t)win[I_].w[2] | ((uint64_t)win[I_].w[3] << 32);
        const uint32_t t = (uint32_t)(w0 & 0xFF);
        const int l = (int)(t >> 4), mn = (int)(t & 15);
        const int offAt = LANE + 1 + l;
        const uint64_t sel = (l <= 5) ? w0 : (l <= 9 ? ((w0 >> 32) | (w1 << 32)) : w1);
        const int      sft = 8 * (1 + l - (l <= 5 ? 0 : (l <= 9 ? 4 : 8)));
        const uint32_t o16 = (uint32_t)((sel >> (sft & 63)) & 0xFFFF);  // (l == 15: sft is 64, the value unused)
        const bool     lng = (mn == 15);
        const int      ek  = 3 + l;
        const uint32_t e   = (uint32_t)(((ek < 8) ? (w0 >> (8 * ek)) : (w1 >> (8 * (ek & 7)))) & 0xFF);
        const int      mlen = lng ? 19 + (int)e : mn + kMinMatch;
        const bool parse = (l < 14) && (offAt <= 64) && (!lng || (l <= 12 && e < 255));
        const bool simple = parse && !lng && o16 >= (uint32_t)mlen;
        b0[I_] = t; ll[I_] = l; ml[I_] = mlen; off[I_] = (int)o16;
        nxt[I_] = offAt + 2 + (lng ? 1 : 0); outLen[I_] = l + mlen;
        coop[I_]  = parse && !simple && o16 >= 1;
        plain[I_] = simple || coop[I_];
    })
    const uint64_t plainMask = BALLOT(plain[I_]);
    if (!(plainMask & 1)) return 0;
    uint64_t members = 0;
    {
        LV(int, nxtC);
        LANES({ nxtC[I_] = min_(nxt[I_], 64); })
        int cur = 0, seen = 0;
        do {
            for (int u = 0; u < 4; ++u) {
                members |= 1ull << (cur & 63);
                cur = RL(nxtC, cur & 63);
                seen |= cur;
            }
        } while (seen < 64);
        const uint64_t odd = members & ~plainMask;
        if (odd) members &= (1ull << ctz64(odd)) - 1;
        if (ipStop - ip0 < 64) members &= (1ull << (ipStop - ip0)) - 1;    // (ip0 < ipStop: bit 0 stays)
    }
    LV(int, acc); LV(int, outStart); LV(int, sp);
    { const uint64_t mL = members; LANES({ acc[I_] = ((mL >> LANE) & 1) ? outLen[I_] : 0; }) }
    SCAN_INCL(acc);
    {
        const uint64_t mL = members;
        LANES({
            outStart[I_] = (int)op0 + acc[I_] - (((mL >> LANE) & 1) ? outLen[I_] : 0);
            sp[I_]       = outStart[I_] + ll[I_] - off[I_];
        })
        const uint64_t stop = BALLOT(((mL >> LANE) & 1) && (sp[I_] < 0 || acc[I_] > 1024));
        if (stop) members &= (1ull << ctz64(stop)) - 1;
    }
    if (!members) return 0;
    const uint64_t mL = members;
    const int last = 63 - __builtin_clzll(members);
    const int ipn  = ip0 + RL(nxt, last);
    LANES({ win[I_] = *(const v16u_t*)(src + ipn + LANE); })                 // (ipn + 63 + 16 < ip0 + 160 <= iend)
    *winIp = ipn;
    // literal bytes: every window byte finds the member it follows
    LANES({
        const uint64_t upto = mL & ((LANE >= 63) ? ~0ull : ((2ull << LANE) - 1));
        const int m  = upto ? 63 - __builtin_clzll(upto) : LANE;
        const int os = SHFL(outStart, m), lm = SHFL(ll, m);
        if (upto && LANE > m && LANE <= m + lm) dst[os + (LANE - m - 1)] = (uint8_t)b0[I_];
    })
    // matches: pointers, nothing is read
    const uint64_t coopM = mL & BALLOT(coop[I_]);
    LANES({
        if (((mL & ~coopM) >> LANE) & 1) {
            const int o = outStart[I_] + ll[I_];
            for (int i = 0; i < ml[I_]; ++i) ptr[o + i] = (uint32_t)(o + i - off[I_]);
        }
    })
    for (uint64_t pend = coopM; pend; pend &= pend - 1) {
        const int f = ctz64(pend);
        dx_fill_match(ptr, (int64_t)RL(outStart, f) + RL(ll, f), RL(off, f), RL(ml, f));
    }
    *ipp = ipn;
    *opp = (int64_t)RL(outStart, last) + RL(outLen, last);
    return __builtin_popcountll(members);
}

// C.  The sequences from (ip0, op0) on: a unit in the middle of a block (tail = false) walks the reference's fast loop
// (lz4.c:2083-2209) up to ipStop and returns -1 for anything that loop would hand to the safe loop or reject; the tail unit walks to
// the end of the block under both loops' rules (:2215-2435).  Returns the output position reached, or -1: the block is left to the
// one-wave decoder, whose verdict is the reference's.  An offset of 0 (liblz4 zero-fills, :499-507) is left to it as well.
// kHist: the block has history in front of it (LZ4_decompress_safe_usingDict's external-dictionary form, lz4.c:2166-2196, :2358-2384):
// a match may start up to 65535 bytes before the block.  Its end-of-output test (op + length > oend - LASTLITERALS) is the one the
// safe loop makes for every match, and the fast loop only sees matches that end 64 bytes before oend; whether the history is long
// enough for the offset (checkOffset, :2161, :2356) is told by dxl_resolve.
template <bool kHist = false, bool kBig = false>
DEV int64_t wave_dx_fill(const uint8_t* __restrict__ src, const int n, uint8_t* __restrict__ dst, const int cap, uint32_t* __restrict__ ptr,
                         const int ip0, const int64_t op0, const int ipStop, const bool tail, const DxRuns* runs = nullptr)
{
    const int iend = n;
    const int64_t oend = cap;
    int ip = ip0; int64_t op = op0;
    bool fast = (oend - op) >= 64;
    if (!tail && !fast) return -1;
    LV(v16u_t, win); int winIp = -1;
    LANES({ win[I_].w[0] = 0; win[I_].w[1] = 0; win[I_].w[2] = 0; win[I_].w[3] = 0; })
    for (;;) {
        if (!tail && ip >= ipStop) return op;
        if (fast && ip + 160 <= iend && op + 1088 <= oend) {
            const int nm = dx_plain_batch(src, dst, ptr, &ip, &op, win, &winIp, tail ? iend : ipStop);
            if (nm > 0) continue;
        }
        const uint32_t token = UNI((uint32_t)src[ip]); ip++;
        int64_t ll = token >> 4, ml; int offset; int64_t mpos;
        if (fast) {
            bool toSafeLit = false;
            if (ll == 15) {
                const int64_t a = (kBig ? dxb_more_len(src, iend, &ip, iend - 15, true) : read_more_len(src, &ip, iend - 15, true));
                if (a < 0) return -1;
                ll += a;
                if (op + ll > oend - 32 || (int64_t)ip + ll > iend - 32) toSafeLit = true;
            } else if (!(ip <= iend - 17)) {
                toSafeLit = true;
            }
            if (toSafeLit) { if (!tail) return -1; fast = false; goto safe_literals; }
            if (kBig) { if (!dxb_put_literals(runs, dst, src, op, ip, ll)) return -1; } else wave_copy(dst + op, src + ip, (int)ll);
            ip += (int)ll; op += ll;
            offset = (int)UNI((uint32_t)ld16u(src + ip)); ip += 2;
            mpos = op - offset;
            ml = token & 15;
            if (ml == 15) {
                const int64_t a = (kBig ? dxb_more_len(src, iend, &ip, iend - kLastLiterals + 1, false) : read_more_len(src, &ip, iend - kLastLiterals + 1, false));
                if (a < 0) return -1;
                ml += a + kMinMatch;
            } else ml += kMinMatch;
            if (op + ml >= oend - 64) { if (!tail) return -1; fast = false; goto safe_match; }
            if ((!kHist && mpos < 0) || offset == 0) return -1;                // lz4.c:2161
            if (kBig) { if (!dxb_put_match(runs, ptr, op, offset, ml)) return -1; } else dx_fill_match<kHist>(ptr, op, offset, (int)ml);
            op += ml;
            continue;
        }
        if (ll != 15 && ip < iend - 16 && op <= oend - 32) {                   // shortcut, lz4.c:2230-2261
            wave_copy(dst + op, src + ip, (int)ll);
            op += ll; ip += (int)ll;
            ml = token & 15;
            offset = (int)UNI((uint32_t)ld16u(src + ip)); ip += 2;
            mpos = op - offset;
            if (ml != 15 && offset >= 8 && mpos >= 0) {
                dx_fill_match(ptr, op, offset, (int)ml + kMinMatch);
                op += ml + kMinMatch;
                continue;
            }
            goto match_len;
        }
        if (ll == 15) {
            const int64_t a = (kBig ? dxb_more_len(src, iend, &ip, iend - 15, true) : read_more_len(src, &ip, iend - 15, true));
            if (a < 0) return -1;
            ll += a;
        }
safe_literals:
        if (op + ll > oend - kMfLimit || (int64_t)ip + ll > iend - (2 + 1 + kLastLiterals)) {
            if ((int64_t)ip + ll != iend || op + ll > oend) return -1;         // lz4.c:2312-2318
            if (kBig) { if (!dxb_put_literals(runs, dst, src, op, ip, ll)) return -1; } else wave_copy(dst + op, src + ip, (int)ll);
            ip += (int)ll; op += ll;
            break;
        }
        if (kBig) { if (!dxb_put_literals(runs, dst, src, op, ip, ll)) return -1; } else wave_copy(dst + op, src + ip, (int)ll);
        ip += (int)ll; op += ll;
        offset = (int)UNI((uint32_t)ld16u(src + ip)); ip += 2;
        mpos = op - offset;
        ml = token & 15;
match_len:
        if (ml == 15) {
            const int64_t a = (kBig ? dxb_more_len(src, iend, &ip, iend - kLastLiterals + 1, false) : read_more_len(src, &ip, iend - kLastLiterals + 1, false));
            if (a < 0) return -1;
            ml += a;
        }
        ml += kMinMatch;
safe_match:
        if ((!kHist && mpos < 0) || offset == 0) return -1;                    // lz4.c:2356
        if (op + ml > oend - kLastLiterals) return -1;                         // lz4.c:2421-2423 (== :2360-2363 for a match out of the history)
        if (kBig) { if (!dxb_put_match(runs, ptr, op, offset, ml)) return -1; } else dx_fill_match<kHist>(ptr, op, offset, (int)ml);
        op += ml;
    }
    return op;
}

// D.  One jump of the 64 x 4 pointers from p0 on: true when one of them moved.
DEV bool dx_jump(uint32_t* __restrict__ ptr, const int p0, const int outLen)
{
    LV(int, mv);
    LANES({
        mv[I_] = 0;
        for (int k = 0; k < 4; ++k) {
            const int p = p0 + 4 * LANE + k;
            if (p < outLen) {
                const uint32_t q = ptr[p];
                if (q != (uint32_t)p) { const uint32_t r = ptr[q]; if (r != q) { ptr[p] = r; mv[I_] = 1; } }
            }
        }
    })
    return BALLOT(mv[I_]) != 0;
}
// E.  out[p] <- out[ptr[p]] for the 64 x 4 bytes from p0 on (a pointer leads to a literal now, and literals are never written here)
DEV void dx_gather(uint8_t* __restrict__ out, const uint32_t* __restrict__ ptr, const int p0, const int outLen)
{
    LANES({
        for (int k = 0; k < 4; ++k) {
            const int p = p0 + 4 * LANE + k;
            if (p < outLen) { const uint32_t q = ptr[p]; if (q != (uint32_t)p) out[p] = out[q]; }
        }
    })
}

// ---- Blocks with history outside the block: linked blocks (a chain: block i's window is the tail of what the blocks before it
// produced, compress/dict.go:28-41) and independent blocks under a dictionary (chains of one).  The token chain needs no history,
// so stages A and B run on every block of the call at once; the copy chain simply crosses the blocks' borders.  The call has ONE
// pointer space: byte pos of block b is b * P + pos, and behind the last block (from nb * P on) lie 64 Ki indices per chain for
// the history the call came in with (the chain's window, or the dictionary), which like the literals are fixed points.
//   C' wave_dx_fill<true>  as C; a source in front of the block is written down as a tagged distance
//   R  dxl_resolve         once the fill has told every block's output length: block-relative pointers become global ones, tagged
//                          distances the byte they mean -- walking back over the outputs of the chain's earlier compressed blocks
//                          (stored blocks do not enter the window: sync/reader.go:75-78), then into the incoming history.  A
//                          distance beyond all of that flags the block (checkOffset).
//   D' dxl_jump, E' dxl_gather   as D and E over global pointers; the rounds follow the call's total output.
// A chain is answered up to its first block that is not plainly good; from there on the one-wave chain walk takes over, starting
// from the window the good blocks leave (dxl_window).
enum : int { kDxlMaxRounds = 32, kDxlHist = 65536 };
// The rounds rule: a copy chain over a span of N bytes is at most N deep, ceil(log2 N) jump rounds bring every pointer home, and one
// more round sees that nothing moves; at most kDxlMaxRounds (a row of moved[] has one entry more).
static constexpr int dx_rounds_for(const int64_t span) { int r = 1; while (r < kDxlMaxRounds && ((int64_t)1 << (r - 1)) < span) ++r; return r; }
static_assert(dx_rounds_for(kDxMaxOut) == kDxRounds, "DxInfo::moved is sized by kDxRounds");

struct DxlCall {
    uint32_t*       ptr;   int64_t P;   int nb;                 // ptr[b * P + pos]
    const DxInfo*   info;                                       // per block: bad, outLen
    const int32_t*  len;                                        // per block: < 0: not a compressed block (stored / not sane); null: all are
    const int32_t*  first;                                      // per block: the first block of its chain (null: its own)
    const int32_t*  chain;                                      // per block: its chain's number (null: 0, one history for all)
    const uint8_t*  hist;  int64_t histStride;                  // chain ch's incoming history: hist + ch * histStride, histLen bytes
    const int*      histLen;  int histLenAll;
    uint8_t*        dst;   int64_t dstStride;
};
DEV uint32_t dxl_hist0(const DxlCall& c) { return (uint32_t)((int64_t)c.nb * c.P); }

// the byte d (1 .. 65535) in front of block b's start; ~0u: the history is shorter than that
DEV uint32_t dxl_source(const DxlCall& c, const int b, uint32_t d)
{
    const int first = c.first ? c.first[b] : b;
    for (int j = b - 1; j >= first; --j) {
        if (c.len && c.len[j] < 0) continue;
        const uint32_t o = (uint32_t)c.info[j].outLen;
        if (d <= o) return (uint32_t)((int64_t)j * c.P + o - d);
        d -= o;
    }
    const int ch = c.chain ? c.chain[b] : 0;
    const int w = c.histLen ? c.histLen[ch] : c.histLenAll;
    if (w > 0 && d <= (uint32_t)w) return dxl_hist0(c) + (uint32_t)ch * kDxlHist + ((uint32_t)w - d);
    return ~0u;
}
// R.  The 64 x 4 entries of block b from p0 on, up to lim; false: a match reaches behind the history.  Run over ALL P entries of
// EVERY block, flagged ones included: whatever a later block's pointers lead to is then an index of the call's space.
DEV bool dxl_resolve(const DxlCall& c, const int b, const int p0, const int lim)
{
    LV(int, no);
    const uint32_t base = (uint32_t)((int64_t)b * c.P);
    LANES({
        no[I_] = 0;
        for (int k = 0; k < 4; ++k) {
            const int p = p0 + 4 * LANE + k;
            if (p < lim) {
                const uint32_t v = c.ptr[base + p];
                uint32_t g = base + v;
                if (v & kDxlTag) { g = dxl_source(c, b, (v & ~kDxlTag) + 1u); if (g == ~0u) { g = base + (uint32_t)p; no[I_] = 1; } }
                c.ptr[base + p] = g;
            }
        }
    })
    return BALLOT(no[I_]) == 0;
}
// D'.  As dx_jump; indices from hist0 on (the incoming history) are fixed points without an entry of their own.  All of a lane's
// loads come before its stores (the four gathers are in flight together, and no pointer sees one moved by the same step).
DEV bool dxl_jump(uint32_t* __restrict__ ptr, const uint32_t hist0, const uint32_t base, const int p0, const int outLen)
{
    LV(v16u_t, nv); LV(int, mv);
    LANES({
        mv[I_] = 0;
        for (int k = 0; k < 4; ++k) {
            const int p = p0 + 4 * LANE + k;
            nv[I_].w[k] = 0;
            if (p < outLen) {
                const uint32_t g = base + (uint32_t)p, q = ptr[g];
                if (q != g && q < hist0) { const uint32_t r = ptr[q]; if (r != q) { nv[I_].w[k] = r; mv[I_] |= 1 << k; } }
            }
        }
    })
    LANES({
        for (int k = 0; k < 4; ++k) if ((mv[I_] >> k) & 1) ptr[base + (uint32_t)(p0 + 4 * LANE + k)] = nv[I_].w[k];
    })
    return BALLOT(mv[I_]) != 0;
}
// E'.  The literal is in the output of the block that owns it, or in the incoming history.
DEV void dxl_gather(const DxlCall& c, const int b, const int p0, const int outLen)
{
    const uint32_t base = (uint32_t)((int64_t)b * c.P), hist0 = dxl_hist0(c);
    uint8_t* const out = c.dst + (int64_t)b * c.dstStride;
    LANES({
        for (int k = 0; k < 4; ++k) {
            const int p = p0 + 4 * LANE + k;
            if (p < outLen) {
                const uint32_t g = base + (uint32_t)p, q = c.ptr[g];
                if (q != g) {
                    if (q >= hist0) { const uint32_t h = q - hist0; out[p] = c.hist[(int64_t)(h >> 16) * c.histStride + (h & 65535u)]; }
                    else { const uint32_t jb = q / (uint32_t)c.P; out[p] = c.dst[(int64_t)jb * c.dstStride + (q - jb * (uint32_t)c.P)]; }
                }
            }
        }
    })
}
// a block's row of moved[] (kDxlMaxRounds + 1 entries, `rounds` of them launched): has it come to rest, and after how many rounds
DEV bool dxl_converged(const uint32_t* moved, const int rounds) { return rounds > 0 && moved[rounds - 1] == 0u; }
DEV int  dxl_rounds_of(const uint32_t* moved, const int rounds) { int r = 0; while (r < rounds && moved[r]) ++r; return r < rounds ? r + 1 : rounds; }

// The window a chain's blocks [first, cut) leave: compress.DictT.Update block by block gives the last 64 KiB of (incoming window,
// outputs of the compressed blocks).  Written to winB (winA is read); returns its length, or -1: nothing was produced, the window stays.
DEV int dxl_window(const DxlCall& c, const int first, const int cut, const uint8_t* winA, const int winLen, uint8_t* winB)
{
    int64_t sum = 0;
    for (int j = cut - 1; j >= first && sum < kDxlHist; --j) if (!(c.len && c.len[j] < 0)) sum += c.info[j].outLen;
    if (sum == 0) return -1;
    const int s = (int)min_(sum, (int64_t)kDxlHist), keep = min_(winLen, kDxlHist - s);
    wave_copy(winB, winA + (winLen - keep), keep);
    int pos = keep + s;
    for (int j = cut - 1; j >= first && pos > keep; --j) {
        if (c.len && c.len[j] < 0) continue;
        const int o = c.info[j].outLen, take = min_(o, pos - keep);
        wave_copy(winB + (pos - take), c.dst + (int64_t)j * c.dstStride + (o - take), take);
        pos -= take;
    }
    return keep + s;
}

// ---- A linked call cut into groups of consecutive blocks (launch_decode): the plan, made on the host, and a group's view of the
// call's chains.  A group is the blocks [g0, g1) and the chains [ch0, ch1): ch0 the chain block g0 belongs to, ch1 - 1 the last chain
// that starts in front of g1; a chain in between may have no block at all.  first: the call's chainFirst (nCh + 1 entries; null: one
// chain); *cursor: where the search for ch0 goes on from group to group (0 at the first).
struct DxlGroup { int g0, g1, ch0, ch1; };
static inline void dxl_group(const int32_t* first, const int nCh, const int nb, const int G, const int g0, int* cursor, DxlGroup* g)
{
    g->g0 = g0; g->g1 = g0 + G < nb ? g0 + G : nb;
    if (!first) { g->ch0 = 0; g->ch1 = 1; return; }
    int ch = *cursor;
    while (ch + 1 < nCh && first[ch + 1] <= g0) ++ch;
    int hi = ch;
    while (hi + 1 < nCh && first[hi + 1] < g->g1) ++hi;
    *cursor = ch; g->ch0 = ch; g->ch1 = hi + 1;
}
// where chain ch (counted from the group's first chain; chainFirst points at that chain's entry) starts inside a group of nb blocks
// that begins at the call's block blk0: the call's own number, clamped to the group
DEV int dxl_chain_lo(const int32_t* chainFirst, const int blk0, const int nb, const int ch)
{
    const int v = chainFirst[ch] - blk0;
    return v < 0 ? 0 : (v > nb ? nb : v);
}

// ---- The finish stage of a linked chain, and the one-wave walk behind it.  One body for k_dxl_finish, k_decode_rec_linked and the
// lane-emulated build.  rec(i, hist, histLen, &r, &st, &stored) decodes record i of the call the serial way against the
// window (hist, histLen): its result, its status (0: ok), and whether it was a stored block (copied out; it does not enter the
// window).  DxlFin: what the stage reads beside the DxlCall (checksum verdicts, the blocks' rows of moved flags, the rounds
// launched) and where the blocks' answers go.
// Records on this path (k_dx_rec_prep): what the path keeps as a record's length -- the payload's size where the record is a
// compressed payload of a sane size (FrameReader._read's checks, blk/frame.go:79-85), -1 for a stored block that fits its output,
// kDxRecBad for a record the frame reader turns away (rec_head's -1, or a stored block above dstCap): both are the one-wave decoder's.
enum : int { kDxRecBad = -2 };
DEV int dx_rec_len(const uint8_t* __restrict__ rec, const int64_t recLen, const int bsz, const bool checksum, const int dstCap)
{
    uint32_t word;
    const int sz = rec_head<false>(rec, recLen, bsz, checksum, &word);
    const bool stored = (word & 0x80000000u) != 0;
    return (sz < 0 || (stored && sz > dstCap)) ? (int)kDxRecBad : (stored ? -1 : sz);
}
// A chain ends at its first bad block.  What is known of that before the decode -- a record in front of block i that the frame
// reader turns away, or a bad block in an earlier group of a cut call (deadIn) -- keeps the stages off block i (k_dxl_link flags
// it), so its output stays as it was, as on the one-wave walk; dxl_finish answers it CORRUPT.  first: the chain's first block.
DEV bool dxl_chain_dead(const int32_t* __restrict__ len, const int first, const int i, const int deadIn)
{
    int dead = deadIn;
    for (int j = first; j < i; ++j) dead |= len[j] == kDxRecBad;
    return dead != 0;
}

enum : int { kDxlStCorrupt = 3 };                                   // PLZ4HIP_BLK_CORRUPT: what a block behind a bad block of its chain gets

struct DxlFin {
    const int32_t*  hashBad;                                        // per block: its checksum does not match (null: none is checked)
    const uint32_t* moved;  int rounds;                             // per block kDxlMaxRounds + 1 flags; the jump rounds launched
    int32_t*        result; int32_t* status;
};
DEV bool dxl_block_good(const DxlCall& c, const DxlFin& f, const int b)
{
    return !(c.len && c.len[b] < 0) && !c.info[b].bad && !(f.hashBad && f.hashBad[b])
        && dxl_converged(f.moved + (int64_t)b * (kDxlMaxRounds + 1), f.rounds);
}
DEV void dxl_answer(const DxlFin& f, const int i, const int r, const int st)
{
    LANES({ if (LANE == 0) { f.result[i] = r; f.status[i] = st; } })
}

// Linked blocks: a serial chain, one wave.  The window follows compress.DictT.Update (compress/dict.go:28-41) and is
// NOT updated by stored blocks (sync/reader.go:75-78, async/reader.go:149-163) -- the reference's behaviour, kept.
// The records [first, last) of a chain from the window (winA, winLen) on; dead: an earlier record of the chain has failed (every
// record then gets result 0 / kDxlStCorrupt, its output and the window stay as they are).  The live window ends up in win0;
// *winLenOut / *deadOut: the state the chain's next records start from.
template <class Rec>
DEV void dxl_walk(const DxlCall& c, const DxlFin& f, Rec& rec, const int first, const int last, uint8_t* const win0,
                  uint8_t* winA, uint8_t* winB, int winLen, bool dead, int* winLenOut, int* deadOut)
{
    for (int i = first; i < last; ++i) {
        int r = 0, st = kDxlStCorrupt; bool stored = false;
        if (!dead) rec(i, winA, winLen, &r, &st, &stored);
        dxl_answer(f, i, r, st);
        if (st != 0) { dead = true; continue; }                             // first error ends the stream
        if (stored) continue;
        const uint8_t* out = c.dst + (int64_t)i * c.dstStride;
        WAVE_FENCE();
        if (r >= kDxlHist) { wave_copy(winB, out + (r - kDxlHist), kDxlHist); winLen = kDxlHist; }
        else {
            int keep = winLen;
            if (winLen + r > kDxlHist) keep = kDxlHist - r;
            wave_copy(winB, winA + (winLen - keep), keep);
            wave_copy(winB + keep, out, r);
            winLen = keep + r;
        }
        WAVE_FENCE();
        uint8_t* t = winA; winA = winB; winB = t;
    }
    // leave the live window in the first half for whoever goes on
    if (winA != win0) { WAVE_FENCE(); wave_copy(win0, winA, winLen); }
    *winLenOut = winLen; *deadOut = dead ? 1 : 0;
}

// The blocks [first, last) of one chain behind the gather, one wave: the chain's good blocks are answered (a stored block among them
// is copied out here and does not enter the window), the window they leave is laid down, and from the first block that is not
// plainly good the one-wave walk goes on (its own verdict for that block, CORRUPT for what follows, the window as it was in front
// of it).  win0: the chain's 2 x 64 KiB, the live window in the first half.  *winLenIO, *deadIO: the chain's state in front of
// `first` and behind `last` -- what a call cut into groups of blocks carries from group to group.  *takenOut: compressed blocks the
// few-block path answered, *roundsOut: the jump rounds the slowest of them took.
template <class Rec>
DEV void dxl_finish(const DxlCall& c, const DxlFin& f, Rec& rec, const int first, const int last, uint8_t* const win0,
                    int* winLenIO, int* deadIO, int* takenOut, int* roundsOut)
{
    uint8_t* winA = win0; uint8_t* winB = win0 + kDxlHist;
    int winLen = *winLenIO;
    bool dead = *deadIO != 0;
    int i = first, taken = 0, rounds = 0;
    if (!dead) for (; i < last; ++i) {
        if (!(c.len && UNI(c.len[i]) < 0)) {
            if (!UNI((int)dxl_block_good(c, f, i))) break;
            dxl_answer(f, i, c.info[i].outLen, 0);
            ++taken;
            const int rr = UNI(dxl_rounds_of(f.moved + (int64_t)i * (kDxlMaxRounds + 1), f.rounds));
            if (rr > rounds) rounds = rr;
        } else {
            int r = 0, st = 0; bool stored = false;
            rec(i, nullptr, 0, &r, &st, &stored);                           // a stored block, or a record that fails the frame reader's checks
            dxl_answer(f, i, r, st);
            if (st != 0) { dead = true; ++i; break; }
        }
    }
    WAVE_FENCE();
    const int t = dxl_window(c, first, i, winA, winLen, winB);
    WAVE_FENCE();
    if (t >= 0) { uint8_t* x = winA; winA = winB; winB = x; winLen = t; }
    *takenOut = taken; *roundsOut = rounds;
    dxl_walk(c, f, rec, i, last, win0, winA, winB, winLen, dead, winLenIO, deadIO);
}

// ---- Raw blocks above kDxMaxOut without history outside the block (the big path; launch_decode takes it for a call of few blocks
// of which one may be larger than that, up to PLZ4HIP_DX_BIG_MAX_MIB).  A, C, D and E are the stages above; what one wave did there
// for a whole block is cut once more:
//   B1 dxb_compose     the segments in groups of G: for every position p of a group's FIRST segment, where the chain from p leaves
//                      the group and the output it passes -- up to G lookups of the base table per position, every position of
//                      every group at once.  An entry the base table could not tell (slow) stops a composition where it stands.
//   B2 dxb_hop         one wave per block hops from group to group -- one lookup of the composed table where the chain enters a
//                      group in its first segment, which is the rule; the base table otherwise -- and writes down where the chain
//                      enters every group, the tail unit, and whether the output fits the capacity.
//   B3 dxb_group_units one wave per group walks its own segments with the base table, all groups at once: the units.
//                      The serial depth is segments / G + G where it was the segments.
//   C  wave_dx_fill<false, true>: length bytes 64 a step; runs of thr bytes or more are written down, not executed (DxRuns)
//   C2 dxb_run_piece   the runs, 16 KiB a wave, over the whole grid
//   D  dx_jump for ceil(log2(output)) + 1 rounds, at most kDxlMaxRounds (16 MiB of one byte value needs 25)
// Positions are 31-bit (dx_ent), sums 32-bit: a segment passes at most 8192 / 35 x 8179 < 2 MiB of output through sequences the
// table can tell, a group of at most kDxbMaxGroup segments 512 MiB.
enum : int { kDxbMaxGroup = 256, kDxbPiece = 16384, kDxbThr = 65536, kDxbTailRoom = 256 };
struct DxbEntry { int32_t ip, op; };                                       // where the chain enters a group (ip < 0: it does not), the output position there
struct DxbInfo  { uint32_t runs, pad; uint32_t moved[kDxlMaxRounds + 1]; };
static inline int    dxb_groups(const int64_t maxSeg, const int G) { return (int)((maxSeg + G - 1) / G); }
static inline size_t dxb_ptr_stride(const int64_t maxOut) { return ((size_t)maxOut + 64 + 1023) / 1024 * 1024; }
static inline int    dxb_run_room(const int64_t maxIn, const int64_t maxOut, const int thr) { return (int)(maxIn / thr + maxOut / thr + 2); }
static inline int    dxb_rounds(const int64_t maxOut) { return dx_rounds_for(maxOut); }
// the group size a call is laid out for: the power of two next to the square root of its segments
static inline int    dxb_group_for(const int64_t maxSeg) { int g = 2; while (g < kDxbMaxGroup && (int64_t)g * g < maxSeg) g *= 2; return g; }

// dx_parse_uniform with the length bytes 64 a step
DEV bool dxb_len_bytes(const uint8_t* __restrict__ in, const int n, int* qq, int64_t* len)
{
    for (;;) {
        const int q = *qq;
        LV(uint32_t, b);
        LANES({ b[I_] = (q + LANE + 24 <= n) ? (uint32_t)in[q + LANE] : 256u; })         // (256: the check in front of that byte fails)
        const uint64_t ends = BALLOT(b[I_] != 255u);
        if (!ends) { *len += 255 * 64; *qq = q + 64; continue; }
        const int k = ctz64(ends);
        const uint32_t v = RL(b, k);
        if (v > 255u) return false;
        *len += (int64_t)255 * k + (int64_t)v; *qq = q + k + 1;
        return true;
    }
}
DEV bool dxb_parse_uniform(const uint8_t* __restrict__ in, const int n, const int e, int* next, int64_t* outLen)
{
    if (e + 24 > n) return false;
    const uint32_t t = UNI((uint32_t)in[e]);
    int64_t l = (int64_t)(t >> 4); int q = e + 1;
    if (l == 15 && !dxb_len_bytes(in, n, &q, &l)) return false;
    if ((int64_t)q + l + 24 > (int64_t)n) return false;
    q += (int)l;
    int64_t m = (int64_t)(t & 15u) + kMinMatch;
    q += 2;
    if ((t & 15u) == 15u && !dxb_len_bytes(in, n, &q, &m)) return false;
    // a long sequence that ends within kDxbTailRoom bytes of the input's end: its match may end where the reference has left its fast
    // loop (less than 64 bytes of output to come), which only the tail unit may walk -- it starts here, then
    if (q + kDxbTailRoom > n) return false;
    *next = q; *outLen = l + m;
    return true;
}

// B1.  TG[g * kDxSeg + i] for the 64 positions i = 64 * sub + lane of group g's first segment (groups that have all their G
// segments in front of the tail unit: g < jt / G)
DEV void dxb_compose(const uint64_t* __restrict__ T, uint64_t* __restrict__ TG, const int n, const int g, const int G, const int sub)
{
    const int64_t g0 = (int64_t)g * G * kDxSeg, g1 = g0 + (int64_t)G * kDxSeg;
    LANES({
        const int64_t p = g0 + 64 * sub + LANE;
        if (p < (int64_t)n) {
            int64_t e = p; uint32_t sum = 0; bool slow = false;
            while (e < g1 && !slow) { const uint64_t x = T[e]; sum += dx_sum(x); e = (int64_t)dx_exit(x); slow = dx_slow(x); }
            TG[(int64_t)g * kDxSeg + 64 * sub + LANE] = dx_ent((uint32_t)e, sum, slow);
        }
    })
}
// the chain from (e, O) on up to `end` (a segment's or a group's end): false when it stands at a sequence that runs into the block's
// end (everything from there on is the tail unit's).  tg: the composed row of the group that starts at tgFrom and ends at `end`
// (null: none) -- taken wherever the chain stands in that group's first segment.
DEV bool dxb_chain_to(const uint8_t* __restrict__ in, const int n, const uint64_t* __restrict__ T, const uint64_t* __restrict__ tg,
                      const int64_t tgFrom, const int64_t end, int* ep, int64_t* Op)
{
    int e = *ep; int64_t O = *Op; bool ok = true;
    while ((int64_t)e < end) {
        const bool hop = tg && (int64_t)e >= tgFrom && (int64_t)e < tgFrom + kDxSeg;
        const uint64_t x = UNI(hop ? tg[(int64_t)e - tgFrom] : T[e]);
        O += dx_sum(x); e = (int)dx_exit(x);
        if (dx_slow(x)) {
            int nx = 0; int64_t ol = 0;
            if (!dxb_parse_uniform(in, n, e, &nx, &ol)) { ok = false; break; }
            O += ol; e = nx;
        }
    }
    *ep = e; *Op = O;
    return ok;
}
// B2.  ent[0 .. groups), units[tailFrom].  Returns 0, or 1 when the block is left to the one-wave decoder.
DEV int dxb_hop(const uint8_t* __restrict__ in, const int n, const int cap, const uint64_t* __restrict__ T, const uint64_t* __restrict__ TG,
                DxbEntry* ent, DxUnit* units, const int nseg, const int G)
{
    if (n <= 0 || cap <= 0) return 1;
    const int jt = dx_tail_from(nseg), ngrp = (jt + G - 1) / G;
    int e = 0; int64_t O = 0; bool early = false;
    for (int g = 0; g < ngrp; ++g) {
        const int64_t g0 = (int64_t)g * G * kDxSeg, gEnd = (int64_t)min_((g + 1) * G, jt) * kDxSeg;
        DxbEntry x; x.ip = -1; x.op = 0;
        if (!early && (int64_t)e < gEnd) {
            x.ip = e; x.op = (int)O;
            const bool full = (g + 1) * G <= jt;                             // (the composed table is the group's: all G segments)
            if (!dxb_chain_to(in, n, T, full ? TG + (int64_t)g * kDxSeg : nullptr, g0, gEnd, &e, &O)) early = true;
            if (O > (int64_t)cap) return 1;
        }
        LANES({ if (LANE == 0) ent[g] = x; })
    }
    if (e >= n) return 1;
    DxUnit u; u.ip = e; u.op = (int)O; u.stop = n; u.pad = 0;
    LANES({ if (LANE == 0) units[jt] = u; })
    return 0;
}
// B3.  units[j] for group g's segments in front of the tail unit (dx_stitch's loop from the group's entry on)
DEV void dxb_group_units(const uint8_t* __restrict__ in, const int n, const uint64_t* __restrict__ T, const DxbEntry* ent, DxUnit* units,
                         const int nseg, const int G, const int g)
{
    const int jt = dx_tail_from(nseg), j1 = min_((g + 1) * G, jt);
    const DxbEntry x = ent[g];
    int e = UNI(x.ip); int64_t O = UNI(x.op);
    bool early = e < 0;
    for (int j = g * G; j < j1; ++j) {
        const int s1 = (j + 1) * kDxSeg;
        DxUnit u; u.ip = -1; u.op = 0; u.stop = s1; u.pad = 0;
        if (!early && e < s1) {
            u.ip = e; u.op = (int)O;
            if (!dxb_chain_to(in, n, T, nullptr, 0, s1, &e, &O)) { early = true; u.stop = e; if (u.ip >= e) u.ip = -1; }
        }
        LANES({ if (LANE == 0) units[j] = u; })
    }
}
// C2.  Piece c (kDxbPiece bytes) of a run
DEV void dxb_run_piece(const DxRun& r, const uint32_t c, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, uint32_t* __restrict__ ptr)
{
    const int64_t at = (int64_t)c * kDxbPiece;
    const int len = (int)min_((int64_t)kDxbPiece, (int64_t)r.len - at);
    if (r.kind == 0u) wave_copy(dst + r.op + at, src + r.from + at, len);
    else dx_fill_match<false>(ptr, (int64_t)r.op + at, (int)r.from, len);
}
DEV uint32_t dxb_run_pieces(const DxRun& r) { return (r.len + (uint32_t)kDxbPiece - 1u) / (uint32_t)kDxbPiece; }

// ---- The stage train (the table at the head of this file): one block's view of the call, the body of every stage, the flavours.
// DxBlk: plain pointers and numbers -- the block (dx_src / dx_len / cap_of of plz4hip.hip), its rows of the call's tables and what
// they were sized for, its DxInfo, its number in the call.
struct DxBlk {
    const uint8_t* src; int n; uint8_t* dst; int cap;
    uint64_t* T; uint32_t* ptr; DxUnit* units;
    int64_t tStride, pStride; int maxSeg;
    DxInfo* info;
    int b;
};

// The misfit rule: a block larger than what the tables, units and pointers were sized for is left to the one-wave kernel.  (The
// first term alone keeps the tables stage off a row of T that is too short; the stitch stage flags the block.)
DEV bool dx_table_misfit(const DxBlk& k) { return (int64_t)k.n > k.tStride - 64; }
DEV bool dx_misfit(const DxBlk& k) { return dx_segments(k.n) > k.maxSeg || dx_table_misfit(k) || (int64_t)k.cap > k.pStride - 64; }

// Where a block's state starts: the stitch stage's verdict, no output yet, no round has moved anything (bi: the big path's state too).
DEV void dx_info_begin(const DxBlk& k, const int bad, DxbInfo* bi = nullptr)
{
    LANES({
        if (LANE == 0) {
            DxInfo inf; inf.bad = bad; inf.outLen = 0; inf.tailFrom = dx_tail_from(dx_segments(k.n)); inf.pad = 0;
            for (int r = 0; r <= kDxRounds; ++r) inf.moved[r] = 0;
            *k.info = inf;
            if (bi) {
                DxbInfo x; x.runs = 0; x.pad = 0;
                for (int r = 0; r <= kDxlMaxRounds; ++r) x.moved[r] = 0;
                *bi = x;
            }
        }
    })
}

// tables: wave j of `shares` lays down its share of the pointer row as the identity, then the table of input segment j
DEV void dx_stage_tables(const DxBlk& k, const int j, const uint32_t shares)
{
    const int64_t share = (k.pStride + shares - 1) / shares;
    const int64_t lo = (int64_t)j * share, hi = lo + share < k.pStride ? lo + share : k.pStride;
    LANES({ for (int64_t p = lo + LANE; p < hi; p += 64) k.ptr[p] = (uint32_t)p; })
    if (k.n <= 0 || (int64_t)j * kDxSeg >= k.n || dx_table_misfit(k)) return;
    dx_segment_table(k.src, k.n, j, k.T);
}
// stitch (DxF, DxlF): one wave per block
DEV void dx_stage_stitch(const DxBlk& k)
{
    const int bad = dx_misfit(k) ? 1 : dx_stitch(k.src, k.n, k.cap, k.T, k.units, dx_segments(k.n));
    dx_info_begin(k, bad);
}
// fill: unit j of the block.  Where a unit stops is where the next one starts, or the block is flagged.  What it found, for whoever
// looks: units that do not meet are a bug of the stitch, and the emulation tells them from a block the fill declines.
enum : int { kDxFillIdle = 0, kDxFillOk = 1, kDxFillLeft = 2, kDxFillDisagree = 3 };
template <class F> DEV int dx_stage_fill(const F& f, const DxBlk& k, const int j)
{
    DxInfo* const inf = k.info;
    if (inf->bad || j > inf->tailFrom) return kDxFillIdle;
    const int jt = inf->tailFrom;
    const DxUnit u = k.units[j];
    if (j < jt && u.ip < 0) return kDxFillIdle;
    const DxRuns runs = f.runs();
    const int64_t r = wave_dx_fill<F::kHist, F::kBig>(k.src, k.n, k.dst, k.cap, k.ptr, u.ip, u.op, u.stop, j == jt, F::kBig ? &runs : nullptr);
    bool ok = r >= 0;
    if (ok && j < jt) {
        int nx = j + 1; while (nx < jt && k.units[nx].ip < 0) ++nx;
        ok = k.units[nx].op == (int)r;
    }
    LANES({ if (LANE == 0) { if (!ok) dx_flag(&inf->bad); else if (j == jt) inf->outLen = (int)r; } })
    return ok ? kDxFillOk : (r >= 0 ? kDxFillDisagree : kDxFillLeft);
}
// jump: round r over the 64 x 4 pointers from p0 on
template <class F> DEV void dx_stage_jump(const F& f, const DxBlk& k, const int r, const int p0)
{
    uint32_t* const moved = f.moved(k);
    if (k.info->bad || (r > 0 && !moved[r - 1])) return;
    const int outLen = k.info->outLen;
    if (p0 >= outLen) return;
    if (f.jump(k, p0, outLen)) { LANES({ if (LANE == 0) moved[r] = 1u; }) }
}
// gather: the 64 x 4 bytes from p0 on
template <class F> DEV void dx_stage_gather(const F& f, const DxBlk& k, const int p0)
{
    if (k.info->bad) return;
    const int outLen = k.info->outLen;
    if (p0 >= outLen) return;
    f.gather(k, p0, outLen);
}

// The flavours.  rounds(nb, maxOut): the jump rounds a call of nb blocks with outputs of up to maxOut bytes launches.
struct DxF {                                                                // blocks up to kDxMaxOut, raw or records
    static constexpr bool kHist = false, kBig = false;
    static constexpr int rounds(int, int64_t) { return dx_rounds_for(kDxMaxOut); }
    DEVM DxRuns runs() const { return DxRuns{nullptr, nullptr, 0, 0}; }
    DEVM uint32_t* moved(const DxBlk& k) const { return k.info->moved; }   // kDxRounds + 1 entries
    DEVM bool jump(const DxBlk& k, int p0, int outLen) const { return dx_jump(k.ptr, p0, outLen); }
    DEVM void gather(const DxBlk& k, int p0, int outLen) const { dx_gather(k.dst, k.ptr, p0, outLen); }
};
struct DxbF {                                                               // raw blocks above kDxMaxOut: the block's rows of the big path's arrays
    static constexpr bool kHist = false, kBig = true;
    static int rounds(int, int64_t maxOut) { return dxb_rounds(maxOut); }
    uint64_t* TG; DxbEntry* ent; int G;                                     // the stitch in three steps: dxb_stage_* below
    DxRun* list; int room, thr; DxbInfo* bi;
    DEVM DxRuns runs() const { return DxRuns{list, &bi->runs, room, thr}; }
    DEVM uint32_t* moved(const DxBlk&) const { return bi->moved; }         // kDxlMaxRounds + 1 entries
    DEVM bool jump(const DxBlk& k, int p0, int outLen) const { return dx_jump(k.ptr, p0, outLen); }
    DEVM void gather(const DxBlk& k, int p0, int outLen) const { dx_gather(k.dst, k.ptr, p0, outLen); }
};
struct DxlF {                                                               // history outside the block: the call's one pointer space
    static constexpr bool kHist = true, kBig = false;
    static int rounds(int nb, int64_t maxOut) { return dx_rounds_for((int64_t)nb * (maxOut < kDxMaxOut ? maxOut : (int64_t)kDxMaxOut) + kDxlHist); }
    DxlCall call; uint32_t* movedAll;                                       // per block kDxlMaxRounds + 1 entries
    DEVM DxRuns runs() const { return DxRuns{nullptr, nullptr, 0, 0}; }
    DEVM uint32_t* moved(const DxBlk& k) const { return movedAll + (int64_t)k.b * (kDxlMaxRounds + 1); }
    DEVM bool jump(const DxBlk& k, int p0, int outLen) const { return dxl_jump(call.ptr, dxl_hist0(call), (uint32_t)((int64_t)k.b * call.P), p0, outLen); }
    DEVM void gather(const DxBlk& k, int p0, int outLen) const { dxl_gather(call, k.b, p0, outLen); }
};

// The big path's stitch, three stages: compose -- (groups x 128, nb) waves, wave `sub` of group g; hop -- nb waves, and the block's
// state starts here; units -- (groups, nb) waves.
DEV void dxb_stage_compose(const DxbF& f, const DxBlk& k, const int g, const int sub)
{
    if (k.n <= 0 || dx_misfit(k)) return;
    if ((g + 1) * f.G > dx_tail_from(dx_segments(k.n))) return;             // (only groups with all their segments are hopped over)
    dxb_compose(k.T, f.TG, k.n, g, f.G, sub);
}
DEV void dxb_stage_hop(const DxbF& f, const DxBlk& k)
{
    const int bad = dx_misfit(k) ? 1 : dxb_hop(k.src, k.n, k.cap, k.T, f.TG, f.ent, k.units, dx_segments(k.n), f.G);
    dx_info_begin(k, bad, f.bi);
}
DEV void dxb_stage_units(const DxbF& f, const DxBlk& k, const int g)
{
    if (k.info->bad) return;
    const int nseg = dx_segments(k.n);
    if (g * f.G >= dx_tail_from(nseg)) return;
    dxb_group_units(k.src, k.n, k.T, f.ent, k.units, nseg, f.G, g);
}

}  // namespace plz4
