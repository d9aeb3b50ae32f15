// lz4hcx_device.inl -- HC levels 2..12 for a block of at most 4 KiB under an attached dictionary context (usingDictCtxHc), by one
// wavefront per block with nothing in device memory but the block, the dictionary, the output and a per-wave slot of the HC workspace (levels 10..12: the price
// table; level 2: the sequence records).
//
//   reference: internal/pkg/clz4/lz4hc.c of the project this one is modelled on
//     LZ4HC_compress_generic_dictCtx :1442-1463 (an input of at most 4 KiB keeps its own, empty tables and searches the
//     dictionary context's behind them), LZ4HC_InsertAndGetWiderMatch :884-1104 (the dictionary's chain :1066-1095),
//     LZ4HC_compress_hashChain :1121-1363, LZ4HC_compress_optimal :1823-2123, LZ4HC_encodeSequence :268-354, LZ4_loadDictHC :1626-1653.
//
// (1) The block's own chain.  Its tables start empty and every position below ip is inserted when ip is searched (:914), so the
//     chain is a function of the block's bytes: hcx_build sorts the block's positions by hash (two stable radix passes over the 15
//     bits, ranks inside a batch of 64 from ballots) into `list` -- the positions of a hash are one ascending run -- and notes in
//     `rank` where a position sits.  Both are 16-bit arrays in LDS: 12 bits of value, and in the upper four bits of the two
//     entries of a position the place of that position in its run, saturated at 255.  17 KiB per wave, nothing to zero.
// (2) The dictionary's chain is laid out the same way once per dictionary (hcx_dict_build, by the host in plz4hip_dict_create): the
//     positions LZ4_loadDictHC inserts (all but the last three) in ascending runs per hash, start[h] .. start[h + 1].
// (3) Levels 3..9: a search has `nb` attempts (1 << (level - 1)).  The own walk takes one per position of the hash's run below ip -- every own
//     candidate of such a block is inside the window, and the chain ends with a saturated link -- so it uses own = min(place of ip
//     in its run, nb) of them, and the dictionary's chain is read with the nb - own left over (:1067), nearest first, while the
//     distance in the block's index space (ip + dictionary length - position) is at most 65535 (:1072-1074; it grows along the
//     chain).  So a search is at most nb candidates, candidate c < own in the block, the others in the dictionary: one per lane
//     (hcx_find_round), each counted exactly -- a dictionary candidate forwards to the dictionary's end only (vLimit, :1080-1081),
//     backwards to its first byte (:1083) -- and the answer is the first candidate with the largest total above `longest`: the
//     walk replaces its best only by a longer one (:934, :1085), and its 2-byte filter (:921) rejects no own candidate that would
//     improve (see hc_find_round, lz4hc_lazy_device.inl).  The first search of a sequence takes 64 / nb positions at once.
//     Level 9's pattern analysis steps in at an own candidate whose link is 1 (:989), and the optimal parser's levels run pattern
//     analysis and the chain swap in every search: there the own walk's attempts are not a count of positions.  Those searches walk
//     the own chain with hc_find_wider_lists (lz4hc_device.inl: up to 63 candidates per round, one per lane, the reference's walk
//     event by event -- here over the lists in LDS), which says how many attempts it left; the dictionary's candidates are then
//     taken one per lane with those (hcx_find_general).
// (4) The walks: levels 3..9 the three-state machine of hc_lazy_run_t, levels 10..12 the optimal parser as hc_opt_run walks it
//     (lz4hc_lazy_device.inl), one segment each; a sequence is written where it is decided, literals by all lanes, with
//     LZ4HC_encodeSequence's own output checks.
// (5) Level 2 is hc_mid_parse with its two tables compacted into LDS and the dictionary step: see hcx_mid_block at the end.
// Compiled for the CPU as-is by tests/emu/emu_hcx.cpp (checked there against the real liblz4).
#pragma once
#include "lz4hc_lazy_device.inl"

namespace plz4 {

enum : int { kHcxMaxBlock = 4096, kHcxMinLevel = 2, kHcxMaxLevel = 12 };
struct HcxLds { uint16_t rank[kHcxMaxBlock]; uint16_t list[kHcxMaxBlock]; uint32_t cnt[256]; };
struct HcxDict {
    const uint8_t* bytes; int len;      // the dictionary (its last <= 64 KiB)
    const uint32_t* start;              // kHcHashEntries + 1 entries: hash h's positions are list[start[h] .. start[h + 1]), ascending
    const uint16_t* list;               // null: no dictionary bytes at all
};
enum : int { kHcxDictStartBytes = ((kHcHashEntries + 1) * 4 + 255) & ~255, kHcxDictBytes = kHcxDictStartBytes + 65536 * 2 };

// What LZ4_loadDictHC leaves in a dictionary context's hash chain (LZ4HC_Insert up to the last three positions, :1647-1650), as
// runs per hash.  Host code: plz4hip_dict_create, and the emulation harness.
static inline void hcx_dict_build(const uint8_t* dict, int len, uint32_t* start, uint16_t* list)
{
    const int m = len >= 4 ? len - 3 : 0;
    for (int h = 0; h <= kHcHashEntries; ++h) start[h] = 0;
    const auto hash = [&](int p) { uint32_t v; memcpy(&v, dict + p, 4); return (v * 2654435761u) >> 17; };
    for (int p = 0; p < m; ++p) start[hash(p) + 1]++;
    for (int h = 0; h < kHcHashEntries; ++h) start[h + 1] += start[h];      // start[h + 1]: where hash h's run ends
    for (int p = m - 1; p >= 0; --p) { const uint32_t h = hash(p); list[--start[h + 1]] = (uint16_t)p; }
    // (filled from the top: start[h + 1] has come down to where hash h's run starts)
    for (int h = 0; h < kHcHashEntries; ++h) start[h] = start[h + 1];
    start[kHcHashEntries] = (uint32_t)m;
}

// ---- (1) the block's lists
// m[lane]: the active lanes with this lane's digit
DEV void hcx_match(LVREF(uint32_t, d), LVREF(bool, on), LVREF(uint64_t, m))
{
    const uint64_t act = BALLOT(on[I_]);
    LANES({ m[I_] = act; })
    for (int b = 0; b < 8; ++b) {
        const uint64_t bal = BALLOT((d[I_] >> b) & 1u);
        LANES({ m[I_] &= ((d[I_] >> b) & 1u) ? bal : ~bal; })
    }
}
// one stable radix pass over eight bits of the hash: in[0 .. M) (kFirst: the positions 0 .. M themselves) -> out
template <bool kFirst>
DEV void hcx_sort_pass(const uint8_t* __restrict__ src, const int M, const uint16_t* in, uint16_t* out, uint32_t* cnt, const int shift)
{
    LANES({ for (int i = LANE; i < 256; i += 64) cnt[i] = 0u; })
    LDS_ORDER();
    for (int phase = 0; phase < 2; ++phase) {                  // 0: how many of every digit; 1: every entry to its place
        for (int i0 = 0; i0 < M; i0 += 64) {
            LV(uint32_t, d); LV(bool, on); LV(uint64_t, m); LV(int, p); LV(uint32_t, base);
            LANES({
                const int i = i0 + LANE;
                on[I_] = i < M; p[I_] = 0; d[I_] = 0u;
                if (on[I_]) { p[I_] = kFirst ? i : (int)in[i]; d[I_] = (hc_hash(src + p[I_]) >> shift) & 255u; }
            })
            hcx_match(d, on, m);
            LANES({ base[I_] = on[I_] ? cnt[d[I_]] : 0u; })
            LDS_ORDER();
            LANES({
                if (on[I_]) {
                    const uint64_t mm = m[I_];
                    if (phase) out[base[I_] + (uint32_t)__builtin_popcountll(mm & (((uint64_t)1 << LANE) - 1))] = (uint16_t)p[I_];
                    if (((mm >> LANE) >> 1) == 0) cnt[d[I_]] = base[I_] + (uint32_t)__builtin_popcountll(mm);   // (the digit's last lane)
                }
            })
            LDS_ORDER();
        }
        if (!phase) {                                          // counts -> where every digit's entries start
            LV(int, s); LV(uint32_t, c0); LV(uint32_t, c1); LV(uint32_t, c2); LV(uint32_t, c3);
            LANES({ c0[I_] = cnt[4 * LANE]; c1[I_] = cnt[4 * LANE + 1]; c2[I_] = cnt[4 * LANE + 2]; c3[I_] = cnt[4 * LANE + 3];
                    s[I_] = (int)(c0[I_] + c1[I_] + c2[I_] + c3[I_]); })
            SCAN_INCL(s);
            LDS_ORDER();
            LANES({
                const uint32_t b = (uint32_t)s[I_] - (c0[I_] + c1[I_] + c2[I_] + c3[I_]);
                cnt[4 * LANE] = b; cnt[4 * LANE + 1] = b + c0[I_]; cnt[4 * LANE + 2] = b + c0[I_] + c1[I_]; cnt[4 * LANE + 3] = b + c0[I_] + c1[I_] + c2[I_];
            })
            LDS_ORDER();
        }
    }
}
DEV void hcx_build(const uint8_t* __restrict__ src, const int n, HcxLds& L)
{
    const int M = n - 3;                                       // the positions with four bytes behind them
    hcx_sort_pass<true>(src, M, nullptr, L.rank, L.cnt, 0);    // (rank[] is the sort's second buffer first)
    hcx_sort_pass<false>(src, M, L.rank, L.list, L.cnt, 8);
    uint32_t prevH = 0; int carry = 0;
    for (int i0 = 0; i0 < M; i0 += 64) {
        LV(uint32_t, h); LV(uint32_t, hp); LV(int, p); LV(bool, on);
        LANES({
            const int i = i0 + LANE;
            on[I_] = i < M; p[I_] = 0; h[I_] = 0u;
            if (on[I_]) { p[I_] = (int)L.list[i]; h[I_] = hc_hash(src + p[I_]); }
        })
        LANES({ hp[I_] = SHFL(h, (LANE + 63) & 63); })
        const int i00 = i0; const uint32_t ph = prevH; const int cr = carry;
        const uint64_t fl = BALLOT(on[I_] && (LANE == 0 ? (i00 == 0 || h[I_] != ph) : h[I_] != hp[I_]));   // a run's first position
        LANES({
            if (on[I_]) {
                const int i = i00 + LANE;
                const uint64_t mk = fl & (((uint64_t)2 << LANE) - 1);
                const int first = mk ? i00 + 63 - (int)__builtin_clzll(mk) : cr;
                const int ord = i - first < 255 ? i - first : 255;
                L.list[i] = (uint16_t)(p[I_] | ((ord & 15) << 12));
                L.rank[p[I_]] = (uint16_t)(i | ((ord >> 4) << 12));
            }
        })
        if (fl) carry = i0 + 63 - (int)__builtin_clzll(fl);
        prevH = RL(h, 63);
    }
    LDS_ORDER();
}

// ---- (3) searches
struct HcxSearch { const uint8_t* src; const HcxLds* L; HcxDict d; int mflimit, matchlimit; };

// One round of a search: the candidates ciBase .. ciBase + nbRound of the search at `pos` (look-back down to `low`), one per lane;
// multi: of the 64 / nbRound positions pos, pos + 1, .. (first searches: no look-back, ciBase 0).  nb: the search's attempts.
// ownUsed >= 0: the own chain has been walked already and took that many attempts (every lane of the round is a dictionary
// candidate).  *more: the round's last candidate exists (there may be others behind it); *link1: an own candidate of the round has
// a link of 1.  len = the largest total of the round (0: none), first candidate first.
DEV LzFound hcx_find_round(const HcxSearch& S, const int pos, const int low, const int nb, const bool multi, const int ciBase,
                           const int nbRound, const int ownUsed, bool* more, bool* link1)
{
    const uint8_t* const src = S.src;
    const uint8_t* const iHigh = src + S.matchlimit;
    const int lookBack = pos - low;
    LV(int, p); LV(int, cl); LV(uint32_t, key); LV(int, bk); LV(int, off); LV(bool, exists); LV(bool, l1);
    LANES({
        const int g = multi ? LANE / nbRound : 0;
        cl[I_] = multi ? LANE % nbRound : LANE;
        p[I_] = pos + g;
        const int ci = ciBase + cl[I_];
        const bool act = multi ? p[I_] <= S.mflimit : LANE < nbRound;
        int total = 0; bk[I_] = 0; off[I_] = 0; exists[I_] = false; l1[I_] = false;
        if (act) {
            const uint8_t* const ipp = src + p[I_];
            const uint32_t v = ld32u(ipp);
            const uint32_t hv = (v * 2654435761u) >> 17;
            int own = ownUsed, rk = 0, ord = 0;
            if (ownUsed < 0) {
                const uint32_t r16 = S.L->rank[p[I_]];
                rk = (int)(r16 & 0xFFFu);
                ord = (int)(((r16 >> 12) << 4) | ((uint32_t)S.L->list[rk] >> 12));
                // (saturated, and the search has 256 attempts: is there a 256th position below?)
                if (ord == 255 && nb > 255 && rk >= 256 && hc_hash(src + (S.L->list[rk - 256] & 0xFFFu)) == hv) ord = 256;
                own = ord < nb ? ord : nb;
            }
            if (ci < own) {
                const int at = rk - 1 - ci;
                const int q = (int)(S.L->list[at] & 0xFFFu);
                const uint8_t* const mp = src + q;
                exists[I_] = true;
                if (link1 && at >= 1) {
                    const int qn = (int)(S.L->list[at - 1] & 0xFFFu);
                    l1[I_] = q - qn == 1 && (ci + 1 < ord || (ord >= 255 && hc_hash(src + qn) == hv));
                }
                if (ld32u(mp) == v) {                                                                 // :930
                    const int back = lookBack ? hc_count_back(ipp, mp, src + low, src) : 0;           // :933 (<= 0)
                    total = kMinMatch + hc_count(ipp + kMinMatch, mp + kMinMatch, iHigh) - back;
                    bk[I_] = back; off[I_] = p[I_] - q;
                }
            } else if (S.d.list) {
                const int k = ci - own;
                const uint32_t e0 = S.d.start[hv], e1 = S.d.start[hv + 1];
                if (k < (int)(e1 - e0)) {
                    const int dp = (int)S.d.list[e1 - 1u - (uint32_t)k];
                    const int dist = p[I_] + S.d.len - dp;                                            // :1072-1074
                    if (dist <= 65535) {
                        const uint8_t* const mp = S.d.bytes + dp;
                        exists[I_] = true;
                        if (ld32u(mp) == v) {                                                         // :1078
                            const uint8_t* vLimit = ipp + (S.d.len - dp);                             // :1080-1081
                            if (vLimit > iHigh) vLimit = iHigh;
                            const int back = lookBack ? hc_count_back(ipp, mp, src + low, S.d.bytes) : 0;   // :1083
                            total = kMinMatch + hc_count(ipp + kMinMatch, mp + kMinMatch, vLimit) - back;
                            bk[I_] = back; off[I_] = dist;
                        }
                    }
                }
            }
        }
        key[I_] = ((uint32_t)total << 6) | (uint32_t)(63 - cl[I_]);                                   // largest total, nearest candidate first
    })
    for (int m = 1; m < nbRound; m <<= 1) {
        LV(uint32_t, o);
        LANES({ o[I_] = SHFL(key, LANE ^ m); })
        LANES({ key[I_] = key[I_] > o[I_] ? key[I_] : o[I_]; })
    }
    *more = ((BALLOT(exists[I_]) >> (nbRound - 1)) & 1ull) != 0;
    if (link1) *link1 = BALLOT(l1[I_]) != 0;
    LzFound f; f.pos = -1; f.len = 0; f.off = 0; f.back = 0;
    const uint64_t hit = BALLOT(cl[I_] == 0 && (key[I_] >> 6) != 0u);
    if (hit) {
        const int l0 = multi ? ctz64(hit) : 0;
        const uint32_t kk = RL(key, l0);
        const int c = l0 + 63 - (int)(kk & 63u);
        f.pos = RL(p, l0); f.len = (int)(kk >> 6); f.off = RL(off, c); f.back = RL(bk, c);
    }
    return f;
}
// The search at `pos`: pos = -1 (len = longest): nothing longer than `longest`; pa (level 9): pos = -2 when an own candidate has
// a link of 1 -- the caller asks hcx_find_pa.
DEV LzFound hcx_find_few(const HcxSearch& S, const int pos, const int low, const int longest, const int nb, const bool multi, const bool pa)
{
    bool more = false, l1 = false, any1 = false;
    LzFound best = hcx_find_round(S, pos, low, nb, multi, 0, nb < 64 ? nb : 64, -1, &more, pa ? &l1 : nullptr);
    any1 = l1;
    for (int base = 64; base < nb && more && !any1; base += 64) {       // (128 / 256 attempts: more rounds, for the one position)
        const LzFound f = hcx_find_round(S, pos, low, nb, false, base, nb - base < 64 ? nb - base : 64, -1, &more, pa ? &l1 : nullptr);
        any1 |= l1;
        if (f.len > best.len) best = f;                                 // a later candidate replaces only when longer (:934, :1085)
    }
    if (any1) { best.pos = -2; best.len = longest; best.off = 0; best.back = 0; return best; }
    if (best.len <= longest) { best.pos = -1; best.len = longest; best.off = 0; best.back = 0; }
    return best;
}
// The general search -- level 9 when an own candidate has a link of 1, and every search of the optimal parser's levels (pattern
// analysis, and with chainSwap the chain swap): the own chain by hc_find_wider_lists over the lists in LDS (up to 63 candidates per
// round, one per lane; the reference's walk event by event), which says how many attempts it left; the dictionary's candidates
// are then read with those, one per lane -- no pattern analysis and no chain swap there (:1066-1095).
DEV HcMatch hcx_find_general(const HcxSearch& S, HcState& st, const int pos, const int low, const int longest, const int nb, const bool chainSwap)
{
    int left = 0;
    HcMatch m = hc_find_wider_lists<false, true>(st, pos, low, S.matchlimit, longest, nb, true, chainSwap, &left);
    bool more = left > 0;
    for (int base = nb - left; base < nb && more; base += 64) {
        const LzFound f = hcx_find_round(S, pos, low, nb, false, base, nb - base < 64 ? nb - base : 64, nb - left, &more, nullptr);
        if (f.len > m.len) { m.len = f.len; m.off = f.off; m.back = f.back; }
    }
    return m;
}
// LZ4HC_FindLongerMatch (:1802-1820) under the context: forward only, pattern analysis and chain swap
DEV HcMatch hcx_find_longer(const HcxSearch& S, HcState& st, const int pos, const int minLen, const int nb)
{
    HcMatch m = hcx_find_general(S, st, pos, pos, minLen, nb, true);
    if (m.len <= minLen) { m.len = 0; m.off = 0; }                                               // :1815
    return m;
}

// ---- (4) output
// LZ4HC_encodeSequence (:268-354) for the match (ml, off) at `pos` behind the literals from *anchor on; true: the output is full
DEV bool hcx_emit_seq(const uint8_t* __restrict__ src, const int pos, uint8_t* __restrict__ dst, int* op, int* anchor, const int ml,
                      const int off, const bool limited, const int oend)
{
    const int lit = pos - *anchor, an = *anchor;
    const int tok = *op, o0 = tok + 1;
    if (limited && (int64_t)o0 + lit / 255 + lit + (2 + 1 + kLastLiterals) > oend) return true;      // :283-288
    const int llx = lit >= 15 ? (lit - 15) / 255 + 1 : 0;                                              // bytes of the literals' length
    const int o1 = o0 + llx + lit;                                                                     // the offset
    const int r = ml - kMinMatch;
    wave_copy(dst + o0 + llx, src + an, lit);
    if (limited && (int64_t)o1 + 2 + r / 255 + (1 + kLastLiterals) > oend) return true;               // :323-327
    const int mlx = r >= 15 ? (r - 15) / 255 + 1 : 0;
    LANES({
        if (LANE == 0) dst[tok] = (uint8_t)(((lit < 15 ? lit : 15) << 4) | (r < 15 ? r : 15));
        if (LANE == 1) st16u(dst + o1, (uint16_t)off);
        if (LANE < llx) dst[o0 + LANE] = (uint8_t)(LANE + 1 < llx ? 255 : (lit - 15) % 255);
        if (LANE < mlx) dst[o1 + 2 + LANE] = (uint8_t)(LANE + 1 < mlx ? 255 : (r - 15) % 255);
    })
    *op = o1 + 2 + mlx;
    *anchor = pos + ml;
    return false;
}
// the last literals (:1325-1352); returns the block's size, 0 when they do not fit
DEV int hcx_last_literals(const uint8_t* __restrict__ src, const int n, const int anchor, uint8_t* __restrict__ dst, const int op, const bool limited, const int oend)
{
    const int last = n - anchor;
    const int llx = last >= 15 ? (last - 15) / 255 + 1 : 0;
    if (limited && (int64_t)op + 1 + (last + 255 - 15) / 255 + last > oend) return 0;
    LANES({
        if (LANE == 0) dst[op] = (uint8_t)((last < 15 ? last : 15) << 4);
        if (LANE < llx) dst[op + 1 + LANE] = (uint8_t)(LANE + 1 < llx ? 255 : (last - 15) % 255);
    })
    wave_copy(dst + op + 1 + llx, src + anchor, last);
    return op + 1 + llx + last;
}

// TWIN of hc_lazy_run_t (lz4hc_lazy_device.inl): the same three-state machine (lz4hc.c:1157-1306), decision for decision, with the
// finders above and bytes instead of records; that one keeps positions of a block behind a segment, segments, a hook and a record
// sink, which is why the two are not one template.  A change to the decisions belongs in both.
// LZ4_compress_HC_continue of a block of n <= 4096 bytes under an attached dictionary context, levels 3..9 (kPa: level 9).
// Returns the compressed size, 0 when it does not fit in cap.
template <bool kPa>
DEV int hcx_lazy_block(const uint8_t* __restrict__ src, const int n, uint8_t* __restrict__ dst, const int cap, const int level,
                       HcxLds& L, const HcxDict& d)
{
    const bool limited = cap < compress_bound(n);                                                // :1505-1508
    const int  maxNb = 1 << (level - 1);
    const int  mflimit = n - kMfLimit, matchlimit = n - kLastLiterals;
    const int  kOptimalMl = 15 - 1 + kMinMatch;                                                  // OPTIMAL_ML, lz4hc.c:75
    int ip = 0, anchor = 0, op = 0;
    if (n < kMinLength) return hcx_last_literals(src, n, 0, dst, 0, limited, cap);               // :1155
    hcx_build(src, n, L);
    HcxSearch S; S.src = src; S.L = &L; S.d = d; S.mflimit = mflimit; S.matchlimit = matchlimit;
    HcState st; st.src = src; st.pfx = 0; st.nextToUpdate = 0;
    st.w.hash = nullptr; st.w.chain = nullptr; st.w.opt = nullptr; st.w.pre = nullptr; st.w.rank = nullptr; st.w.list = nullptr;
    st.w.xrank = L.rank; st.w.xlist = L.list;
    st.d.mode = kHcNone; st.d.len = 0; st.d.bytes = nullptr; st.d.hash = nullptr; st.d.chain = nullptr;

    auto wider = [&](int pos, int low, int longest) {
        const LzFound f = hcx_find_few(S, pos, low, longest, maxNb, false, kPa);
        if (kPa && f.pos == -2) return hcx_find_general(S, st, pos, low, longest, maxNb, false);
        HcMatch m; m.len = f.len; m.off = f.off; m.back = f.back;
        return m;
    };
    auto put = [&](int pos, int ml, int off) { return hcx_emit_seq(src, pos, dst, &op, &anchor, ml, off, limited, cap); };

    int state = kLzFirst;
    int start0 = 0, start2 = 0, start3 = 0;
    HcMatch m0 = {0, 0, 0}, m1 = {0, 0, 0}, m2 = {0, 0, 0}, m3 = {0, 0, 0};
    for (;;) {
        if (state == kLzFirst) {
            // the literal run: the first position at or behind ip whose first search found something (:1157-1162)
            bool found = false;
            while (ip <= mflimit) {
                const LzFound f = hcx_find_few(S, ip, ip, kMinMatch - 1, maxNb, true, kPa);
                if (kPa && f.pos == -2) {
                    m1 = hcx_find_general(S, st, ip, ip, kMinMatch - 1, maxNb, false);
                    if (m1.len < kMinMatch) { ip++; continue; }
                } else {
                    if (f.pos < 0) { ip += maxNb < 64 ? 64 / maxNb : 1; continue; }
                    ip = f.pos; m1.len = f.len; m1.off = f.off; m1.back = 0;
                }
                found = true;
                break;
            }
            if (!found) break;
            start0 = ip; m0 = m1;
            state = kLzSecond;
        }
        if (state == kLzSecond) {
            // one match in hand: is there a longer one that starts inside it? (:1167-1196)
            m2.len = 0; m2.off = 0; m2.back = 0;
            if (ip + m1.len <= mflimit) {
                start2 = ip + m1.len - 2;
                m2 = wider(start2, ip, m1.len);
                start2 += m2.back;
            }
            if (m2.len <= m1.len) {                                                              // no: m1 goes out
                if (put(ip, m1.len, m1.off)) return 0;
                ip += m1.len;
                state = kLzFirst;
                continue;
            }
            if (start0 < ip && start2 < ip + m0.len) { ip = start0; m1 = m0; }                   // :1186-1189
            if (start2 - ip < 3) { ip = start2; m1 = m2; continue; }                             // m1 too short to keep: m2 takes its place
            state = kLzThird;
        }
        // kLzThird -- two overlapping matches in hand: a third one? (:1198-1306)
        if (start2 - ip < kOptimalMl) {                                                          // :1199-1210
            int newMl = m1.len;
            if (newMl > kOptimalMl) newMl = kOptimalMl;
            if (ip + newMl > start2 + m2.len - kMinMatch) newMl = (start2 - ip) + m2.len - kMinMatch;
            const int correction = newMl - (start2 - ip);
            if (correction > 0) { start2 += correction; m2.len -= correction; }
        }
        m3.len = 0; m3.off = 0; m3.back = 0;
        if (start2 + m2.len <= mflimit) {                                                        // :1212-1220
            start3 = start2 + m2.len - 3;
            m3 = wider(start3, start2, m2.len);
            start3 += m3.back;
        }
        if (m3.len <= m2.len) {                                                                  // no: m1 (cut at m2's start) and m2 go out, :1222-1240
            if (start2 < ip + m1.len) m1.len = start2 - ip;
            if (put(ip, m1.len, m1.off)) return 0;
            if (put(start2, m2.len, m2.off)) return 0;
            ip = start2 + m2.len;
            state = kLzFirst;
            continue;
        }
        if (start3 < ip + m1.len + 3) {                                                          // :1242-1270
            if (start3 >= ip + m1.len) {                                                         // m3 leaves no room for m2: m1 goes out, m3 is the match in hand
                if (start2 < ip + m1.len) {
                    const int correction = ip + m1.len - start2;
                    start2 += correction;
                    m2.len -= correction;
                    if (m2.len < kMinMatch) { start2 = start3; m2 = m3; }
                }
                if (put(ip, m1.len, m1.off)) return 0;
                ip = start3; m1 = m3;
                start0 = start2; m0 = m2;
                state = kLzSecond;
                continue;
            }
            start2 = start3; m2 = m3;                                                            // m3 swallows m2
            continue;
        }
        if (start2 < ip + m1.len) {                                                              // three in a row: m1 goes out, :1277-1306
            if (start2 - ip < kOptimalMl) {
                if (m1.len > kOptimalMl) m1.len = kOptimalMl;
                if (ip + m1.len > start2 + m2.len - kMinMatch) m1.len = (start2 - ip) + m2.len - kMinMatch;
                const int correction = m1.len - (start2 - ip);
                if (correction > 0) { start2 += correction; m2.len -= correction; }
            } else m1.len = start2 - ip;
        }
        if (put(ip, m1.len, m1.off)) return 0;
        ip = start2; m1 = m2;
        start2 = start3; m2 = m3;
    }
    return hcx_last_literals(src, n, anchor, dst, op, limited, cap);
}
// TWIN of hc_opt_run (lz4hc_lazy_device.inl; see hcx_lazy_block): a change to the price DP belongs in both.
// Levels 10..12: LZ4HC_compress_optimal (:1823-2123) as hc_opt_run walks it (lz4hc_lazy_device.inl: the price DP over a window of
// up to LZ4_OPT_NUM positions, one table entry per lane where the reference loops over lengths), with the searches above and the
// sequences written where they are decided.  opt: the wave's price table (kHcOptNum + kHcTrailing + 1 entries, device memory).
DEV int hcx_opt_block(const uint8_t* __restrict__ src, const int n, uint8_t* __restrict__ dst, const int cap, const int level,
                      HcxLds& L, const HcxDict& d, HcOpt* const opt)
{
    const bool limited = cap < compress_bound(n);                                                // :1505-1508
    const int  nbSearches = level >= 12 ? 16384 : (level == 11 ? 512 : 96);                      // table :92-106
    const int  sufficient = level >= 12 ? kHcOptNum - 1 : (level == 11 ? 128 : 64);              // (:1860: capped to LZ4_OPT_NUM - 1)
    const bool fullUpdate = level >= 12;
    const int  mflimit = n - kMfLimit, matchlimit = n - kLastLiterals;
    int ip = 0, anchor = 0, op = 0;
    if (mflimit >= 0) hcx_build(src, n, L);                                                      // (no LZ4_minLength test here: 12 bytes are searched at 0)
    HcxSearch S; S.src = src; S.L = &L; S.d = d; S.mflimit = mflimit; S.matchlimit = matchlimit;
    HcState st; st.src = src; st.pfx = 0; st.nextToUpdate = 0;
    st.w.hash = nullptr; st.w.chain = nullptr; st.w.opt = nullptr; st.w.pre = nullptr; st.w.rank = nullptr; st.w.list = nullptr;
    st.w.xrank = L.rank; st.w.xlist = L.list;
    st.d.mode = kHcNone; st.d.len = 0; st.d.bytes = nullptr; st.d.hash = nullptr; st.d.chain = nullptr;
    auto put = [&](int pos, int ml, int off) { return hcx_emit_seq(src, pos, dst, &op, &anchor, ml, off, limited, cap); };

    while (ip <= mflimit) {                                                                      // :1863
        const int llen = ip - anchor;
        int bestMl = 0, bestOff = 0, cur, last = 0;
        const HcMatch first = hcx_find_longer(S, st, ip, kMinMatch - 1, nbSearches);
        if (first.len == 0) { ip++; continue; }
        if (first.len > sufficient) {                                                            // :1871-1882
            if (put(ip, first.len, first.off)) return 0;
            ip += first.len;
            continue;
        }
        // the window's table from the first match (:1885-1919), one entry per lane
        for (int i0 = 0; i0 <= first.len + kHcTrailing; i0 += 64) {
            const int pm = hc_seq_price(llen, first.len);
            LANES({
                const int i = i0 + LANE;
                HcOpt e;
                if (i < kMinMatch) { e.mlen = 1; e.off = 0; e.litlen = llen + i; e.price = hc_lit_price(llen + i); opt[i] = e; }
                else if (i <= first.len) { e.mlen = i; e.off = first.off; e.litlen = llen; e.price = hc_seq_price(llen, i); opt[i] = e; }
                else if (i <= first.len + kHcTrailing) { e.mlen = 1; e.off = 0; e.litlen = i - first.len; e.price = pm + hc_lit_price(i - first.len); opt[i] = e; }
            })
        }
        WAVE_FENCE();
        last = first.len;
        bool direct = false;
        for (cur = 1; cur < last; ++cur) {                                                       // :1922-2019
            const int curPos = ip + cur;
            if (curPos > mflimit) break;
            if (fullUpdate) { if (opt[cur + 1].price <= opt[cur].price && opt[cur + kMinMatch].price < opt[cur].price + 3) continue; }   // :1929-1931
            else if (opt[cur + 1].price <= opt[cur].price) continue;                             // :1932-1934
            const HcMatch nm = hcx_find_longer(S, st, curPos, fullUpdate ? kMinMatch - 1 : last - cur, nbSearches);
            if (!nm.len) continue;
            if (nm.len > sufficient || nm.len + cur >= kHcOptNum) {                              // :1948-1956
                bestMl = nm.len; bestOff = nm.off; last = cur + 1; direct = true;
                break;
            }
            {   const int baseLit = opt[cur].litlen;                                             // :1958-1972
                for (int l = 1; l < kMinMatch; ++l) {
                    const int price = opt[cur].price - hc_lit_price(baseLit) + hc_lit_price(baseLit + l);
                    const int pos = cur + l;
                    if (price < opt[pos].price) { opt[pos].mlen = 1; opt[pos].off = 0; opt[pos].litlen = baseLit + l; opt[pos].price = price; }
                }
            }
            {   // every length of the match, one per lane (:1974-2009: each reads and writes its own entry; `last` moves at the last one)
                const int ll = (opt[cur].mlen == 1) ? opt[cur].litlen : 0;
                const int basePrice = (opt[cur].mlen == 1) ? ((cur > ll) ? opt[cur - ll].price : 0) : opt[cur].price;
                const int lastOld = last;
                for (int ml0 = kMinMatch; ml0 <= nm.len; ml0 += 64) {
                    LV(int, took);
                    LANES({
                        const int ml = ml0 + LANE;
                        took[I_] = 0;
                        if (ml <= nm.len) {
                            const int pos = cur + ml;
                            const int price = basePrice + hc_seq_price(ll, ml);
                            if (pos > lastOld + kHcTrailing || price <= opt[pos].price) {
                                took[I_] = 1;
                                opt[pos].mlen = ml; opt[pos].off = nm.off; opt[pos].litlen = ll; opt[pos].price = price;
                            }
                        }
                    })
                    if (nm.len - ml0 < 64) {
                        const int lastLane = nm.len - ml0;
                        if (RL(took, lastLane) && lastOld < cur + nm.len) last = cur + nm.len;
                    }
                }
            }
            for (int a = 1; a <= kHcTrailing; ++a) {                                             // :2011-2018
                opt[last + a].mlen = 1; opt[last + a].off = 0; opt[last + a].litlen = a;
                opt[last + a].price = opt[last].price + hc_lit_price(a);
            }
        }
        if (!direct) { bestMl = opt[last].mlen; bestOff = opt[last].off; cur = last - bestMl; }   // :2022-2024
        {   // the chosen path, marked backwards (:2026-2046) ...
            int cand = cur, selML = bestMl, selOff = bestOff;
            for (;;) {
                const int nextML = opt[cand].mlen, nextOff = opt[cand].off;
                opt[cand].mlen = selML; opt[cand].off = selOff;
                selML = nextML; selOff = nextOff;
                if (nextML > cand) break;
                cand -= nextML;
            }
        }
        {   // ... and its sequences in order (:2048-2064)
            int r = 0;
            while (r < last) {
                const int ml = opt[r].mlen, off = opt[r].off;
                if (ml == 1) { ip++; r++; continue; }
                r += ml;
                if (put(ip, ml, off)) return 0;
                ip += ml;
            }
        }
    }
    return hcx_last_literals(src, n, anchor, dst, op, limited, cap);                             // :2067-2098
}
// ---- level 2: LZ4MID_compress (:521-775) under the context.  hc_mid_parse (lz4hc_lazy_device.inl) as it runs on independent
// blocks -- batches of a literal run over the two tables -- with the dictionary step (:652-665) through its Ctx policy and the two
// tables in LDS.  The reference's tables are direct-mapped by a 14-bit hash, 2 x 16384 entries; a block of at most 4 KiB only ever
// touches the hashes of its own positions, at most 4096 per table.  So per table: a bitmap of the hashes the block's positions have
// (2 KiB) with the number of set bits in front of every 64-bit word (512 B) turns a hash into a dense number -- exactly, no
// probing, no tags -- and the entries are 16-bit (index - 64 KiB + 1; 0: empty) in an array of 4096: 10.5 KiB per table, 21 KiB per
// wave (seven waves per CU).  Built by all lanes: one LDS atomic OR per position and table, one scan.
struct HcxMidLds { uint64_t bits[2][256]; uint16_t base[2][256]; uint16_t val[2][kHcxMaxBlock]; };
#if defined(PLZ4_EMU)
static inline void lds_or64(uint64_t* p, uint64_t v) { *p |= v; }
#else
__device__ __forceinline__ void lds_or64(uint64_t* p, uint64_t v) { atomicOr((unsigned long long*)p, (unsigned long long)v); }
#endif
struct HcxMidTab {
    const uint64_t* bits; const uint16_t* base; uint16_t* val;
    struct Ref {
        uint16_t* p;
        DEVM operator uint32_t() const { const uint32_t v = *p; return v ? v - 1u + kHcBase : 0u; }
        DEVM void operator=(uint32_t idx) const { *p = (uint16_t)(idx - kHcBase + 1u); }
    };
    DEVM Ref operator[](uint32_t h) const
    {
        const uint32_t w = h >> 6;
        Ref r; r.p = val + base[w] + (uint32_t)__builtin_popcountll(bits[w] & (((uint64_t)1 << (h & 63u)) - 1));
        return r;
    }
};
DEV void hcx_mid_build(const uint8_t* __restrict__ src, const int n, HcxMidLds& L)
{
    LANES({
        for (int i = LANE; i < 256; i += 64) { L.bits[0][i] = 0; L.bits[1][i] = 0; }
        uint32_t* const v = (uint32_t*)&L.val[0][0];
        for (int i = LANE; i < kHcxMaxBlock; i += 64) v[i] = 0u;               // (2 x 4096 16-bit entries)
    })
    LDS_ORDER();
    LANES({
        for (int p = LANE; p + 4 <= n; p += 64) {
            const uint32_t h4 = mid_hash4(src + p);
            lds_or64(&L.bits[0][h4 >> 6], (uint64_t)1 << (h4 & 63u));
            if (p + 8 <= n) { const uint32_t h8 = mid_hash8(src + p); lds_or64(&L.bits[1][h8 >> 6], (uint64_t)1 << (h8 & 63u)); }
        }
    })
    LDS_ORDER();
    for (int t = 0; t < 2; ++t) {
        LV(int, s); LV(int, c0); LV(int, c1); LV(int, c2);
        LANES({
            c0[I_] = __builtin_popcountll(L.bits[t][4 * LANE]); c1[I_] = __builtin_popcountll(L.bits[t][4 * LANE + 1]);
            c2[I_] = __builtin_popcountll(L.bits[t][4 * LANE + 2]);
            s[I_] = c0[I_] + c1[I_] + c2[I_] + __builtin_popcountll(L.bits[t][4 * LANE + 3]);
        })
        LV(int, tot);
        LANES({ tot[I_] = s[I_]; })
        SCAN_INCL(s);
        LANES({
            const int b = s[I_] - tot[I_];
            L.base[t][4 * LANE] = (uint16_t)b; L.base[t][4 * LANE + 1] = (uint16_t)(b + c0[I_]);
            L.base[t][4 * LANE + 2] = (uint16_t)(b + c0[I_] + c1[I_]); L.base[t][4 * LANE + 3] = (uint16_t)(b + c0[I_] + c1[I_] + c2[I_]);
        })
    }
    LDS_ORDER();
}
// seq: room for the block's sequence records in device memory (at most n / 4 + 64 of 8 bytes), read back 64 at a time
DEV int hcx_mid_block(const uint8_t* __restrict__ src, const int n, uint8_t* __restrict__ dst, const int cap, HcxMidLds& L, const HcxDict& d,
                      const uint32_t* dictMidTables, uint64_t* seq)
{
    const bool limited = cap < compress_bound(n);
    int lastAnchor = 0, nseq = 0;
    if (n >= kMinLength) {
        hcx_mid_build(src, n, L);
        HcxMidTab t4; t4.bits = L.bits[0]; t4.base = L.base[0]; t4.val = L.val[0];
        HcxMidTab t8; t8.bits = L.bits[1]; t8.base = L.base[1]; t8.val = L.val[1];
        MidDictCtx ctx; ctx.d.mode = kHcCtx; ctx.d.len = d.len; ctx.d.bytes = d.bytes; ctx.d.hash = dictMidTables; ctx.d.chain = nullptr;
        nseq = hc_mid_parse<false, HcxMidTab, MidDictCtx>(src, n, t4, t8, seq, &lastAnchor, 0, ctx);
        WAVE_FENCE();
    }
    int op = 0, anchor = 0;
    for (int i0 = 0; i0 < nseq; i0 += 64) {
        LV(uint64_t, r);
        LANES({ r[I_] = i0 + LANE < nseq ? seq[i0 + LANE] : 0ull; })
        for (int k = 0; k < 64 && i0 + k < nseq; ++k) {
            const uint64_t e = RL(r, k);
            if (hcx_emit_seq(src, (int)seq_pos(e), dst, &op, &anchor, (int)seq_fwd(e) + kMinMatch, (int)seq_off(e), limited, cap)) return 0;
        }
    }
    return hcx_last_literals(src, n, anchor, dst, op, limited, cap);
}

DEV int hcx_compress(const uint8_t* __restrict__ src, const int n, uint8_t* __restrict__ dst, const int cap, const int level, HcxLds& L, const HcxDict& d,
                     HcOpt* const opt)
{
    if (level >= 10) return hcx_opt_block(src, n, dst, cap, level, L, d, opt);
    if ((1 << (level - 1)) > 128) return hcx_lazy_block<true>(src, n, dst, cap, level, L, d);     // pattern analysis above 128 attempts
    return hcx_lazy_block<false>(src, n, dst, cap, level, L, d);
}

}  // namespace plz4
