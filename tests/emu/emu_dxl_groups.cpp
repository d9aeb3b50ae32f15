// Lane-emulation harness of a LINKED decode call cut into groups of consecutive blocks (launch_decode in plz4_amd/csrc/plz4hip.hip;
// dxl_* in plz4_amd/csrc/lz4_dx_device.inl): the call's plan (dxl_group), and per group the stage train over the group's view of the
// call -- record prep and checksums, tables, stitch, fill, resolve, jump rounds sized by the group's output, gather -- then per
// chain the finish stage (dxl_finish, the body k_dxl_finish runs) with the window, its length and the chain's dead word carried from
// group to group.  Test infrastructure only: built into tests/emu/_build/, never loaded by plz4_amd, not a CPU fallback.
#define PLZ4_EMU 1
#include "../../plz4_amd/csrc/lz4_dx_device.inl"
#include <stdlib.h>
#include <string.h>
#include <vector>

int plz4_emu_descending = 0;

using namespace plz4;

extern "C" void emu_dxlg_set_descending(int d) { plz4_emu_descending = d; }

namespace {
enum { kOk = 0, kHashMismatch = 1, kSizeOverflow = 2, kCorrupt = 3 };       // PLZ4HIP_BLK_*

// the group's view of the call, as launch_decode makes it
struct View {
    const uint8_t* const* rec; const int32_t* recLen; int nb; int bsz, blockChecksum, dstCap;
    uint8_t* dst; int64_t dstStride; int32_t* result; int32_t* status;
};
// decode_one_record: one record the serial way
struct RecEmu {
    const View& v;
    void operator()(int i, const uint8_t* hist, int histLen, int* rOut, int* stOut, bool* stored) const
    {
        const uint8_t* rec = v.rec[i]; const int64_t recLen = v.recLen[i];
        uint8_t* out = v.dst + (int64_t)i * v.dstStride;
        const uint32_t word = ld32u(rec);
        const int sz = (int)(word & 0x7FFFFFFFu);
        int st = kOk, r = 0;
        *stored = false;
        if (sz > v.bsz || (int64_t)sz + 4 + (v.blockChecksum ? 4 : 0) > recLen) st = kSizeOverflow;
        else {
            if (v.blockChecksum && wave_xxh32(rec + 4, sz) != ld32u(rec + 4 + sz)) st = kHashMismatch;
            if (st == kOk) {
                if (word & 0x80000000u) {
                    if (sz > v.dstCap) st = kSizeOverflow;
                    else { wave_copy(out, rec + 4, sz); r = sz; *stored = true; }
                } else {
                    r = wave_decode_block(rec + 4, sz, out, v.dstCap, hist, histLen);
                    if (r < 0) st = kCorrupt;
                }
            }
        }
        *rOut = r; *stOut = st;
    }
};
}  // namespace

// One call.  Record i: rec[i], recLen[i] bytes ([LE32 size | stored bit][payload][LE32 xxh32?]).  chainFirst: nCh + 1 entries.
// windows: nCh x 131072 (the live window in the first 64 KiB), windowLen[nCh]: in/out.  group: blocks per group (>= nb: one group).
// forcedRounds: per group, the jump rounds to launch instead of the plan's (0 / null: the plan's) -- too few leave the group's
// blocks unconverged: valid blocks the path does not answer for.
// Out: dst, result, status, taken[i] (1: answered by the few-block path), counters: [0] blocks taken, [1] the maximum over the
// groups of the jump rounds their slowest taken block took, [2] groups.
extern "C" int emu_dxlg_decode(int nb, const uint8_t* const* rec, const int32_t* recLen, int bsz, int blockChecksum,
                               int nCh, const int32_t* chainFirst, uint8_t* windows, int32_t* windowLen,
                               int group, const int32_t* forcedRounds, uint8_t* dst, int64_t dstStride, int dstCap,
                               int32_t* result, int32_t* status, int32_t* taken, int64_t* counters)
{
    const int64_t outB = dstCap < kDxMaxOut ? dstCap : kDxMaxOut;
    const int64_t P = (outB + 64 + 1023) / 1024 * 1024, tStride = ((int64_t)bsz + 64 + 63) / 64 * 64;
    const int maxSeg = dx_segments(bsz);
    const int G = group < nb ? group : nb;
    std::vector<uint8_t> in((size_t)G * tStride, 0);
    std::vector<uint64_t> T((size_t)G * tStride, 0);
    std::vector<DxUnit> units((size_t)G * (maxSeg + 1));
    std::vector<DxInfo> info(G);
    std::vector<uint32_t> ptr((size_t)G * P);
    std::vector<int32_t> dxLen(G), hashBad(G), first(G), chain(G);
    std::vector<uint32_t> moved((size_t)G * (kDxlMaxRounds + 1));
    std::vector<int32_t> dead(nCh, 0);
    counters[0] = counters[1] = counters[2] = 0;
    for (int i = 0; i < nb; ++i) taken[i] = 0;

    int chCursor = 0, gi = 0;
    for (int g0 = 0; g0 < nb; g0 += G, ++gi) {
        DxlGroup g;
        dxl_group(chainFirst, nCh, nb, G, g0, &chCursor, &g);
        const int ng = g.g1 - g.g0, nChG = g.ch1 - g.ch0;
        // the group's view: every pointer moved to the group's first block / first chain, chainFirst stays the call's
        View v{rec + g.g0, recLen + g.g0, ng, bsz, blockChecksum, dstCap, dst + (int64_t)g.g0 * dstStride, dstStride, result + g.g0, status + g.g0};
        const int32_t* const cf = chainFirst + g.ch0;
        uint8_t* const win = windows + (size_t)g.ch0 * 131072;
        int32_t* const winLen = windowLen + g.ch0;
        // k_dx_rec_prep, k_dx_rec_hash
        for (int i = 0; i < ng; ++i) {
            int n = -1;
            if (v.recLen[i] >= 4) {
                const uint32_t word = ld32u(v.rec[i]); const int sz = (int)(word & 0x7FFFFFFFu);
                if (!(word & 0x80000000u) && sz <= bsz && (int64_t)sz + 4 + (blockChecksum ? 4 : 0) <= v.recLen[i]) n = sz;
            }
            dxLen[i] = n; hashBad[i] = 0;
            memset(&in[(size_t)i * tStride], 0, (size_t)tStride);
            if (n > 0) memcpy(&in[(size_t)i * tStride], v.rec[i] + 4, (size_t)n);
            if (n >= 0 && blockChecksum) hashBad[i] = wave_xxh32(v.rec[i] + 4, n) != ld32u(v.rec[i] + 4 + n);
            for (int64_t p = 0; p < P; ++p) ptr[(size_t)i * P + p] = (uint32_t)p;
            for (int r = 0; r <= kDxlMaxRounds; ++r) moved[(size_t)i * (kDxlMaxRounds + 1) + r] = 0;
        }
        // k_dxl_link
        for (int i = 0; i < ng; ++i) {
            int ch = 0;
            while (ch + 1 < nChG && dxl_chain_lo(cf, g.g0, ng, ch + 1) <= i) ++ch;
            first[i] = dxl_chain_lo(cf, g.g0, ng, ch); chain[i] = ch;
        }
        DxlCall c;
        c.ptr = ptr.data(); c.P = P; c.nb = ng; c.info = info.data(); c.len = dxLen.data(); c.first = first.data(); c.chain = chain.data();
        c.hist = win; c.histStride = 131072; c.histLen = winLen; c.histLenAll = 0;
        c.dst = v.dst; c.dstStride = dstStride;
        // k_dx_tables, k_dx_stitch, k_dxl_fill
        for (int b = 0; b < ng; ++b) {
            const uint8_t* s = &in[(size_t)b * tStride]; const int n = dxLen[b];
            const int nseg = dx_segments(n), jt = dx_tail_from(nseg);
            DxUnit* u = &units[(size_t)b * (maxSeg + 1)];
            info[b].bad = 1; info[b].outLen = 0; info[b].tailFrom = jt;
            if (n <= 0) continue;
            for (int j = nseg - 1; j >= 0; --j) dx_segment_table(s, n, j, &T[(size_t)b * tStride]);
            if (dstCap > P - 64 || dx_stitch(s, n, dstCap, &T[(size_t)b * tStride], u, nseg) != 0) continue;
            bool bad = false;
            for (int j = jt; j >= 0 && !bad; --j) {
                if (j < jt && u[j].ip < 0) continue;
                const int64_t r = wave_dx_fill<true>(s, n, v.dst + (int64_t)b * dstStride, dstCap, &ptr[(size_t)b * P], u[j].ip, u[j].op, u[j].stop, j == jt);
                if (r < 0) { bad = true; break; }
                if (j == jt) info[b].outLen = (int)r;
                else { int k = j + 1; while (k < jt && u[k].ip < 0) ++k; if (u[k].op != (int)r) return -888888; }
            }
            info[b].bad = bad ? 1 : 0;
        }
        // k_dxl_resolve over every entry of every block
        for (int b = ng - 1; b >= 0; --b)
            for (int64_t p0 = 0; p0 < P; p0 += 256) if (!dxl_resolve(c, b, (int)p0, (int)P)) info[b].bad = 1;
        // the jump rounds follow the group's own output
        int rounds = 1;
        while (rounds < kDxlMaxRounds && ((int64_t)1 << (rounds - 1)) < (int64_t)ng * outB + kDxlHist) ++rounds;
        if (forcedRounds && forcedRounds[gi] > 0) rounds = forcedRounds[gi];
        const uint32_t hist0 = dxl_hist0(c);
        for (int r = 0; r < rounds; ++r)
            for (int b = ng - 1; b >= 0; --b) {
                uint32_t* mv = &moved[(size_t)b * (kDxlMaxRounds + 1)];
                if (info[b].bad || (r > 0 && !mv[r - 1])) continue;
                const int outLen = info[b].outLen;
                for (int p0 = outLen > 0 ? ((outLen - 1) / 256) * 256 : -1; p0 >= 0; p0 -= 256)
                    if (dxl_jump(c.ptr, hist0, (uint32_t)((int64_t)b * P), p0, outLen)) mv[r] = 1u;
            }
        for (int b = 0; b < ng; ++b) {
            if (info[b].bad) continue;
            for (int p0 = 0; p0 < info[b].outLen; p0 += 256) dxl_gather(c, b, p0, info[b].outLen);
        }
        // k_dxl_finish: one wave per chain of the group
        DxlFin f; f.hashBad = blockChecksum ? hashBad.data() : nullptr; f.moved = moved.data(); f.rounds = rounds; f.result = v.result; f.status = v.status;
        RecEmu recEmu{v};
        for (int ch = nChG - 1; ch >= 0; --ch) {
            const int lo = dxl_chain_lo(cf, g.g0, ng, ch), hi = dxl_chain_lo(cf, g.g0, ng, ch + 1);
            if (lo >= hi) continue;
            int wl = winLen[ch], dd = dead[g.ch0 + ch], tk = 0, rr = 0;
            dxl_finish(c, f, recEmu, lo, hi, win + (size_t)ch * 131072, &wl, &dd, &tk, &rr);
            winLen[ch] = wl; dead[g.ch0 + ch] = dd;
            if (tk) { counters[0] += tk; if (rr > counters[1]) counters[1] = rr; }
            // which blocks the path answered: the chain's compressed blocks up to the count dxl_finish gives
            for (int i = lo; i < hi && tk > 0; ++i) if (dxLen[i] >= 0) { taken[g.g0 + i] = 1; --tk; }
        }
    }
    counters[2] = gi;
    return 0;
}
