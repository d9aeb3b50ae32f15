// Lane-emulation harness of a LINKED decode call cut into groups of consecutive blocks (launch_decode in plz4_amd/csrc/plz4hip.hip;
// dxl_* in plz4_amd/csrc/lz4_dx_device.inl): the call's plan (dxl_group), and per group the stage train over the group's view of the
// call -- record prep and checksums, then the stages of dx_train.h with the jump rounds sized by the group's output -- then per
// chain the finish stage (dxl_finish, the body k_dxl_finish runs) with the window, its length and the chain's dead word carried from
// group to group.  Test infrastructure only: built into tests/emu/_build/, never loaded by plz4_amd, not a CPU fallback.
#define PLZ4_EMU 1
#include "dx_train.h"

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
    const int G = group < nb ? group : nb;
    std::vector<const uint8_t*> src(G);
    std::vector<int32_t> dxLen(G), hashBad(G), first(G), chain(G), caps(G, dstCap);
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
            src[i] = v.rec[i] + 4;
            if (n >= 0 && blockChecksum) hashBad[i] = wave_xxh32(v.rec[i] + 4, n) != ld32u(v.rec[i] + 4 + n);
        }
        // k_dxl_link
        for (int i = 0; i < ng; ++i) {
            int ch = 0;
            while (ch + 1 < nChG && dxl_chain_lo(cf, g.g0, ng, ch + 1) <= i) ++ch;
            first[i] = dxl_chain_lo(cf, g.g0, ng, ch); chain[i] = ch;
        }
        DxlCall c{};
        c.first = first.data(); c.chain = chain.data();
        c.hist = win; c.histStride = 131072; c.histLen = winLen; c.histLenAll = 0;
        // the group's layout, as launch_decode's layout_for(ng) makes it; the jump rounds follow the group's own output
        DxEmuTrain t;
        dx_emu_train(DxlF{}, t, DxEmuCall{ng, src.data(), dxLen.data(), caps.data(), v.dst, dstStride}, c, G, bsz, dstCap, true, nCh, [] {},
                     forcedRounds ? forcedRounds[gi] : 0);
        if (t.disagree) return kDxEmuUnitsDisagree;
        const int rounds = t.launched;
        // k_dxl_finish: one wave per chain of the group
        DxlFin f; f.hashBad = blockChecksum ? hashBad.data() : nullptr; f.moved = t.moved; f.rounds = rounds; f.result = v.result; f.status = v.status;
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
