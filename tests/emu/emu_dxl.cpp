// Lane-emulation harness of the few-block decoder for blocks with history outside the block (dxl_* in
// plz4_amd/csrc/lz4_dx_device.inl): the stage train over ONE call of several blocks as the kernels run it (tests/emu/dx_train.h: the
// fill writes sources in front of a block as tagged distances, the resolve pass goes over the whole pointer space, the jump rounds
// follow the call's output), and per chain the good prefix, the window it leaves and the one-wave walk from the
// first block that is not plainly good (k_dxl_finish / linked_walk; k_dxl_verdict + k_decode_raw_dict for chains of one under a
// dictionary).  Test infrastructure only: built into tests/emu/_build/, never loaded by plz4_amd, not a CPU fallback.
#define PLZ4_EMU 1
#include "dx_train.h"

int plz4_emu_descending = 0;

using namespace plz4;

extern "C" void emu_dxl_set_descending(int d) { plz4_emu_descending = d; }

// One call.  Block i: payload src[i] of len[i] bytes, stored[i] != 0: a stored block (copied out, not in the window), capacity cap[i];
// first[i]: the first block of its chain, chain[i]: the chain's number.  hist: nCh x 65536 bytes, chain ch's incoming history in the
// first histLen[ch] of its 64 KiB.  linked != 0: chains of linked blocks (windows handed back in hist / histLen); 0: chains of one.
// Out: dst (nb x dstStride), result[i] (bytes, or liblz4's negative code), status[i] (0 ok, 1 corrupt), taken[i] (1: answered by the
// few-block path, 0: by the one-wave walk), *roundsOut (jump rounds until the slowest taken block came to rest, + 1).
extern "C" int emu_dxl_decode(int nb, const uint8_t* const* src, const int32_t* len, const int32_t* stored, const int32_t* cap,
                              const int32_t* first, const int32_t* chain, int nCh, uint8_t* hist, int32_t* histLen, int linked,
                              uint8_t* dst, int64_t dstStride, int32_t* result, int32_t* status, int32_t* taken, int* roundsOut, int roundsForced)
{
    int maxIn = 1, maxCap = 1;
    for (int i = 0; i < nb; ++i) { if (len[i] > maxIn) maxIn = len[i]; if (cap[i] > maxCap) maxCap = cap[i]; }
    std::vector<int32_t> dxLen(nb);
    // two halves per chain, as the kernels' window buffers are
    std::vector<uint8_t> win((size_t)(nCh > 0 ? nCh : 1) * 131072, 0);
    std::vector<int> winLen(nCh > 0 ? nCh : 1, 0);
    for (int ch = 0; ch < nCh; ++ch) { memcpy(&win[(size_t)ch * 131072], hist + (size_t)ch * 65536, 65536); winLen[ch] = histLen[ch]; }
    for (int i = 0; i < nb; ++i) dxLen[i] = stored[i] ? -1 : len[i];
    DxlCall c{};
    c.first = first; c.chain = chain;
    if (linked) { c.hist = win.data(); c.histStride = 131072; c.histLen = winLen.data(); c.histLenAll = 0; }
    else { c.hist = win.data(); c.histStride = 0; c.histLen = nullptr; c.histLenAll = winLen[0]; }
    DxEmuTrain t;
    dx_emu_train(DxlF{}, t, DxEmuCall{nb, src, dxLen.data(), cap, dst, dstStride}, c, nb, maxIn, maxCap, false, 0, [] {}, roundsForced);
    if (t.disagree) return kDxEmuUnitsDisagree;
    const DxInfo* const info = t.info; const uint32_t* const moved = t.moved; const int rounds = t.launched;
    auto good = [&](int b) { return dxLen[b] >= 0 && !info[b].bad && dxl_converged(moved + (size_t)b * (kDxlMaxRounds + 1), rounds); };
    int roundsSeen = 0;
    auto note = [&](int b) { const int rr = dxl_rounds_of(moved + (size_t)b * (kDxlMaxRounds + 1), rounds); if (rr > roundsSeen) roundsSeen = rr; };
    if (!linked) {
        // k_dxl_verdict, then k_decode_raw_dict for the rest
        for (int b = 0; b < nb; ++b) {
            status[b] = 0;
            if (good(b)) { taken[b] = 1; result[b] = info[b].outLen; note(b); continue; }
            taken[b] = 0;
            result[b] = wave_decode_block(src[b], len[b], dst + (int64_t)b * dstStride, cap[b], winLen[0] > 0 ? win.data() : nullptr, winLen[0]);
        }
    } else {
        // k_dxl_finish per chain
        for (int ch = 0; ch < nCh; ++ch) {
            int f = nb, l = 0;
            for (int b = 0; b < nb; ++b) if (chain[b] == ch) { if (b < f) f = b; l = b + 1; }
            if (f >= l) continue;
            uint8_t* const win0 = &win[(size_t)ch * 131072];
            uint8_t* winA = win0; uint8_t* winB = win0 + 65536;
            int wl = winLen[ch], i = f;
            for (; i < l; ++i) {
                if (dxLen[i] >= 0) {
                    if (!good(i)) break;
                    result[i] = info[i].outLen; status[i] = 0; taken[i] = 1; note(i);
                } else {
                    taken[i] = 0; status[i] = 0; result[i] = len[i];
                    memcpy(dst + (int64_t)i * dstStride, src[i], (size_t)len[i]);
                }
            }
            const int t = dxl_window(c, f, i, winA, wl, winB);
            if (t >= 0) { uint8_t* x = winA; winA = winB; winB = x; wl = t; }
            // linked_walk
            bool dead = false;
            for (; i < l; ++i) {
                taken[i] = 0;
                int r = 0, st = 1;
                if (!dead) {
                    uint8_t* out = dst + (int64_t)i * dstStride;
                    if (stored[i]) { memcpy(out, src[i], (size_t)len[i]); result[i] = len[i]; status[i] = 0; continue; }
                    r = wave_decode_block(src[i], len[i], out, cap[i], winA, wl);
                    st = r < 0 ? 1 : 0;                                     // (the result stays liblz4's code, as decode_one_record leaves it)
                }
                result[i] = r; status[i] = st;
                if (st) { dead = true; continue; }
                const uint8_t* out = dst + (int64_t)i * dstStride;
                if (r >= 65536) { memcpy(winB, out + (r - 65536), 65536); wl = 65536; }
                else {
                    int keep = wl;
                    if (wl + r > 65536) keep = 65536 - r;
                    memcpy(winB, winA + (wl - keep), (size_t)keep);
                    memcpy(winB + keep, out, (size_t)r);
                    wl = keep + r;
                }
                uint8_t* x = winA; winA = winB; winB = x;
            }
            memcpy(hist + (size_t)ch * 65536, winA, (size_t)wl);
            histLen[ch] = wl;
        }
    }
    if (roundsOut) *roundsOut = roundsSeen;
    return 0;
}
