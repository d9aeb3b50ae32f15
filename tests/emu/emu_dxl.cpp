// Lane-emulation harness of the few-block decoder for blocks with history outside the block (dxl_* in
// plz4_amd/csrc/lz4_dx_device.inl): the stages over ONE call of several blocks as the kernels run them -- tables and stitch per
// block, the fill that writes sources in front of a block as tagged distances, the resolve pass over the whole pointer space, jump
// rounds sized by the call's output, gather, and per chain the good prefix, the window it leaves and the one-wave walk from the
// first block that is not plainly good (k_dxl_finish / linked_walk; k_dxl_verdict + k_decode_raw_dict for chains of one under a
// dictionary).  Test infrastructure only: built into tests/emu/_build/, never loaded by plz4_amd, not a CPU fallback.
#define PLZ4_EMU 1
#include "../../plz4_amd/csrc/lz4_dx_device.inl"
#include <stdlib.h>
#include <string.h>
#include <vector>

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
    const int64_t P = ((int64_t)maxCap + 64 + 1023) / 1024 * 1024, tStride = (int64_t)maxIn + 64;
    const int maxSeg = dx_segments(maxIn);
    std::vector<uint8_t> in((size_t)nb * tStride, 0);
    std::vector<uint64_t> T((size_t)nb * tStride, 0);
    std::vector<DxUnit> units((size_t)nb * (maxSeg + 1));
    std::vector<DxInfo> info(nb);
    std::vector<uint32_t> ptr((size_t)nb * P);
    std::vector<int32_t> dxLen(nb);
    std::vector<uint32_t> moved((size_t)nb * (kDxlMaxRounds + 1), 0);
    // two halves per chain, as the kernels' window buffers are
    std::vector<uint8_t> win((size_t)(nCh > 0 ? nCh : 1) * 131072, 0);
    std::vector<int> winLen(nCh > 0 ? nCh : 1, 0);
    for (int ch = 0; ch < nCh; ++ch) { memcpy(&win[(size_t)ch * 131072], hist + (size_t)ch * 65536, 65536); winLen[ch] = histLen[ch]; }
    for (int i = 0; i < nb; ++i) {
        dxLen[i] = stored[i] ? -1 : len[i];
        if (len[i] > 0) memcpy(&in[(size_t)i * tStride], src[i], (size_t)len[i]);
        for (int64_t p = 0; p < P; ++p) ptr[(size_t)i * P + p] = (uint32_t)p;
    }
    DxlCall c;
    c.ptr = ptr.data(); c.P = P; c.nb = nb; c.info = info.data(); c.len = dxLen.data(); c.first = first; c.chain = chain;
    if (linked) { c.hist = win.data(); c.histStride = 131072; c.histLen = winLen.data(); c.histLenAll = 0; }
    else { c.hist = win.data(); c.histStride = 0; c.histLen = nullptr; c.histLenAll = winLen[0]; }
    c.dst = dst; c.dstStride = dstStride;
    // k_dx_tables, k_dx_stitch, k_dxl_fill
    for (int b = 0; b < nb; ++b) {
        const uint8_t* s = &in[(size_t)b * tStride]; const int n = dxLen[b];
        const int nseg = dx_segments(n), jt = dx_tail_from(nseg);
        DxUnit* u = &units[(size_t)b * (maxSeg + 1)];
        info[b].bad = 1; info[b].outLen = 0; info[b].tailFrom = jt;
        if (n <= 0) continue;
        for (int j = nseg - 1; j >= 0; --j) dx_segment_table(s, n, j, &T[(size_t)b * tStride]);
        if (cap[b] > P - 64 || dx_stitch(s, n, cap[b], &T[(size_t)b * tStride], u, nseg) != 0) continue;
        bool bad = false;
        for (int j = jt; j >= 0 && !bad; --j) {
            if (j < jt && u[j].ip < 0) continue;
            const int64_t r = wave_dx_fill<true>(s, n, dst + (int64_t)b * dstStride, cap[b], &ptr[(size_t)b * P], u[j].ip, u[j].op, u[j].stop, j == jt);
            if (r < 0) { bad = true; break; }
            if (j == jt) info[b].outLen = (int)r;
            else { int k = j + 1; while (k < jt && u[k].ip < 0) ++k; if (u[k].op != (int)r) return -888888; }
        }
        info[b].bad = bad ? 1 : 0;
    }
    // k_dxl_resolve over every entry of every block
    for (int b = nb - 1; b >= 0; --b)
        for (int64_t p0 = 0; p0 < P; p0 += 256) if (!dxl_resolve(c, b, (int)p0, (int)P)) info[b].bad = 1;
    // the jump rounds (launch_decode's count, or the test's)
    int64_t total = kDxlHist;
    for (int b = 0; b < nb; ++b) total += maxCap;
    int rounds = 1;
    while (rounds < kDxlMaxRounds && ((int64_t)1 << (rounds - 1)) < total) ++rounds;
    if (roundsForced > 0) rounds = roundsForced;
    const uint32_t hist0 = dxl_hist0(c);
    for (int r = 0; r < rounds; ++r)
        for (int b = nb - 1; b >= 0; --b) {                                 // (from the top down: the slowest order the kernel's workgroups can take)
            uint32_t* mv = &moved[(size_t)b * (kDxlMaxRounds + 1)];
            if (info[b].bad || (r > 0 && !mv[r - 1])) continue;
            const int outLen = info[b].outLen;
            for (int p0 = outLen > 0 ? ((outLen - 1) / 256) * 256 : -1; p0 >= 0; p0 -= 256)
                if (dxl_jump(c.ptr, hist0, (uint32_t)((int64_t)b * P), p0, outLen)) mv[r] = 1u;
        }
    for (int b = 0; b < nb; ++b) {
        if (info[b].bad) continue;
        for (int p0 = 0; p0 < info[b].outLen; p0 += 256) dxl_gather(c, b, p0, info[b].outLen);
    }
    auto good = [&](int b) { return dxLen[b] >= 0 && !info[b].bad && dxl_converged(&moved[(size_t)b * (kDxlMaxRounds + 1)], rounds); };
    int roundsSeen = 0;
    auto note = [&](int b) { const int rr = dxl_rounds_of(&moved[(size_t)b * (kDxlMaxRounds + 1)], rounds); if (rr > roundsSeen) roundsSeen = rr; };
    if (!linked) {
        // k_dxl_verdict, then k_decode_raw_dict for the rest
        for (int b = 0; b < nb; ++b) {
            status[b] = 0;
            if (good(b)) { taken[b] = 1; result[b] = info[b].outLen; note(b); continue; }
            taken[b] = 0;
            result[b] = wave_decode_block(&in[(size_t)b * tStride], len[b], dst + (int64_t)b * dstStride, cap[b], winLen[0] > 0 ? win.data() : nullptr, winLen[0]);
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
                    r = wave_decode_block(&in[(size_t)i * tStride], len[i], out, cap[i], winA, wl);
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
