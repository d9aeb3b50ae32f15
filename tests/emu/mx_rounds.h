// The rounds of the few-block level-2 path for ONE block (k_mx_piece per round, k_mx_gather; plz4_amd/csrc/lz4_mx_device.inl), launch
// by launch as plz4hip.hip enqueues them, on the lane-emulated device code.  Shared by the emulation the tests load (emu_mx.cpp) and
// the sanitizer program (mx_bounds_main.cpp): every workspace array is a heap allocation of exactly what mx_layout plans for one
// block of P pieces, so a sanitizer sees every access outside one.  Test infrastructure only.
#pragma once
#include "../../plz4_amd/csrc/lz4_device.inl"
#include "../../plz4_amd/csrc/lz4_seq_device.inl"
#include "../../plz4_amd/csrc/lz4hc_device.inl"
#include "../../plz4_amd/csrc/lz4hc12_device.inl"
#include "../../plz4_amd/csrc/lz4hc_lazy_device.inl"
#include "../../plz4_amd/csrc/lz4hcx_device.inl"
#include "../../plz4_amd/csrc/lz4_dx_device.inl"
#include "../../plz4_amd/csrc/lz4_fx_device.inl"
#include "../../plz4_amd/csrc/lz4_mx_device.inl"
#include "../../plz4_amd/csrc/ws_layout.h"
#include <stdlib.h>
#include <string.h>
#include <vector>

namespace plz4 {

struct MxEmuBlock {
    int n, pb, P, recStride;
    MxLayout L;
    FxPiece* meta; uint32_t* tabIn; uint32_t* tabOut; uint64_t* rec;
    long long walked = 0;                                                   // bytes the pieces' walks covered, all rounds
    // maxLen: what the call's workspace is sized for (the block's own length unless the call has longer blocks)
    MxEmuBlock(int n_, int pb_, int maxLen = -1) : n(n_), pb(pb_)
    {
        if (maxLen < n) maxLen = n;
        P = (maxLen + pb - 1) / pb; if (P < 1) P = 1;                       // MxWant::P of a call whose largest block this is
        recStride = mx_rec_stride_host(pb);
        std::vector<WsTake> log;
        L = mx_layout(1, P, recStride, &log);
        const auto exact = [&](int i) { void* p = malloc(log[i].count * log[i].size ? log[i].count * log[i].size : 1); if (!p) abort(); return p; };
        meta = (FxPiece*)exact(0); tabIn = (uint32_t*)exact(1); tabOut = (uint32_t*)exact(2); rec = (uint64_t*)exact(3);
        memset(meta, 0xEE, log[0].count * log[0].size);                      // (the device workspace comes uninitialised)
    }
    MxEmuBlock(const MxEmuBlock&) = delete;
    ~MxEmuBlock() { free(meta); free(tabIn); free(tabOut); free(rec); }

    // P launches of k_mx_piece (grid x = P), the pieces of a round in ascending (order 0) or descending order; returns the last round
    // in which a piece walked
    int run(const uint8_t* src, int warm, int order)
    {
        int rounds = 0;
        for (int r = 1; r <= P; ++r) {
            int ran = 0;
            for (int j = 0; j < P; ++j) {
                const int k = order ? P - 1 - j : j;
                if (!mx_piece(src, n, k, r, pb, warm, meta, tabIn, tabOut, rec, recStride)) continue;
                ++ran;
                const int from = r > 1 ? meta[k].inAnchor : (k > 0 && k * pb - warm > 0 ? k * pb - warm : 0);
                walked += (meta[k].fin ? n : meta[k].outAnchor[r & 1]) - from;
            }
            if (ran) rounds = r;
        }
        return rounds;
    }
    // k_mx_gather (grid x = P); true: exactly one piece was the chain's last
    bool gather(uint64_t* seq, int seqCap, SeqInfo* info, int order, int* chained)
    {
        int last = 0; *chained = 0;
        for (int j = 0; j < P; ++j) {
            const int k = order ? P - 1 - j : j;
            if (k >= mx_pieces(n, pb)) continue;
            const int g = mx_gather(n, k, pb, meta, rec, recStride, seq, seqCap, info);
            *chained += g > 0; last += g == 2;
        }
        return last == 1;
    }
};

}  // namespace plz4
