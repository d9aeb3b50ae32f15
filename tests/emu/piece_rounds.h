// The rounds of a few-block parse for ONE block (k_piece per round, k_piece_gather; plz4_amd/csrc/lz4_pieces_device.inl), launch by
// launch as plz4hip.hip enqueues them, on the lane-emulated device code, for any flavour F (FxFlavour<false>, FxFlavour<true>,
// MxFlavour).  Shared by the emulations the tests load (emu_fx.cpp, emu_fxl.cpp, emu_mx.cpp, emu_parse_flow.cpp) and the sanitizer
// program (piece_bounds_main.cpp): every workspace array is a heap allocation of exactly what piece_layout plans for one block of
// P pieces, so a sanitizer sees every access outside one.  Test infrastructure only.
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

template <class F> struct PieceEmuBlock {
    int n, pb, P, recStride;
    PieceLayout L;
    PieceMeta* meta; uint32_t* tabIn; uint32_t* tabOut; uint64_t* rec; FxlBlk* xb;
    long long walked = 0;                                                   // bytes the pieces' runs covered, all rounds
    // maxLen: what the call's workspace is sized for (the block's own length unless the call has longer blocks); hist: with the
    // block's FxlBlk behind the records
    PieceEmuBlock(int n_, int pb_, int maxLen = -1, bool hist = false) : n(n_), pb(pb_)
    {
        if (maxLen < n) maxLen = n;
        P = (maxLen + pb - 1) / pb; if (P < 1) P = 1;                       // PieceCut::P of a call whose largest block this is
        recStride = piece_rec_stride(pb);
        std::vector<WsTake> log;
        L = piece_layout(1, P, recStride, F::kTab, hist, &log);
        const auto exact = [&](size_t i) { const size_t b = i < log.size() ? log[i].count * log[i].size : 0; void* p = malloc(b ? b : 1); if (!p) abort(); return p; };
        meta = (PieceMeta*)exact(0); tabIn = (uint32_t*)exact(1); tabOut = (uint32_t*)exact(2); rec = (uint64_t*)exact(3); xb = (FxlBlk*)exact(4);
        memset(meta, 0xEE, log[0].count * log[0].size);                      // (the device workspace comes uninitialised)
    }
    PieceEmuBlock(const PieceEmuBlock&) = delete;
    ~PieceEmuBlock() { free(meta); free(tabIn); free(tabOut); free(rec); free(xb); }

    // P launches of k_piece (grid x = P), the pieces of a round in ascending (order 0) or descending order; returns the last round
    // in which a piece ran
    int run(const F& f, const uint8_t* src, int warm, int order)
    {
        int rounds = 0;
        const int bs = f.base();
        for (int r = 1; r <= P; ++r) {
            int ran = 0;
            for (int j = 0; j < P; ++j) {
                const int k = order ? P - 1 - j : j;
                if (!piece_round(f, src, n, k, r, pb, warm, meta, tabIn, tabOut, rec, recStride)) continue;
                ++ran;
                const int p0 = bs + k * pb - warm;
                const int from = r > 1 ? meta[k].inAnchor : (k > 0 && f.guessed(p0) ? p0 : bs);
                walked += (meta[k].fin ? bs + n : meta[k].outAnchor[r & 1]) - from;
            }
            if (ran) rounds = r;
            // (the kernels run all P rounds; later ones find nothing to do -- kept here as a check that they really would not)
        }
        return rounds;
    }
    // k_piece_gather (grid x = P); true: exactly one piece was the chain's last
    bool gather(uint64_t* seq, int seqCap, SeqInfo* info, int order, int* chained)
    {
        int last = 0; *chained = 0;
        for (int j = 0; j < P; ++j) {
            const int k = order ? P - 1 - j : j;
            if (k >= piece_count<F::kPiece0>(n, pb)) continue;
            const int g = piece_gather<F::kPiece0>(n, k, pb, meta, rec, recStride, seq, seqCap, info);
            *chained += g > 0; last += g == 2;
        }
        return last == 1;
    }
    long long again() const { long long a = 0; for (int k = 0; k < piece_count<F::kPiece0>(n, pb); ++k) a += meta[k].runs > 1; return a; }
};

}  // namespace plz4
