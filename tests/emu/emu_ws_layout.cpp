// The workspace layouts and group sizing of plz4_amd/csrc/ws_layout.h, compiled for the CPU (tests/test_ws_layout.py).  One entry
// point: a layout's name and its inputs in, every field out as a 64-bit value with its name, and the takes the carver made
// (offset, count, element size, element alignment) for the checks that need no reference.  The group-sizing entries run fit_groups
// against an allocator that refuses its first `refuse` requests (-1: all of them) and report what was asked of it.
#define PLZ4_EMU 1
#include "../../plz4_amd/csrc/lz4_device.inl"
#include "../../plz4_amd/csrc/lz4_seq_device.inl"
#include "../../plz4_amd/csrc/lz4hc_device.inl"
#include "../../plz4_amd/csrc/lz4hc12_device.inl"
#include "../../plz4_amd/csrc/lz4hc_lazy_device.inl"
#include "../../plz4_amd/csrc/lz4_dx_device.inl"
#include "../../plz4_amd/csrc/lz4_fx_device.inl"
#include "../../plz4_amd/csrc/ws_layout.h"
#include <string.h>
#include <string>
using namespace plz4;

namespace {
std::string names;
std::vector<uint64_t> values;
std::vector<WsTake> takes;
void put(const char* name, uint64_t v) { names += name; names += ' '; values.push_back(v); }
#define F(x) put(#x, (uint64_t)L.x)

// the allocator of the group-sizing cases
struct Refuser {
    int64_t refuse; uint64_t requests = 0, last = 0, sum = 0;
    bool ask(size_t need) { ++requests; last = need; sum += need; return refuse < 0 || (int64_t)requests <= refuse; }
    void report() const { put("requests", requests); put("last", last); put("sum", sum); }
};
}  // namespace

extern "C" {

const char* wsl_names(void) { return names.c_str(); }
const uint64_t* wsl_values(void) { return values.data(); }
int wsl_n_takes(void) { return (int)takes.size(); }
const uint64_t* wsl_takes(void) { static_assert(sizeof(WsTake) == 4 * sizeof(uint64_t), "four 64-bit words"); return (const uint64_t*)takes.data(); }

// returns the number of values, -1: no such layout
int wsl_run(const char* kind, const int64_t* in)
{
    names.clear(); values.clear(); takes.clear();
    const std::string k = kind;
    if (k == "l1") {
        const L1Layout L = l1_layout((int)in[0], (int)in[1], in[2] != 0, &takes);
        F(seqStride); F(maxChunks); F(perBlock); F(offInfo); F(offChunkBytes); F(offChunkOff); F(offSeq); F(offBk); F(offBlk); F(total);
    } else if (k == "fx") {
        const PieceLayout L = piece_layout((int)in[0], (int)in[1], (int)in[2], kFxTab, in[3] != 0, &takes);
        F(offMeta); F(offIn); F(offOut); F(offRec); F(offBlk); F(total);
    } else if (k == "hc") {
        const HcLayout L = hc_layout((int)in[0], (int)in[1], in[2] != 0, in[3] != 0, (int)in[4], &takes);
        F(chainStride); F(fStride); F(recStride); F(maxChunks); F(perBlock); F(offErr); F(offChain); F(offRank); F(offList); F(offOffsets); F(offF); F(offWs);
        F(offInfo); F(offChunkB); F(offChunkO); F(offRec); F(offBridge); F(offMeta); F(offStarts); F(offPieces); F(total);
    } else if (k == "hc_pre") {
        const HcPreLayout L = hc_pre_layout((int)in[0], (int)in[1], in[2] != 0, &takes);
        F(stride); F(perBlock); F(slack); F(offChain); F(offRank); F(offList); F(offOffsets); F(total);
    } else if (k == "dx") {
        const DxLayout L = dx_layout((int)in[0], (int)in[1], in[2], in[3], in[4] != 0, in[5] != 0, (int)in[6], &takes);
        F(tStride); F(pStride); F(maxSeg); F(offT); F(offPtr); F(offUnits); F(offInfo); F(offSrcOff); F(offLen); F(offHashBad); F(offFirst); F(offChain); F(offGood);
        F(offMoved); F(offDead); F(total);
    } else if (k == "dxb") {
        const DxbLayout L = dxb_layout((int)in[0], in[1], in[2], (int)in[3], (int)in[4], &takes);
        F(tStride); F(pStride); F(tgStride); F(maxSeg); F(groups); F(room); F(offT); F(offPtr); F(offUnits); F(offInfo); F(offTG); F(offEnt); F(offRuns); F(offBi); F(total);
    } else if (k == "staging") {
        const Staging L = staging_layout((int)in[0], (int)in[1], (int)in[2], (size_t)in[3], in[4] != 0, (int)in[5], &takes);
        F(offA); F(offB); F(offRes); F(offSt); F(offLen); F(offOff); F(offIn); F(offOut); F(offPack); F(offExtra); F(offWin); F(offWinLen); F(offFirst); F(winBytes);
        F(total); F(inStride); F(outStride); F(gap);
    } else if (k == "hc_pre_plan") {
        const HcPrePlan L = hc_pre_plan((size_t)in[0], (size_t)in[1], (long)in[2], (int)in[3], in[4] != 0, (int)in[5], (int)in[6], (int)in[7]);
        F(perLists); F(perChain); F(lists);
    } else if (k == "l1_group") {
        // freeB held gib mib nb maxLen l1x refuse -- as launch_l1 sizes its groups; no workspace at all: the fused kernels
        const int nb = (int)in[4], maxLen = (int)in[5]; const bool l1x = in[6] != 0;
        Refuser r{in[7]};
        int per = nb, rc = 0;
        const int64_t grp = l1_first_group((size_t)in[0], (size_t)in[1], (long)in[2], (long)in[3], l1_layout(1, maxLen, l1x).perBlock, nb);
        const int got = fit_groups(nb, grp, false, [&](int p, bool* refused) { per = p; *refused = r.ask(l1_layout(p, maxLen, l1x).total); return 0; }, &rc);
        put("fused", got < 1); put("per", (uint64_t)per); r.report();
    } else if (k == "hc_group") {
        // freeB held gib group nb maxLen lazy needF parseWaves refuse -- as plan_h12 does; not one block: PLZ4HIP_E_NOMEM
        const int nb = (int)in[4], maxLen = (int)in[5], waves = (int)in[8]; const bool lazy = in[6] != 0, needF = in[7] != 0;
        Refuser r{in[9]};
        HcLayout L{}; int rc = 0;
        const int64_t grp = hc_first_group((size_t)in[0], (size_t)in[1], (long)in[2], (int)in[3], hc_layout(1, maxLen, lazy, needF, waves).perBlock, nb);
        const int got = fit_groups(nb, grp, true, [&](int p, bool* refused) { L = hc_layout(p, maxLen, lazy, needF, waves); *refused = r.ask(L.total); return 0; }, &rc);
        put("nomem", got < 1); put("per", (uint64_t)L.group); F(total); r.report();
    } else return -1;
    return (int)values.size();
}

}  // extern "C"
