// The route decisions of plz4_amd/csrc/route.h, compiled for the CPU (tests/test_routes.py).  One entry point: a function's name and
// its inputs in -- the call's shape, what was granted, the switches as the launcher would have read them (kUnset: not set) -- every
// answer out as a 64-bit value with its name; the group list of hc_groups as (start, size) pairs beside them.
#define PLZ4_EMU 1
#include "../../plz4_amd/csrc/lz4_device.inl"
#include "../../plz4_amd/csrc/lz4_seq_device.inl"
#include "../../plz4_amd/csrc/lz4hc_device.inl"
#include "../../plz4_amd/csrc/lz4hc12_device.inl"
#include "../../plz4_amd/csrc/lz4hc_lazy_device.inl"
#include "../../plz4_amd/csrc/lz4hcx_device.inl"
#include "../../plz4_amd/csrc/lz4_dx_device.inl"
#include "../../plz4_amd/csrc/lz4_fx_device.inl"
#include "../../plz4_amd/csrc/lz4_block_io.inl"
#include "../../plz4_amd/csrc/ws_layout.h"
#include "../../plz4_amd/csrc/route.h"
#include <string>
using namespace plz4;

namespace {
std::string names;
std::vector<int64_t> values, list;
void put(const char* name, int64_t v) { names += name; names += ' '; values.push_back(v); }
#define P(x) put(#x, (int64_t)p.x)
}  // namespace

extern "C" {

const char* rt_names(void) { return names.c_str(); }
const int64_t* rt_values(void) { return values.data(); }
int rt_n_list(void) { return (int)list.size(); }
const int64_t* rt_list(void) { return list.data(); }
int64_t rt_unset(void) { return kUnset; }

// The switches out of an environment given as "NAME=value\n" lines, as read_*_switches parse them: every field by name.
int rt_parse(const char* kind, const char* env)
{
    names.clear(); values.clear(); list.clear();
    const std::string k = kind, e = env;
    std::vector<std::pair<std::string, std::string>> vars;
    for (size_t at = 0; at < e.size(); ) {
        const size_t nl = e.find('\n', at), eq = e.find('=', at);
        vars.push_back({e.substr(at, eq - at), e.substr(eq + 1, nl - eq - 1)});
        at = nl + 1;
    }
    const auto get = [&](const char* n) -> const char* { for (auto& v : vars) if (v.first == n) return v.second.c_str(); return nullptr; };
    if (k == "l1") {
        const L1Switches p = parse_l1_switches(get);
        P(fused); P(fxLinked); P(fxMax); P(fxPieceKiB); P(fxWarmKiB); P(l1x); P(oneWorkspace); P(budgetGiB); P(budgetMiB); P(noGate); P(duplexP); P(duplexD); P(duplexPrio);
    } else if (k == "hc") {
        const HcSwitches p = parse_hc_switches(get);
        P(hcx); P(extOff); P(midOff); P(lazyOff); P(preOff); P(listsOff); P(h12Off); P(h12Lazy); P(h12SegOff); P(minSeg); P(segs); P(gather); P(idle);
        P(overlapMin); P(overlapOff); P(overlapGroups); P(budgetGiB); P(h12Group); P(group);
    } else if (k == "dx") {
        const DxSwitches p = parse_dx_switches(get);
        P(dxMax); P(linked); P(groupBlocks); P(big); P(bigMaxMiB); P(bigGroup); P(bigRunKiB);
    } else return -1;
    return (int)values.size();
}

// returns the number of values, -1: no such function
int rt_run(const char* kind, const int64_t* in)
{
    names.clear(); values.clear(); list.clear();
    const std::string k = kind;
    if (k == "l1") {
        // nb maxLen raw mid rider hist l1x body ctx | wsGranted fxGranted | fused fxLinked fxMax fxPieceKiB fxWarmKiB l1x
        const L1Shape s{(int)in[0], (int)in[1], in[2] != 0, in[3] != 0, in[4] != 0, in[5] != 0, in[6] != 0, in[7] != 0, in[8] != 0};
        L1Switches sw;
        sw.fused = in[11] != 0; sw.fxLinked = (int)in[12]; sw.fxMax = (int)in[13]; sw.fxPieceKiB = (int)in[14]; sw.fxWarmKiB = (int)in[15]; sw.l1x = (int)in[16];
        const L1Want p = l1_want(s, sw);
        P(staged); P(fx); P(piece); P(warm); P(P);
        put("route", (int64_t)l1_route(s, sw, p, in[9] != 0, in[10] != 0));
        put("fxl_wanted", fxl_wanted(sw, s.nb, s.maxLen)); put("l1x_on", l1x_on(sw));
    } else if (k == "hc") {
        // level nb maxLen raw hcEx dict dictCtx linked hcxStart | midDeclined | hcx extOff midOff lazyOff preOff h12Off h12Lazy h12SegOff minSeg segs gather idle
        const HcShape s{(int)in[0], (int)in[1], (int)in[2], in[3] != 0, in[4] != 0, in[5] != 0, in[6] != 0, in[7] != 0, in[8] != 0};
        HcSwitches sw;
        sw.hcx = (int)in[10]; sw.extOff = in[11] != 0; sw.midOff = in[12] != 0; sw.lazyOff = in[13] != 0; sw.preOff = in[14] != 0;
        sw.h12Off = in[15] != 0; sw.h12Lazy = in[16] != 0; sw.h12SegOff = in[17] != 0;
        sw.minSeg = (int)in[18]; sw.segs = (int)in[19]; sw.gather = (int)in[20]; sw.idle = (int)in[21];
        const HcPlan p = hc_route(s, sw, in[9] != 0);
        put("route", (int64_t)p.route);
        P(hcx); P(lazy); P(lazyEx); P(seg12); P(segs); P(pre); P(prepExt); P(ctxBlocks); P(hcxBehind); P(lzMinSeg); P(lzSegs); P(gather); P(idle);
    } else if (k == "hc_groups") {
        // nb group lazy | overlapMin overlapOff overlapGroups
        HcSwitches sw;
        sw.overlapMin = (int)in[3]; sw.overlapOff = in[4] != 0; sw.overlapGroups = (int)in[5];
        const HcGroups p = hc_groups((int)in[0], (int)in[1], in[2] != 0, sw);
        P(overlap); P(per); P(nGroups);
        for (size_t i = 0; i < p.gStart.size(); ++i) { list.push_back(p.gStart[i]); list.push_back(p.gSize[i]); }
    } else if (k == "dx") {
        // nb maxIn maxOut records hist window nChains longest hostFirst | groupsOk granted | dxMax linked groupBlocks big bigMaxMiB bigGroup bigRunKiB
        const DxShape s{(int)in[0], in[1], in[2], in[3] != 0, (int)in[4], in[5] != 0, (int)in[6], (int)in[7], in[8] != 0};
        DxSwitches sw;
        sw.dxMax = (int)in[11]; sw.linked = (int)in[12]; sw.groupBlocks = (int)in[13]; sw.big = (int)in[14]; sw.bigMaxMiB = in[15];
        sw.bigGroup = (int)in[16]; sw.bigRunKiB = (int)in[17];
        const DxWant p = dx_want(s, sw);
        P(dx); P(G); P(big); P(bigG); P(thr); P(rounds);
        const DxPlan q = dx_route(s, p, in[9] != 0, in[10] != 0);
        put("route", (int64_t)q.route); put("tail", (int64_t)q.tail);
    } else return -1;
    return (int)values.size();
}

}  // extern "C"
