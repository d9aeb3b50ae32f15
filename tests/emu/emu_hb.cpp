// Lane-emulation harness of the builder that cuts a block's chain and lists into pieces (plz4_amd/csrc/lz4hc_lists_device.inl, the
// kernels k_hb_count .. k_hb_chain of plz4hip.hip): hb_staged.h runs its four stages over the pieces and compares every array with
// hc12_build_lists's and with a loop written from the definition.  Beside it: hb_want of route.h and HbLayout of ws_layout.h for
// tests/test_hb_lists.py.  Test infrastructure only: built into tests/emu/_build/, never loaded by plz4_amd, not a CPU fallback.
#define PLZ4_EMU 1
#include "hb_staged.h"
#include <string>

int plz4_emu_descending = 0;

using namespace plz4;

extern "C" {

void emu_hb_set_descending(int d) { plz4_emu_descending = d; }

// 0: the staged builder (pieces ascending and descending) writes what hc12_build_lists and the definition give
int emu_hb_compare(const uint8_t* src, int n, int piece, int skipLo, int skipHi) { return hbt::compare(src, n, piece, skipLo, skipHi); }

// The definition loop over src, for the search of an input: out[0] positions whose predecessor is exactly 65535 back with a piece
// boundary between them, out[1] exactly 65536 back likewise, out[2] positions whose predecessor lies two or more pieces back.
void emu_hb_probe(const uint8_t* src, int n, int piece, int64_t* out)
{
    out[0] = out[1] = out[2] = 0;
    std::vector<int> last(kHcHashEntries, -1);
    for (int p = 0; p + 4 <= n; ++p) {
        const uint32_t h = hbt::def_hash(src + p);
        const int q = last[h];
        last[h] = p;
        if (q < 0) continue;
        const bool crosses = p / piece != q / piece;
        if (p - q == 65535 && crosses) out[0]++;
        if (p - q == 65536 && crosses) out[1]++;
        if (p / piece - q / piece >= 2) out[2]++;
    }
}

// hb_want under an environment given as "NAME=value\n" lines: out = {on, piece, P, hbMax, hbPieceKiB}
void emu_hb_want(const char* env, int level, int nb, int maxLen, int span, int segmented, int overlap, int64_t* out)
{
    const std::string e = env;
    std::vector<std::pair<std::string, std::string>> vars;
    for (size_t at = 0; at < e.size(); ) {
        const size_t nl = e.find('\n', at), eq = e.find('=', at);
        vars.push_back({e.substr(at, eq - at), e.substr(eq + 1, nl - eq - 1)});
        at = nl + 1;
    }
    const auto get = [&](const char* n) -> const char* { for (auto& v : vars) if (v.first == n) return v.second.c_str(); return nullptr; };
    const HcSwitches sw = parse_hc_switches(get);
    const HbWant w = hb_want(HbShape{level, nb, maxLen, span, segmented != 0, overlap != 0}, sw);
    out[0] = w.on; out[1] = w.piece; out[2] = w.P; out[3] = sw.hbMax; out[4] = sw.hbPieceKiB;
}
int emu_hb_default_max_blocks() { return kHbMaxBlocks; }
int emu_hb_default_piece_kib() { return kHbPieceKiB; }

// HbLayout: out = {offCnt, offSlot, total, pieceStride}; takes (offset, count, element size, alignment) into `takes`, returns how many
int emu_hb_layout(int per, int P, uint64_t* out, uint64_t* takes, int room)
{
    std::vector<WsTake> log;
    const HbLayout L = hb_layout(per, P, &log);
    out[0] = L.offCnt; out[1] = L.offSlot; out[2] = L.total; out[3] = L.pieceStride;
    for (int i = 0; i < (int)log.size() && i < room; ++i) { takes[4 * i] = log[i].off; takes[4 * i + 1] = log[i].count; takes[4 * i + 2] = log[i].size; takes[4 * i + 3] = log[i].align; }
    return (int)log.size();
}

}  // extern "C"
