"""Writes tests/golden/prime_parent.json: how block i of an encode call is primed, as the kernels decided it BEFORE the rule moved to
plz4_amd/csrc/lz4_block_io.inl.  The C++ program below carries those conditions verbatim (k_encode_rec_dict, k_encode_raw_dict,
fxl_dict_of, hc_dict_of without its copy, hc_is_ctx, k_hc_ext_prep's pfx) over stand-in addresses; it was run once, the table is
committed, tests/test_block_io.py holds the shared rule to every row.  Run again only to add inputs: python tests/golden/make_prime_golden.py"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))

# inputs of a row (null: the rule does not read it) and what is recorded.  "bytes": 0 none, 1 prevTail, 2 the dictionary, 3 the
# previous block's tail -- then "off" is where it starts in that block
IN = "raw linked i prevTailLen dictLen prevLen n"
OUT = "l1Mode l1Size l1Bytes l1Off hcMode hcLen hcBytes hcOff isCtx hcPfx"

PROGRAM = r"""
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
enum : int { kDictFreshPrefix = 0, kDictLoad = 1, kDictCtxCopy = 2, kDictCtxLookup = 3, kDictNonePrefix = 4 };
enum : int { kHcNone = 0, kHcExt = 1, kHcCtx = 2 };
enum : int { kHcxMaxBlock = 4096 };
struct DictEnc { const uint8_t* dict; int dictSize; int mode; const uint32_t* dictTable; };
struct HcDict { int mode; int len; const uint8_t* bytes; const uint32_t* hash; const uint16_t* chain; };
struct CodecArgs {
    const uint8_t* src; int64_t srcStride; const int32_t* srcLen; int64_t srcBytes; int bsz;
    const uint8_t* dict; int dictLen; const uint32_t* dictTable; int linked; const uint8_t* prevTail; int prevTailLen;
    const uint32_t* hcDictHash; const uint16_t* hcDictChain; int rawMode;
};
static int block_len(const CodecArgs& a, int i)
{
    if (a.srcLen) return a.srcLen[i];
    const int64_t rem = a.srcBytes - (int64_t)i * a.bsz;
    return (int)(rem < a.bsz ? rem : a.bsz);
}
// k_encode_rec_dict
static DictEnc rec_dict(const CodecArgs& a, int i, int n)
{
        DictEnc dc{nullptr, 0, kDictFreshPrefix, nullptr};
        const uint8_t* tail = nullptr; int tailLen = -1;
        if (a.linked) {
            if (i > 0) { const int pl = block_len(a, i - 1); tailLen = pl < 65536 ? pl : 65536; tail = a.src + (int64_t)(i - 1) * a.srcStride + (pl - tailLen); }
            else if (a.prevTailLen >= 0) { tail = a.prevTail; tailLen = a.prevTailLen; }
        }
        if (tailLen >= 0) {                                   // linked block after another block: LZ4_loadDict(previous tail)
            dc.mode = tailLen >= 8 ? kDictLoad : kDictNonePrefix;
            if (tailLen >= 8) { dc.dict = tail; dc.dictSize = tailLen; }
        } else if (a.dict != nullptr || a.dictLen >= 0) {     // a dictionary context is attached (possibly an empty one)
            if (a.dictLen >= 8) { dc.dict = a.dict; dc.dictSize = a.dictLen; dc.dictTable = a.dictTable; dc.mode = n > 4096 ? kDictCtxCopy : kDictCtxLookup; }
            else dc.mode = kDictNonePrefix;
        }                                                     // else: linked frame start without dictionary -> kDictFreshPrefix
        return dc;
}
// k_encode_raw_dict
static DictEnc raw_dict(const CodecArgs& a, int i, int n)
{
        DictEnc dc{nullptr, 0, kDictNonePrefix, nullptr};
        if (a.dictLen >= 8) { dc.dict = a.dict; dc.dictSize = a.dictLen; dc.dictTable = a.dictTable; dc.mode = n > 4096 ? kDictCtxCopy : kDictCtxLookup; }
        return dc;
}
static DictEnc fxl_dict_of(const CodecArgs& a, int i, int n)
{
    DictEnc dc{nullptr, 0, a.rawMode ? kDictNonePrefix : kDictFreshPrefix, nullptr};
    const uint8_t* tail = nullptr; int tailLen = -1;
    if (!a.rawMode && a.linked) {
        if (i > 0) { const int pl = block_len(a, i - 1); tailLen = pl < 65536 ? pl : 65536; tail = a.src + (int64_t)(i - 1) * a.srcStride + (pl - tailLen); }
        else if (a.prevTailLen >= 0) { tail = a.prevTail; tailLen = a.prevTailLen; }
    }
    if (tailLen >= 0) {                                       // linked block after another block: LZ4_loadDict(previous tail)
        dc.mode = tailLen >= 8 ? kDictLoad : kDictNonePrefix;
        if (tailLen >= 8) { dc.dict = tail; dc.dictSize = tailLen; }
    } else if (a.rawMode || a.dict != nullptr || a.dictLen >= 0) {     // a dictionary context is attached (possibly an empty one)
        if (a.dictLen >= 8) { dc.dict = a.dict; dc.dictSize = a.dictLen; dc.dictTable = a.dictTable; dc.mode = n > 4096 ? kDictCtxCopy : kDictCtxLookup; }
        else dc.mode = kDictNonePrefix;
    }
    return dc;
}
// hc_dict_of; *from: the segment it would lay in front of the block (its copy is left out)
static HcDict hc_dict_of(const CodecArgs& a, int i, int n, const uint8_t* s, bool rawApi, const uint8_t** from)
{
    HcDict d; d.mode = kHcNone; d.len = 0; d.bytes = nullptr; d.hash = nullptr; d.chain = nullptr;
    const uint8_t* seg = nullptr; int segLen = -1;
    if (!rawApi && a.linked) {
        if (i > 0) { const int pl = block_len(a, i - 1); segLen = pl < 65536 ? pl : 65536; seg = a.src + (int64_t)(i - 1) * a.srcStride + (pl - segLen); }
        else if (a.prevTailLen >= 0) { seg = a.prevTail; segLen = a.prevTailLen; }
    }
    if (segLen < 0 && (a.dict != nullptr || a.dictLen >= 0)) {           // a dictionary context is attached (lz4hc.c:1438-1461)
        const int dl = a.dictLen > 0 ? a.dictLen : 0;
        if (n > 4096) { seg = a.dict; segLen = dl; }                      // its state is copied: same as LZ4_loadDictHC + setExternalDict
        else { d.mode = kHcCtx; d.len = dl; d.bytes = a.dict; d.hash = a.hcDictHash; d.chain = a.hcDictChain; }
    }
    if (segLen >= 0) {
        d.mode = kHcExt; d.len = segLen;
        *from = seg;
    }
    return d;
}
static bool hc_is_ctx(const CodecArgs& a, int i, int n, bool rawApi)
{
    if (n > kHcxMaxBlock) return false;
    if (!rawApi && a.linked && (i > 0 || a.prevTailLen >= 0)) return false;
    return a.dict != nullptr || a.dictLen >= 0;
}

static const uint8_t* const SRC = (const uint8_t*)0x10000000, * const DICT = (const uint8_t*)0x20000000, * const TAIL = (const uint8_t*)0x30000000;
static const int64_t STRIDE = 1 << 20;
static void where(const uint8_t* p, int i, int* kind, long long* off)
{
    *off = -1;
    if (!p) *kind = 0;
    else if (p == TAIL) *kind = 1;
    else if (p == DICT) *kind = 2;
    else { *kind = 3; *off = (long long)(p - (SRC + (int64_t)(i - 1) * STRIDE)); }
}
static bool same(const DictEnc& x, const DictEnc& y) { return x.dict == y.dict && x.dictSize == y.dictSize && x.mode == y.mode && x.dictTable == y.dictTable; }

int main()
{
    static const uint32_t table[1] = {0}, hash[1] = {0}; static const uint16_t chain[1] = {0};
    const int ptls[] = {-1, 0, 7, 8, 65536}, dls[] = {-1, 0, 7, 8, 65536}, pls[] = {-1, 0, 7, 8, 65535, 65536, 70000}, ns[] = {0, 1, 4096, 4097};
    bool first = true;
    for (int raw = 0; raw < 2; ++raw) for (int linked = 0; linked < 2; ++linked) for (int i = 0; i < 3; ++i)
    for (int ptl : ptls) for (int dl : dls) for (int n : ns) {
        const bool readsPrev = !raw && linked && i > 0;
        for (int k = 0; k < (readsPrev ? 7 : 1); ++k) {
            int32_t lens[3] = {5, 5, 5};
            if (i > 0) lens[i - 1] = readsPrev ? pls[k] : 5;
            lens[i] = n;
            CodecArgs a{};
            a.src = SRC; a.srcStride = STRIDE; a.srcLen = lens; a.bsz = 1 << 20;
            a.dict = dl >= 0 ? DICT : nullptr; a.dictLen = dl; a.dictTable = table; a.hcDictHash = hash; a.hcDictChain = chain;
            a.linked = linked; a.prevTail = ptl >= 0 ? TAIL : nullptr; a.prevTailLen = ptl; a.rawMode = raw;
            const DictEnc dc = fxl_dict_of(a, i, n);
            if (!same(dc, raw ? raw_dict(a, i, n) : rec_dict(a, i, n))) { fprintf(stderr, "the level-1 copies disagree\n"); return 1; }
            if ((dc.dictTable != nullptr) != (dc.mode == kDictCtxCopy || dc.mode == kDictCtxLookup)) { fprintf(stderr, "table\n"); return 1; }
            const uint8_t* from = nullptr;
            const HcDict d = hc_dict_of(a, i, n, SRC + (int64_t)i * STRIDE, raw != 0, &from);
            if ((d.hash != nullptr) != (d.mode == kHcCtx) || (d.chain != nullptr) != (d.mode == kHcCtx)) { fprintf(stderr, "tables\n"); return 1; }
            const int pfx = d.mode == kHcCtx ? -1 : (d.mode == kHcExt ? d.len : 0);           // k_hc_ext_prep
            int k1, k2; long long o1, o2;
            where(dc.dict, i, &k1, &o1);
            where(d.mode == kHcExt ? from : d.bytes, i, &k2, &o2);
            printf("%s[%d,%d,%d,%d,%d,", first ? "" : ",\n", raw, linked, i, ptl, dl);
            if (readsPrev) printf("%d", pls[k]); else printf("null");
            printf(",%d, %d,%d,%d,%lld, %d,%d,%d,%lld, %d,%d]", n, dc.mode, dc.dictSize, k1, o1, d.mode, d.len, k2, o2, (int)hc_is_ctx(a, i, n, raw != 0), pfx);
            first = false;
        }
    }
    printf("\n");
    return 0;
}
"""


def main():
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "prime_parent.cpp"), os.path.join(tmp, "prime_parent")
        with open(src, "w") as f:
            f.write(PROGRAM)
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-w", "-o", exe, src])
        rows = subprocess.check_output([exe], text=True)
    cases = json.loads("[" + rows + "]")
    with open(os.path.join(HERE, "prime_parent.json"), "w") as f:
        f.write('{"in": "%s",\n "out": "%s",\n "cases": [\n%s]}\n' % (IN, OUT, rows))
    print("%d rows" % len(cases), file=sys.stderr)


if __name__ == "__main__":
    main()
