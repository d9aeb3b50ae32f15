"""The launchers' route decisions (plz4_amd/csrc/route.h) compiled for the CPU (tests/emu/emu_routes.cpp).
(a) Every route, flag and derived parameter equals what the conditions this header replaced gave for the same shape, switches and
grants: tests/golden/routes_parent.json, written once by a program that carried those conditions verbatim (-1: a value the old code
did not compute on that path).  (b) The golden file itself covers every route, every switch that bears on a route and the edges the
code names.  (c) The group list of the segmented HC route tiles the call.  (d) The three callers of the level-1 decision with
history outside the block cannot contradict each other."""
import ctypes as C
import json
import os
import subprocess

import pytest

from orclib import ROOT

SRC = os.path.join(ROOT, "tests", "emu", "emu_routes.cpp")
CSRC = os.path.join(ROOT, "plz4_amd", "csrc")
SO = os.path.join(ROOT, "tests", "emu", "_build", "libemu_routes.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "routes_parent.json")

# the enums of route.h, in their order
L1_ROUTES = ("Fused", "DictKernels", "Parse", "Duplex", "Mid", "Fx", "Fxl", "L1x", "MidDeclined", "NoMemBody")
HC_ROUTES = ("HcxOnly", "MidStaged", "Segmented", "OneThread")
DX_ROUTES = ("OneWave", "Dx", "DxGrouped", "DxBig")
DX_TAILS = ("Raw", "Rec", "RecDx", "RawDict", "RecDict", "RecLinked", "None")
ROUTES = {"l1": L1_ROUTES, "hc": HC_ROUTES, "dx": DX_ROUTES}
# the inputs that are switch fields.  The other fields of the structs (workspace count and budgets, the gate, the duplex shape, the
# group budgets) size or shape a launch and choose no route: the launchers read them, the route functions do not.
SWITCHES = {"l1": ("fused", "fxLinked", "fxMax", "fxPieceKiB", "fxWarmKiB", "l1x_sw"),
            "hc": ("hcx", "extOff", "midOff", "lazyOff", "preOff", "h12Off", "h12Lazy", "h12SegOff", "minSeg", "segs", "gather", "idle"),
            "hc_groups": ("overlapMin", "overlapOff", "overlapGroups"),
            "dx": ("dxMax", "linked", "groupBlocks", "big", "bigMaxMiB", "bigGroup", "bigRunKiB")}
UNSET = -(1 << 31)


class Lib:
    def __init__(self):
        deps = [SRC] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".inl", ".h"))]
        if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(p) for p in deps):
            os.makedirs(os.path.dirname(SO), exist_ok=True)
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-w", "-o", SO, SRC])
        L = self.L = C.CDLL(SO)
        L.rt_names.restype = C.c_char_p
        L.rt_values.restype = C.POINTER(C.c_int64)
        L.rt_list.restype = C.POINTER(C.c_int64)
        L.rt_unset.restype = C.c_int64
        L.rt_run.argtypes = [C.c_char_p, C.POINTER(C.c_int64)]
        L.rt_parse.argtypes = [C.c_char_p, C.c_char_p]
        assert L.rt_unset() == UNSET

    def run(self, kind, inputs):
        """({field: value}, [(start, size)]) of one question"""
        n = self.L.rt_run(kind.encode(), (C.c_int64 * len(inputs))(*inputs))
        assert n >= 0, kind
        vals = self.L.rt_values()
        fields = dict(zip(self.L.rt_names().decode().split(), (int(vals[i]) for i in range(n))))
        assert len(fields) == n
        t = self.L.rt_list()
        return fields, [(int(t[2 * i]), int(t[2 * i + 1])) for i in range(self.L.rt_n_list() // 2)]


@pytest.fixture(scope="module")
def lib():
    return Lib()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    for sec in g.values():
        sec["in"] = sec["in"].split()
        sec["out"] = sec["out"].split()
    return g


def rows(sec):
    n = len(sec["in"])
    for r in sec["cases"]:
        assert len(r) == n + len(sec["out"])
        yield [UNSET if v is None else v for v in r[:n]], dict(zip(sec["out"], r[n:]))     # (null: a switch that is not set)


@pytest.mark.parametrize("kind", ("l1", "hc", "hc_groups", "dx"))
def test_same_answers_as_the_conditions_it_replaced(lib, golden, kind):
    sec = golden[kind]
    for inputs, want in rows(sec):
        got, groups = lib.run(kind, inputs)
        what = dict(zip(sec["in"], inputs))
        for name, v in want.items():
            if name == "groups":
                assert [x for g in groups for x in g] == v, (kind, what)
            elif v >= 0:
                assert got[name] == v, (kind, what, name, got[name], v)


@pytest.mark.parametrize("kind", ("l1", "hc", "dx"))
def test_golden_file_has_every_route_and_enough_cases(golden, kind):
    sec = golden[kind]
    assert len(sec["cases"]) >= 200
    seen = {want["route"] for _, want in rows(sec)}
    assert seen == set(range(len(ROUTES[kind]))), (kind, seen)
    if kind == "dx":
        assert {want["tail"] for _, want in rows(sec)} == set(range(len(DX_TAILS)))


@pytest.mark.parametrize("kind", ("l1", "hc", "hc_groups", "dx"))
def test_every_switch_changes_some_answer(golden, kind):
    sec = golden[kind]
    by_inputs = {tuple(i): w for i, w in rows(sec)}
    for name in SWITCHES[kind]:
        at = sec["in"].index(name)
        groups = {}
        for inputs, want in by_inputs.items():
            groups.setdefault(inputs[:at] + inputs[at + 1:], []).append(want)
        assert any(any(a != b for a in ws for b in ws) for ws in groups.values() if len(ws) > 1), (kind, name)


def test_golden_file_has_the_edges_the_code_names(golden):
    def values(kind, name, where=lambda d: True):
        sec = golden[kind]
        return {i[sec["in"].index(name)] for i, _ in rows(sec) if where(dict(zip(sec["in"], i)))}
    assert {65546, 65547, 1 << 22, (1 << 22) + 1} <= values("l1", "maxLen")
    assert {128, 129} <= values("l1", "nb") and {128, 129} <= values("dx", "nb")
    assert {16383, 16384} <= values("dx", "maxIn")
    assert {(4 << 20) + 8, (4 << 20) + 9} <= values("dx", "maxOut")
    assert {4096, 4097} <= values("hc", "maxLen", lambda d: d["dictCtx"] and d["hcxStart"])
    assert {2047, 2048} <= values("hc_groups", "nb", lambda d: d["lazy"])


def test_groups_tile_the_call(lib):
    for group, switches in ((2048, [2048, 0, 4]), (2048, [2, 0, 4]), (64, [2, 0, 4]), (3, [2, 0, 2]), (1, [2, 0, 4]), (5000, [2, 0, 16]), (700, [2, 1, 4])):
        for nb in range(1, 5001 if group >= 64 else 301):            # (groups of 1 and 3: thousands of them per call say nothing new)
            for lazy in (0, 1):
                got, groups = lib.run("hc_groups", [nb, group, lazy] + switches)
                per = got["per"]
                assert 1 <= per <= group and got["nGroups"] == len(groups)
                at = 0
                for start, size in groups:
                    assert start == at and 1 <= size <= per, (nb, group, switches, groups)
                    at += size
                assert at == nb
                sizes = [s for _, s in groups]
                if got["overlap"]:
                    assert lazy and nb >= switches[0] and not switches[1] and 2 * per <= group   # two groups' worth of workspace
                    assert sizes[0] == min(max(per // 8, 1), nb)
                    for a, b in zip(sizes, sizes[1:-1]):
                        assert b == min(2 * a, per)
                    if len(sizes) > 1:
                        assert sizes[-1] <= min(2 * sizes[-2], per)
                else:
                    assert all(s == per for s in sizes[:-1])


def test_the_three_callers_of_the_level_1_decision_agree(lib, golden):
    """History outside the block: the host-buffer calls (their slot's workspace has no room for the bulk staged route), the device
    entry point that stages its records, and the one that writes them into a frame body and allocates a staging area when, and only
    when, launch_l1 will run the one-kernel encoder."""
    sec = golden["l1"]
    ix = {n: sec["in"].index(n) for n in sec["in"]}
    seen = set()
    for inputs, _ in rows(sec):
        if not inputs[ix["hist"]]:
            continue
        key = (inputs[ix["nb"]], inputs[ix["maxLen"]]) + tuple(inputs[ix["fused"]:])
        if key in seen or inputs[ix["maxLen"]] > 1 << 22 or inputs[ix["maxLen"]] <= 0:     # (the body entry point refuses larger blocks)
            continue
        seen.add(key)

        def ask(l1x, body, ws, fx):
            i = list(inputs)
            i[ix["raw"]] = i[ix["mid"]] = i[ix["rider"]] = 0
            i[ix["hist"]], i[ix["l1x"]], i[ix["body"]], i[ix["wsGranted"]], i[ix["fxGranted"]] = 1, l1x, body, ws, fx
            got, _ = lib.run("l1", i)
            return got["staged"], L1_ROUTES[got["route"]]
        for ws, fx in ((1, 1), (1, 0), (0, 0)):
            staged, route = ask(0, 0, ws, fx)                       # host_codec
            assert route in (("Fxl", "DictKernels") if staged else ("DictKernels",)), (key, route)
            staged_dev, route = ask(1, 0, ws, fx)                   # plz4hip_dev_encode_records_ex
            assert route in (("Fxl", "L1x", "DictKernels") if staged_dev else ("DictKernels",)), (key, route)
            staged_body, _ = ask(1, 1, ws, fx)                      # plz4hip_dev_encode_body_ex: what it asks ...
            assert staged_body == staged_dev
            if staged_body:                                         # ... no staging area: launch_l1 writes into the body or refuses
                assert ask(1, 1, ws, fx)[1] in ("Fxl", "L1x", "NoMemBody"), key
            else:                                                   # ... a staging area: launch_l1 gets a stage and runs the one-kernel encoder
                assert ask(1, 0, ws, fx)[1] == "DictKernels", key
    assert len(seen) >= 90                                         # 3 block counts x 3 lengths x the switch settings of the sweep


def test_switches_are_parsed_and_clamped_as_before(lib):
    """parse_*_switches on a table instead of the environment: the defaults, "unset" where it differs from a value, and every clamp
    the launchers had (PLZ4HIP_FX_PIECE_KIB in 1..4096, _WARMUP_KIB in 0..4096, PLZ4HIP_HC_MIN_SEG >= 64, PLZ4HIP_HC_SEGS in 1..512,
    PLZ4HIP_HC_OVERLAP_GROUPS >= 2, PLZ4HIP_DX_BIG_GROUP in 2..256, _RUN_KIB in 1..2^20, PLZ4HIP_DUPLEX falling back to 1,1)."""
    def parse(kind, **env):
        n = lib.L.rt_parse(kind.encode(), "".join("PLZ4HIP_%s=%s\n" % kv for kv in env.items()).encode())
        vals = lib.L.rt_values()
        return dict(zip(lib.L.rt_names().decode().split(), (int(vals[i]) for i in range(n))))
    assert parse("l1") == dict(fused=0, fxLinked=UNSET, fxMax=128, fxPieceKiB=64, fxWarmKiB=64, l1x=UNSET, oneWorkspace=0, budgetGiB=0, budgetMiB=0,
                               noGate=0, duplexP=1, duplexD=1, duplexPrio=3)
    assert parse("hc") == dict(hcx=UNSET, extOff=0, midOff=0, lazyOff=0, preOff=0, listsOff=0, h12Off=0, h12Lazy=0, h12SegOff=0, minSeg=8192, segs=512,
                               gather=12, idle=16, overlapMin=2048, overlapOff=0, overlapGroups=4, budgetGiB=0, h12Group=0, group=0)
    assert parse("dx") == dict(dxMax=128, linked=UNSET, groupBlocks=UNSET, big=UNSET, bigMaxMiB=1024, bigGroup=0, bigRunKiB=0)
    for v, want in ((0, 64), (1, 1), (4096, 4096), (4097, 64)):
        assert parse("l1", FX_PIECE_KIB=v)["fxPieceKiB"] == want
    for v, want in ((-1, 64), (0, 0), (4096, 4096), (4097, 64)):
        assert parse("l1", FX_WARMUP_KIB=v)["fxWarmKiB"] == want
    assert parse("l1", L1_FUSED=0)["fused"] == 1 and parse("l1", EXP_NO_GATE="")["noGate"] == 1     # (set, whatever the value)
    assert [parse("l1", L1_WORKSPACES=v)["oneWorkspace"] for v in (1, 2)] == [1, 0]
    got = parse("l1", FX_LINKED=0, FX_MAX_BLOCKS=0, L1X=0, L1_BUDGET_GIB=3, L1_BUDGET_MIB=5, DUPLEX_PRIO=0, DUPLEX="9,7")
    assert [got[k] for k in ("fxLinked", "fxMax", "l1x", "budgetGiB", "budgetMiB", "duplexPrio", "duplexP", "duplexD")] == [0, 0, 0, 3, 5, 0, 9, 7]
    for text in ("9", "x,7", ""):
        got = parse("l1", DUPLEX=text)
        assert (got["duplexP"], got["duplexD"]) == (1, 1), text
    assert [parse("hc", HC_MIN_SEG=v)["minSeg"] for v in (63, 64, 100000)] == [8192, 64, 100000]
    assert [parse("hc", HC_SEGS=v)["segs"] for v in (-5, 0, 1, 512, 513)] == [1, 1, 1, 512, 512]
    assert [parse("hc", HC_OVERLAP_GROUPS=v)["overlapGroups"] for v in (0, 1, 2, 9)] == [2, 2, 2, 9]
    got = parse("hc", HCX=0, HC_EXT_OFF=1, HC12_LAZY=1, HC_LISTS_OFF=1, HC12_GATHER=8, HC12_IDLE=4, HC_OVERLAP_MIN=2, HC_BUDGET_GIB=7, HC12_GROUP=5, HC_GROUP=6)
    assert [got[k] for k in ("hcx", "extOff", "h12Lazy", "listsOff", "gather", "idle", "overlapMin", "budgetGiB", "h12Group", "group", "midOff")] == \
        [0, 1, 1, 1, 8, 4, 2, 7, 5, 6, 0]
    assert [parse("dx", DX_BIG_GROUP=v)["bigGroup"] for v in (1, 2, 256, 257)] == [0, 2, 256, 0]
    assert [parse("dx", DX_BIG_RUN_KIB=v)["bigRunKiB"] for v in (0, 1, 1 << 20, (1 << 20) + 1)] == [0, 1, 1 << 20, 0]
    got = parse("dx", DX_MAX_BLOCKS=0, DX_LINKED=0, DXL_GROUP_BLOCKS=0, DX_BIG=0, DX_BIG_MAX_MIB=4096)
    assert [got[k] for k in ("dxMax", "linked", "groupBlocks", "big", "bigMaxMiB")] == [0, 0, 0, 0, 4096]    # (dx_want caps the last at 1024)
