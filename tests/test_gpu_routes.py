"""What ran on the GPU is what the route function said (plz4_amd/csrc/route.h).  Each case of tests/route_cases.py is one call in a
child process with the call's switches in its environment.  The bytes must equal the oracle's / the real liblz4's, and the deltas of
plz4hip_ctx_counters must be those of the route that the CPU build of the route function (tests/emu/emu_routes.cpp) names for the
call's shape and the same switches, every reservation granted: [0]/[7] count Fx/Fxl, [8] L1x, [9] k_hcx, [3]/[4] Dx with and
without history, [6] the groups, [10] DxBig; every one of them is zero where the route is none of those."""
import json
import os
import subprocess
import sys

import pytest

import route_cases
from orclib import ROOT
from test_routes import DX_ROUTES, HC_ROUTES, L1_ROUTES, UNSET, Lib

pytestmark = pytest.mark.gpu
COUNTED = ("fx_blocks", "fxl_blocks", "l1x_blocks", "hcx_blocks", "dx_blocks", "dxl_blocks", "dxl_groups_last", "dx_big_blocks")
CHILD_TIMEOUT = 120


@pytest.fixture(scope="module")
def lib():
    return Lib()


def _switch(env, name, unset, lo=None, hi=None):
    """A switch as read_*_switches hands it on: the value, or `unset` where it is absent or outside [lo, hi]."""
    if name not in env:
        return unset
    v = int(env[name])
    return v if (lo is None or v >= lo) and (hi is None or v <= hi) else unset


def expected(lib, kind, shape, env):
    """(route name, the counters it implies) for the call's shape and switches, everything granted"""
    zero = dict.fromkeys(COUNTED, 0)
    nb = shape["nb"]
    if kind == "l1":
        ask = lambda sh: lib.run("l1", [sh[k] for k in ("nb", "maxLen", "raw", "mid", "rider", "hist", "l1x", "body", "ctx")] + [1, 1] + [
            int("PLZ4HIP_L1_FUSED" in env), _switch(env, "PLZ4HIP_FX_LINKED", UNSET), _switch(env, "PLZ4HIP_FX_MAX_BLOCKS", 128),
            _switch(env, "PLZ4HIP_FX_PIECE_KIB", 64, 1, 4096), _switch(env, "PLZ4HIP_FX_WARMUP_KIB", 64, 0, 4096), _switch(env, "PLZ4HIP_L1X", UNSET)])[0]
        got = ask(shape)
        if shape["body"] and not got["staged"]:
            # plz4hip_dev_encode_body_ex: "not staged" -> a staging area of the ctx's, and launch_l1 is handed that instead of the body
            got = ask(dict(shape, body=0))
        route = L1_ROUTES[got["route"]]
        moved = {"Fx": {"fx_blocks": nb}, "Fxl": {"fx_blocks": nb, "fxl_blocks": nb}, "L1x": {"l1x_blocks": nb}}.get(route, {})
    elif kind == "hc":
        on = lambda name: int(name in env)
        got, _ = lib.run("hc", [shape[k] for k in ("level", "nb", "maxLen", "raw", "hcEx", "dict", "dictCtx", "linked", "hcxStart")] + [0] + [
            _switch(env, "PLZ4HIP_HCX", UNSET), on("PLZ4HIP_HC_EXT_OFF"), on("PLZ4HIP_HC_MID_OFF"), on("PLZ4HIP_HC_LAZY_OFF"), on("PLZ4HIP_HC_PRE_OFF"),
            on("PLZ4HIP_HC12_OFF"), on("PLZ4HIP_HC12_LAZY"), on("PLZ4HIP_HC12_SEG_OFF"), _switch(env, "PLZ4HIP_HC_MIN_SEG", 8192, 64),
            min(max(_switch(env, "PLZ4HIP_HC_SEGS", 512), 1), 512), _switch(env, "PLZ4HIP_HC12_GATHER", 12), _switch(env, "PLZ4HIP_HC12_IDLE", 16)])
        route = HC_ROUTES[got["route"]]
        # (every block of these calls under a dictionary is one of at most 4 KiB: k_hcx's wherever the route launches it)
        moved = {"hcx_blocks": nb} if got["hcx"] and (route == "HcxOnly" or got["ctxBlocks"] or got["hcxBehind"]) else {}
        route += "".join("+" + f for f in ("lazy", "seg12", "pre") if got[f])
    else:
        got, _ = lib.run("dx", [shape[k] for k in ("nb", "maxIn", "maxOut", "records", "hist", "window", "nChains", "longest", "hostFirst")] + [1, 1] + [
            _switch(env, "PLZ4HIP_DX_MAX_BLOCKS", 128), _switch(env, "PLZ4HIP_DX_LINKED", UNSET), _switch(env, "PLZ4HIP_DXL_GROUP_BLOCKS", UNSET),
            _switch(env, "PLZ4HIP_DX_BIG", UNSET), _switch(env, "PLZ4HIP_DX_BIG_MAX_MIB", 1024), _switch(env, "PLZ4HIP_DX_BIG_GROUP", 0, 2, 256),
            _switch(env, "PLZ4HIP_DX_BIG_RUN_KIB", 0, 1, 1 << 20)])
        route = DX_ROUTES[got["route"]]
        # (a raw block with a capacity above kDxMaxOut is not Dx's to answer: the tail kernel's)
        moved = {"OneWave": {}, "Dx": {"dxl_blocks" if shape["hist"] else "dx_blocks": nb if shape["maxOut"] <= (4 << 20) + 8 else 0},
                 "DxGrouped": {"dxl_blocks": nb, "dxl_groups_last": -(-nb // max(got["G"], 1))},
                 "DxBig": {"dx_blocks": nb, "dx_big_blocks": 1}}[route]
    return route, dict(zero, **moved)


# the routes the issue names for these cases, so that a case that drifts to another route is seen even if its counters agree
NAMED = {"l1_plain": "Fx", "l1_plain-PLZ4HIP_FX_MAX_BLOCKS=0": "Parse", "l1_plain-PLZ4HIP_L1_FUSED=1": "Fused",
         "l1_linked_host": "Fxl", "l1_linked_host-PLZ4HIP_FX_LINKED=0": "DictKernels", "l1_linked_host-PLZ4HIP_L1_FUSED=1": "DictKernels",
         "l1_linked_host-PLZ4HIP_FX_LINKED=0-PLZ4HIP_L1X=0": "DictKernels",
         "l1_linked_body": "Fxl", "l1_linked_body-PLZ4HIP_FX_LINKED=0": "L1x", "l1_linked_body-PLZ4HIP_L1_FUSED=1": "DictKernels",
         "l1_linked_body-PLZ4HIP_FX_LINKED=0-PLZ4HIP_L1X=0": "DictKernels",
         "hc_dict_small-2": "HcxOnly", "hc_dict_small-9": "HcxOnly", "hc_plain-2": "MidStaged", "hc_plain-9": "Segmented+lazy",
         "hc_plain-12": "Segmented+seg12", "hc_plain-12-SEG_OFF": "Segmented", "hc_plain-9-overlap": "Segmented+lazy",
         "hc_plain-9-LAZY_OFF": "OneThread+pre", "dx_raw": "Dx", "dx_raw-MAX=0": "OneWave", "dx_linked_chain": "DxGrouped",
         "dx_big": "DxBig", "dx_big-BIG=0": "Dx"}

_stop = []                                                          # a child ended by a signal or its time limit: nothing more runs


@pytest.mark.parametrize("name", list(route_cases.CASES))
def test_gpu_route_is_what_the_function_said(lib, name):
    if _stop:
        pytest.fail("not run: %s ended by a signal or its time limit" % _stop[0])
    _, _, switches, (kind, shape) = route_cases.CASES[name]
    env = {k: v for k, v in os.environ.items() if not k.startswith("PLZ4HIP_")}
    env.update(switches)
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "route_cases.py"), name], env=env, capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _stop.append(name)
        raise
    if p.returncode < 0:
        _stop.append(name)
    assert p.returncode == 0, (name, p.returncode, p.stderr[-2000:])
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["parity"], name
    route, want = expected(lib, kind, dict(shape, **out["shape"]), switches)
    print(name, route, {k: v for k, v in out["counters"].items() if v})
    assert {k: out["counters"][k] for k in COUNTED} == want, (name, route, out["counters"])
    if name in NAMED:
        assert route == NAMED[name], (name, route)
