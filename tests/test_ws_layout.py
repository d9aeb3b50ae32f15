"""The device workspaces' layouts and group sizing (plz4_amd/csrc/ws_layout.h) compiled for the CPU (tests/emu/emu_ws_layout.cpp).
(a) Every offset, stride, perBlock, total and group size equals what the expressions this header replaced computed for the same
shape: tests/golden/ws_layout_parent.json, written once by a program that carried those expressions verbatim (-1: a value the old
code did not compute for that shape).  (b) Each layout is sound by itself: its arrays are pairwise disjoint, aligned for their
element type and inside `total`, and a larger group never needs less.  All numbers are 64-bit on both sides."""
import ctypes as C
import json
import os
import subprocess

import pytest

from orclib import ROOT

SRC = os.path.join(ROOT, "tests", "emu", "emu_ws_layout.cpp")
CSRC = os.path.join(ROOT, "plz4_amd", "csrc")
SO = os.path.join(ROOT, "tests", "emu", "_build", "libemu_ws_layout.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "ws_layout_parent.json")
LAYOUTS = ("l1", "fx", "hc", "hc_pre", "dx", "dxb", "staging")
PLANS = ("l1_group", "hc_group", "hc_pre_plan")
GROUP_SIZED = {"l1": "per", "fx": "per", "hc": "group", "hc_pre": "per", "dx": "wb", "dxb": "nb", "staging": "n"}


class Lib:
    def __init__(self):
        deps = [SRC] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".inl", ".h"))]
        if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(p) for p in deps):
            os.makedirs(os.path.dirname(SO), exist_ok=True)
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-w", "-o", SO, SRC])
        L = self.L = C.CDLL(SO)
        L.wsl_names.restype = C.c_char_p
        L.wsl_values.restype = C.POINTER(C.c_uint64)
        L.wsl_takes.restype = C.POINTER(C.c_uint64)
        L.wsl_run.argtypes = [C.c_char_p, C.POINTER(C.c_int64)]

    def run(self, kind, inputs):
        """({field: value}, [(off, count, size, align)]) of one layout / plan"""
        n = self.L.wsl_run(kind.encode(), (C.c_int64 * len(inputs))(*inputs))
        assert n >= 0, kind
        vals = self.L.wsl_values()
        fields = dict(zip(self.L.wsl_names().decode().split(), (int(vals[i]) for i in range(n))))
        assert len(fields) == n
        t = self.L.wsl_takes()
        return fields, [tuple(int(t[4 * i + j]) for j in range(4)) for i in range(self.L.wsl_n_takes())]


@pytest.fixture(scope="module")
def lib():
    return Lib()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def rows(sec):
    n = len(sec["in"])
    for r in sec["cases"]:
        assert len(r) == n + len(sec["out"])
        yield r[:n], dict(zip(sec["out"], r[n:]))


@pytest.mark.parametrize("kind", LAYOUTS + PLANS)
def test_same_numbers_as_the_expressions_it_replaced(lib, golden, kind):
    sec = golden[kind]
    assert len(sec["cases"]) >= 60
    for inputs, want in rows(sec):
        got, _ = lib.run(kind, inputs)
        assert set(want) <= set(got)
        for name, v in want.items():
            if v >= 0:
                assert got[name] == v, (kind, dict(zip(sec["in"], inputs)), name, got[name], v)


@pytest.mark.parametrize("kind", LAYOUTS)
def test_arrays_disjoint_aligned_and_inside_total(lib, golden, kind):
    sec = golden[kind]
    largest = 0
    for inputs, _ in rows(sec):
        got, takes = lib.run(kind, inputs)
        assert takes
        for off, count, size, align in takes:
            assert off % align == 0, (kind, inputs, off, align)
        spans = sorted((off, off + count * size) for off, count, size, _ in takes if count)
        for (_, end), (nxt, _) in zip(spans, spans[1:]):
            assert end <= nxt, (kind, inputs, end, nxt)
        assert got["total"] >= max(end for _, end in spans), (kind, inputs)
        largest = max(largest, got["total"])
    if kind in ("l1", "hc"):
        assert largest > 1 << 39                                   # 66 049 blocks of 4 MiB: nothing has passed through an int


@pytest.mark.parametrize("kind", LAYOUTS)
def test_total_does_not_decrease_with_the_group(lib, golden, kind):
    sec = golden[kind]
    at = sec["in"].index(GROUP_SIZED[kind])
    shapes = {}
    for inputs, _ in rows(sec):
        shapes.setdefault(tuple(inputs[:at] + inputs[at + 1:]), set()).add(inputs[at])
    assert any(len(v) > 1 for v in shapes.values())
    for rest, sizes in shapes.items():
        if kind == "dx":                                           # (nb, which follows wb in the inputs, stays at one block)
            rest = (1,) + rest[1:]
        sizes = sorted(sizes | set(range(1, 40)))
        totals = [lib.run(kind, list(rest[:at]) + [n] + list(rest[at:]))[0]["total"] for n in sizes]
        assert totals == sorted(totals), (kind, rest)


def test_per_block_is_what_one_block_more_costs_up_to_rounding(lib):
    """perBlock comes out of the same takes as the offsets: two groups' totals differ by it per block, give or take the 256-byte
    rounding of each array (the layouts have at most 15)."""
    for kind, inputs in (("l1", [0, 65536, 1]), ("hc", [0, 65536, 1, 0, 2048]), ("hc_pre", [0, 65536, 1])):
        a, _ = lib.run(kind, [100] + inputs[1:])
        b, _ = lib.run(kind, [101] + inputs[1:])
        assert a["perBlock"] == b["perBlock"] > 0
        assert abs((b["total"] - a["total"]) - a["perBlock"]) <= 15 * 256
