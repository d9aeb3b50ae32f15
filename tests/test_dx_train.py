"""The stage train of the three few-block decoders (dx, dxb, dxl: the dx_stage_* bodies of plz4_amd/csrc/lz4_dx_device.inl) on the
lane-emulated build, through the one driver the other decode emulations use (tests/emu/dx_train.h): the misfit rule on both sides of
each of its terms, a unit that flags its block while the block's other units still run, and the rounds rule beside the three rules
it replaced.  Every answer is checked against the oracle.  The same cases run under the sanitizers in tests/emu/decode_bounds_main.cpp."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lz4blocks
from orclib import ROOT, _ptr, u8p

SRC = os.path.join(ROOT, "tests", "emu", "emu_dx_train.cpp")
SO = os.path.join(ROOT, "tests", "emu", "_build", "libemu_dx_train.so")
DEPS = [SRC, os.path.join(ROOT, "tests", "emu", "dx_train.h")] + \
       [os.path.join(ROOT, "plz4_amd", "csrc", f) for f in ("lz4_dx_device.inl", "lz4_device.inl", "wave.h", "ws_layout.h")]
i32p = C.POINTER(C.c_int32)
LEFT = -999999
SEG = 8192                                                   # kDxSeg
DX_MAX_OUT = (4 << 20) + 8                                   # kDxMaxOut
MAX_ROUNDS, HIST = 32, 65536                                 # kDxlMaxRounds, kDxlHist
FLAVOURS = {"dx": 0, "dxb": 1, "dxl": 2}


class Train:
    def __init__(self):
        newest = max(os.path.getmtime(p) for p in DEPS)
        if not os.path.exists(SO) or os.path.getmtime(SO) < newest:
            os.makedirs(os.path.dirname(SO), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-parameter", "-o", SO, SRC])
        L = self.L = C.CDLL(SO)
        L.emu_dxt_call.restype = C.c_int
        L.emu_dxt_call.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_void_p), i32p, i32p, C.c_int64, C.c_int64, u8p, C.c_int, u8p, C.c_int64, i32p]
        L.emu_dx_rounds_for.restype = C.c_int; L.emu_dx_rounds_for.argtypes = [C.c_int64]
        L.emu_dxb_rounds.restype = C.c_int; L.emu_dxb_rounds.argtypes = [C.c_int64]
        L.emu_dx_rounds.restype = C.c_int; L.emu_dx_rounds.argtypes = [C.c_int, C.c_int, C.c_int64]
        L.emu_dxt_strides.restype = None; L.emu_dxt_strides.argtypes = [C.c_int, C.c_int64, C.c_int64, C.POINTER(C.c_int64)]

    def strides(self, flavour, max_in, max_out):
        out = (C.c_int64 * 3)()
        self.L.emu_dxt_strides(flavour, max_in, max_out, out)
        return int(out[0]), int(out[1]), int(out[2])

    def call(self, flavour, comps, caps, max_in, max_out, dct=None):
        """A call of raw blocks whose workspace is laid out for max_in / max_out.  Returns [(answer, bytes)]."""
        nb = len(comps)
        keep = [np.ascontiguousarray(c) for c in comps]
        ptrs = (C.c_void_p * nb)(*[a.ctypes.data for a in keep])
        ln = np.array([a.size for a in keep], dtype=np.int32); cap = np.array(caps, dtype=np.int32)
        stride = int(cap.max())
        dst = np.zeros(nb * stride, dtype=np.uint8); ans = np.zeros(nb, np.int32)
        nul = C.cast(None, u8p)
        rc = self.L.emu_dxt_call(flavour, nb, ptrs, ln.ctypes.data_as(i32p), cap.ctypes.data_as(i32p), max_in, max_out,
                                 _ptr(dct) if dct is not None else nul, 0 if dct is None else dct.size, _ptr(dst), stride, ans.ctypes.data_as(i32p))
        assert rc == 0, rc                                                  # (-888888: the units of a block disagree about where they meet)
        return [(int(ans[b]), dst[b * stride:b * stride + max(int(ans[b]), 0)].copy()) for b in range(nb)]


@pytest.fixture(scope="module")
def train():
    return Train()


def _block(rng, min_comp, mod=None):
    """A generator-built valid block of at least min_comp compressed bytes (and mod modulo 64)."""
    nseq = min_comp // 150 + 1
    while True:
        comp, plain = lz4blocks.make_block(rng, nseq)
        if comp.size >= min_comp and (mod is None or comp.size % 64 == mod):
            return comp, plain
        nseq += 1


@pytest.fixture(scope="module")
def blocks():
    rng = np.random.default_rng(20261020)
    dct = rng.integers(0, 256, 5000, dtype=np.uint8)
    return {"dict": dct, "sib": _block(rng, 200), "x0": _block(rng, 1500, 0), "x1": _block(rng, 1500, 1), "x3": _block(rng, 2 * SEG + 64)}


def _oracle(orc, flavour, comp, cap, dct):
    return orc.decompress_safe_dict(comp, cap, dct) if flavour == 2 else orc.decompress_safe(comp, cap)


def _pair(orc, train, flavour, blocks, x, cap_x, max_in, max_out, misfit):
    """The block under test beside the sibling that fits, in a call laid out for max_in / max_out."""
    dct = blocks["dict"] if flavour == 2 else None
    (xc, xp), (sc, sp) = x, blocks["sib"]
    (ax, ox), (as_, os_) = train.call(flavour, [xc, sc], [cap_x, sp.size], max_in, max_out, dct)
    want, wbytes = _oracle(orc, flavour, sc, sp.size, dct)
    assert as_ == want == sp.size and np.array_equal(os_, wbytes), ("the sibling", as_, want)
    if misfit:
        assert ax == LEFT, ("a misfit block is answered", ax)
    else:
        want, wbytes = _oracle(orc, flavour, xc, cap_x, dct)
        assert ax == want == xp.size and np.array_equal(ox, wbytes), ("the fitting block", ax, want)


@pytest.mark.parametrize("name", list(FLAVOURS))
def test_misfit_rule_on_both_sides_of_each_term(orc, train, blocks, name):
    """dx_misfit: n > tStride - 64, cap > pStride - 64, dx_segments(n) > maxSeg -- each term on its last fitting and its first
    misfitting value, in a two-block call whose workspace the sibling's side of the call sizes.  A misfit block is left, the
    sibling decodes to the oracle's bytes."""
    fl = FLAVOURS[name]
    x0, x1, x3 = blocks["x0"], blocks["x1"], blocks["x3"]
    # a row of T: n == tStride - 64, n == tStride - 63
    t, _, segs = train.strides(fl, x0[0].size, x0[1].size)
    assert t - 64 == x0[0].size and segs == 1
    _pair(orc, train, fl, blocks, x0, x0[1].size, x0[0].size, x0[1].size, False)
    t, _, segs = train.strides(fl, x1[0].size - 1, x1[1].size)
    assert t - 63 == x1[0].size and segs == 1
    _pair(orc, train, fl, blocks, x1, x1[1].size, x1[0].size - 1, x1[1].size, True)
    # a row of pointers: cap == pStride - 64, cap == pStride - 63
    _, p, _ = train.strides(fl, x0[0].size, x0[1].size)
    assert p - 64 >= x0[1].size
    _pair(orc, train, fl, blocks, x0, p - 64, x0[0].size, x0[1].size, False)
    _pair(orc, train, fl, blocks, x0, p - 63, x0[0].size, x0[1].size, True)
    # the units: dx_segments(n) == maxSeg, == maxSeg + 1
    assert -(-x3[0].size // SEG) == 3
    assert train.strides(fl, x3[0].size, x3[1].size)[2] == 3 and train.strides(fl, 2 * SEG, x3[1].size)[2] == 2
    _pair(orc, train, fl, blocks, x3, x3[1].size, x3[0].size, x3[1].size, False)
    _pair(orc, train, fl, blocks, x3, x3[1].size, 2 * SEG, x3[1].size, True)


def _offsets(comp):
    """Where the offset fields of a valid block's sequences are."""
    at, ip, n = [], 0, comp.size
    while True:
        tok = int(comp[ip]); ip += 1
        ll = tok >> 4
        if ll == 15:
            while True:
                b = int(comp[ip]); ip += 1; ll += b
                if b != 255: break
        ip += ll
        if ip >= n:
            return at
        at.append(ip); ip += 2
        if tok & 15 == 15:
            while int(comp[ip]) == 255: ip += 1
            ip += 1


@pytest.mark.parametrize("name", list(FLAVOURS))
@pytest.mark.parametrize("segs", [3, 4])
def test_a_flagged_unit_leaves_the_block(orc, train, name, segs):
    """A block of three (four) segments, n a little over two (three) times kDxSeg, with an offset zeroed in its second segment: the
    stitch follows the chain as ever, the unit that meets the offset flags the block, every unit of the grid is still run by the
    driver as the kernel runs it, and the block is left (liblz4 fills such a match with zeros, lz4.c:499-507: the block is the
    one-wave decoder's, which does the same).  Undamaged, the same block is answered with the oracle's bytes."""
    rng = np.random.default_rng(segs)
    comp, plain = _block(rng, (segs - 1) * SEG + 64)
    assert -(-comp.size // SEG) == segs
    at = [a for a in _offsets(comp) if SEG + SEG // 2 <= a < 2 * SEG][0]
    bad = comp.copy(); bad[at:at + 2] = 0
    fl = FLAVOURS[name]
    good, out = train.call(fl, [comp], [plain.size], comp.size, plain.size)[0]
    want, wbytes = orc.decompress_safe(comp, plain.size)
    assert good == want == plain.size and np.array_equal(out, wbytes)
    ans, _ = train.call(fl, [bad], [plain.size], comp.size, plain.size)[0]
    assert ans == LEFT


def _rounds_loop(span):
    """The loop the parent wrote out three times: ceil(log2(span)) rounds bring every pointer home, one more sees that."""
    r = 1
    while r < MAX_ROUNDS and (1 << (r - 1)) < span:
        r += 1
    return r


def test_rounds_rule_equals_the_three_it_replaces(train):
    spans = {1, 2, 3} | {(1 << k) + d for k in range(1, 32) for d in (-1, 0, 1)} | {1 << 40, (1 << 31) - 1, 1 << 31, (1 << 31) + 1}
    for span in sorted(spans):
        got = train.L.emu_dx_rounds_for(span)
        assert got == _rounds_loop(span) == min(MAX_ROUNDS, (span - 1).bit_length() + 1), span
        # dxb_rounds(maxOut): the same loop over the call's largest output
        assert train.L.emu_dxb_rounds(span) == _rounds_loop(span) == train.L.emu_dx_rounds(1, 1, span)
    assert train.L.emu_dx_rounds_for(1 << 40) == MAX_ROUNDS and train.L.emu_dx_rounds_for(1 << 31) == MAX_ROUNDS
    # kDxRounds = 24: 2^24 > kDxMaxOut, for any call
    assert (1 << 24) > DX_MAX_OUT > (1 << 22) and train.L.emu_dx_rounds_for(DX_MAX_OUT) == 24
    for nb, max_out in ((1, 100), (16, DX_MAX_OUT), (64, 1 << 30)):
        assert train.L.emu_dx_rounds(0, nb, max_out) == 24
    # launch_dx_train's loop: the call's total output, each block's clamped to kDxMaxOut, and the history in front of it
    for nb in (1, 2, 3, 16, 64, 511, 512, 513, 4096, 65535):
        for max_out in (1, 100, 65536, (1 << 20) - 1, 1 << 20, DX_MAX_OUT - 1, DX_MAX_OUT, DX_MAX_OUT + 1, 1 << 30):
            assert train.L.emu_dx_rounds(2, nb, max_out) == _rounds_loop(nb * min(max_out, DX_MAX_OUT) + HIST), (nb, max_out)
