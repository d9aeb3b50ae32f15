"""The two owner types of the ctx's stream-ordered device workspaces (plz4_amd/csrc/stream_ws.h: StreamOrder with its scope guard
MarkOnExit, DeviceBuffer) compiled for the CPU against a recording stand-in for the HIP calls they use
(tests/emu/emu_stream_ws.cpp).  Everything is asserted from the log of those calls: what is issued, in which order, and what is
not issued at all."""
import ctypes as C
import os
import subprocess

import pytest

from orclib import ROOT

SRC = os.path.join(ROOT, "tests", "emu", "emu_stream_ws.cpp")
HDR = os.path.join(ROOT, "plz4_amd", "csrc", "stream_ws.h")
SO = os.path.join(ROOT, "tests", "emu", "_build", "libemu_stream_ws.so")
OUT_OF_MEMORY, UNKNOWN = 2, 999


class Ws:
    def __init__(self):
        newest = max(os.path.getmtime(p) for p in (SRC, HDR))
        if not os.path.exists(SO) or os.path.getmtime(SO) < newest:
            os.makedirs(os.path.dirname(SO), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", SO, SRC])
        L = self.L = C.CDLL(SO)
        L.ws_log.restype = C.c_char_p
        for f in ("ws_stream", "ws_event", "ws_bytes"):
            getattr(L, f).restype = C.c_long
        L.ws_reserve.argtypes = [C.c_long]
        L.ws_reserve_on_stream.argtypes = [C.c_long, C.c_int]

    def calls(self, clear=True):
        """[(name, arg, arg)] since the log was last cleared"""
        out = [(a, int(b), int(c)) for a, b, c in (ln.split() for ln in self.L.ws_log().decode().splitlines())]
        if clear:
            self.L.ws_clear_log()
        return out

    def names(self):
        return [c[0] for c in self.calls()]


@pytest.fixture()
def ws():
    w = Ws()
    w.L.ws_reset()
    yield w
    w.L.ws_reset()


def test_order_wait_only_behind_a_job_on_another_stream(ws):
    L = ws.L
    assert L.ws_wait(1) == 0 and L.ws_wait(2) == 0
    assert ws.calls() == []                                        # before any mark: nothing
    assert L.ws_mark(1) == 0
    ev = L.ws_event()
    assert ws.calls() == [("hipEventCreateWithFlags", ev, 0), ("hipEventRecord", ev, 1)]     # (timing disabled: the plain name)
    assert L.ws_pending() == 1 and L.ws_stream() == 1
    assert L.ws_wait(1) == 0
    assert ws.calls() == []                                        # the stream of the last job: nothing
    assert L.ws_wait(2) == 0
    assert ws.calls() == [("hipStreamWaitEvent", 2, ev)]           # another stream: exactly one device-side wait
    assert L.ws_mark(2) == 0
    assert ws.calls() == [("hipEventRecord", ev, 2)]               # the event is created once
    assert L.ws_stream() == 2
    assert L.ws_wait(2) == 0 and ws.calls() == []
    assert L.ws_wait(1) == 0 and ws.names() == ["hipStreamWaitEvent"]


def test_order_drain_and_idle(ws):
    L = ws.L
    assert L.ws_idle() == 1 and L.ws_drain() == 0
    assert ws.calls() == []                                        # nothing pending: neither a query nor a wait
    L.ws_mark(3)
    ev = L.ws_event()
    ws.calls()
    L.ws_query_not_ready(1)
    assert L.ws_idle() == 0
    assert ws.names() == ["hipEventQuery", "hipGetLastError"] and L.ws_last_error() == 0     # hipErrorNotReady is cleared
    L.ws_query_not_ready(0)
    assert L.ws_idle() == 1 and ws.names() == ["hipEventQuery"]
    assert L.ws_pending() == 1                                     # (asking is not waiting)
    assert L.ws_drain() == 0
    assert ws.calls() == [("hipEventSynchronize", ev, 0)] and L.ws_pending() == 0
    assert L.ws_drain() == 0 and L.ws_wait(4) == 0 and ws.calls() == []
    # a drain that fails leaves the job pending and hands the error on
    L.ws_mark(3); ws.calls()
    L.ws_sync_fails(1)
    assert L.ws_drain() == UNKNOWN and L.ws_pending() == 1


def test_reserve_within_the_size_issues_nothing(ws):
    L = ws.L
    assert L.ws_reserve(1000) == 0
    assert ws.calls() == [("hipMalloc", 1000, 0)]                  # nothing held: nothing to wait for or to free
    assert L.ws_bytes() == 1000 and L.ws_has_memory() == 1
    L.ws_mark(1); ws.calls()
    for need in (1, 999, 1000):
        assert L.ws_reserve(need) == 0
    assert ws.calls() == [] and L.ws_bytes() == 1000 and L.ws_pending() == 1


def test_reserve_beyond_the_size_drains_then_frees_then_allocates(ws):
    L = ws.L
    L.ws_reserve(1000); L.ws_mark(1)
    ev = L.ws_event()
    ws.calls()
    assert L.ws_reserve(1001) == 0
    assert ws.calls() == [("hipEventSynchronize", ev, 0), ("hipFree", 0, 0), ("hipMalloc", 1001, 0)]
    assert L.ws_bytes() == 1001 and L.ws_pending() == 0 and L.ws_live_allocations() == 1
    # not pending: nothing to wait for
    assert L.ws_reserve(5000) == 0
    assert ws.names() == ["hipFree", "hipMalloc"]
    # a drain that fails: its error, and nothing was freed under the job
    L.ws_mark(2); ws.calls()
    L.ws_sync_fails(1)
    assert L.ws_reserve(6000) == -UNKNOWN
    assert ws.names() == ["hipEventSynchronize"] and L.ws_bytes() == 5000 and L.ws_has_memory() == 1


def test_reserve_of_a_staging_slot_waits_for_the_slots_stream(ws):
    L = ws.L
    assert L.ws_reserve_on_stream(100, 7) == 0
    assert ws.calls() == [("hipMalloc", 100, 0)]
    assert L.ws_reserve_on_stream(100, 7) == 0 and ws.calls() == []
    assert L.ws_reserve_on_stream(200, 7) == 0
    assert ws.calls() == [("hipStreamSynchronize", 7, 0), ("hipFree", 0, 0), ("hipMalloc", 200, 0)]


def test_refused_reserve_leaves_the_buffer_empty_and_the_error_cleared(ws):
    L = ws.L
    L.ws_reserve(1000); L.ws_mark(1); ws.calls()
    L.ws_refuse_mallocs(1)
    assert L.ws_reserve(1 << 40) == 1                              # refused: reported, no error
    names = ws.names()
    assert names == ["hipEventSynchronize", "hipFree", "hipMalloc", "hipGetLastError"]
    assert names.index("hipEventSynchronize") < names.index("hipFree")
    assert L.ws_has_memory() == 0 and L.ws_bytes() == 0 and L.ws_last_error() == 0 and L.ws_live_allocations() == 0
    # the caller's next, smaller request
    assert L.ws_reserve(500) == 0
    assert ws.calls() == [("hipMalloc", 500, 0)] and L.ws_bytes() == 500 and L.ws_has_memory() == 1
    # refused on an empty buffer (the second level-1 workspace: whole or not at all)
    L.ws_reset()
    L.ws_refuse_mallocs(1)
    assert L.ws_reserve(4096) == 1
    assert ws.names() == ["hipMalloc", "hipGetLastError"] and L.ws_has_memory() == 0 and L.ws_last_error() == 0


@pytest.mark.parametrize("early", [False, True])
def test_guard_marks_once_on_every_way_out(ws, early):
    L = ws.L
    rc = L.ws_launch(5, 1, int(early))
    assert rc == (UNKNOWN if early else 0)
    ev = L.ws_event()
    assert ws.calls() == [("enqueue", 5, 0), ("hipEventCreateWithFlags", ev, 0), ("hipEventRecord", ev, 5)]      # exactly one record
    assert L.ws_pending() == 1 and L.ws_stream() == 5
    L.ws_launch(6, 1, int(early))
    assert ws.calls() == [("enqueue", 6, 0), ("hipEventRecord", ev, 6)]
    assert L.ws_stream() == 6


@pytest.mark.parametrize("early", [False, True])
def test_guard_that_was_never_armed_records_nothing(ws, early):
    L = ws.L
    L.ws_launch(5, 0, int(early))
    assert ws.calls() == [("enqueue", 5, 0)]
    assert L.ws_pending() == 0 and L.ws_event() == 0


def test_release_and_destroy_drain_before_they_free(ws):
    L = ws.L
    L.ws_reserve(1000); L.ws_mark(9)
    ev = L.ws_event()
    ws.calls()
    assert L.ws_release() == 0
    assert ws.calls() == [("hipEventSynchronize", ev, 0), ("hipFree", 0, 0)]
    assert L.ws_pending() == 0 and L.ws_stream() == 0              # not pending, its stream forgotten
    assert L.ws_has_memory() == 0 and L.ws_bytes() == 0 and L.ws_live_allocations() == 0
    assert L.ws_wait(3) == 0 and L.ws_release() == 0 and ws.calls() == []
    # the owner's teardown: the buffer behind the last job, then the order's event
    L.ws_reserve(64); L.ws_mark(9); ws.calls()
    L.ws_release(); L.ws_destroy()
    assert ws.calls() == [("hipEventSynchronize", ev, 0), ("hipFree", 0, 0), ("hipEventDestroy", ev, 0)]
    assert L.ws_event() == 0 and L.ws_pending() == 0 and L.ws_stream() == 0
    # destroy by itself waits for a job that is still pending
    L.ws_mark(2)
    ev2 = L.ws_event()
    ws.calls()
    L.ws_destroy()
    assert ws.calls() == [("hipEventSynchronize", ev2, 0), ("hipEventDestroy", ev2, 0)]
    L.ws_destroy()
    assert ws.calls() == []
