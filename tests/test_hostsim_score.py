"""The scorer (include/nnn_score.h) under the test-only SIMT interpreter: frame sums and totals bit for bit
against the NumPy restatement of the header's summation order (tests/score_cases.py), across every cut into calls, layout, alignment
and mask, and everything the C ABI refuses."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import score_cases as sc
from conftest import ROOT


@pytest.fixture(scope="module")
def mem():
    return sc.HostMem()


def test_abi_symbols():
    """The functions nnn_score.h declares are _ffi.SCORE_SYMBOLS, and the built library exports each (as test_abi.py reads them)."""
    from nnnoiseless_amd import _ffi
    from nnnoiseless_amd.build import build_library
    src = open(os.path.join(ROOT, "include", "nnn_score.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b((?:nnn|rnnoise)_[a-z0-9_]+)\s*\(", src))
    assert declared == set(_ffi.SCORE_SYMBOLS) and len(_ffi.SCORE_SYMBOLS) == 9
    out = subprocess.check_output(["nm", "-D", "--defined-only", build_library()]).decode()
    for sym in declared:
        assert re.search(rf"\bT {sym}\b", out), sym
    assert not set(_ffi.SCORE_SYMBOLS) & set(_ffi.BATCH_SYMBOLS)
    assert re.search(r"#define NNN_SCORE_MAX_DELAY (\d+)", src).group(1) == str(_ffi.SCORE_MAX_DELAY)


@pytest.mark.parametrize("S, T", sc.SHAPES)
def test_against_the_restatement(hostsim_lib, mem, S, T):
    sc.check_restatement(hostsim_lib, mem, S, T)


def test_chunking(hostsim_lib, mem):
    sc.check_chunking(hostsim_lib, mem)


def test_layout_and_alignment(hostsim_lib, mem):
    sc.check_layout(hostsim_lib, mem)


def test_a_long_call(hostsim_lib, mem):
    """11 frames: three runs of frames per stream, the last one short, with a mask that switches frames off inside the runs."""
    S, T = 6, 11
    d = sc.mixed_delays(S)
    r, y = sc.signals(71, S, T)
    valid = (np.arange(T * S).reshape(T, S) % 3 != 0).astype(np.uint8)
    s, rs = sc.scorer(hostsim_lib, S, d), sc.Restated(S, 960, d)
    sc.assert_same(sc.device_call(s, mem, r, y, valid), rs.accumulate(r, y, valid))
    sc.assert_totals(s, rs)
    s.close()


def test_valid_mask(hostsim_lib, mem):
    sc.check_valid(hostsim_lib, mem)


def test_exact_identities(hostsim_lib, mem):
    sc.check_identities(hostsim_lib, mem)


def test_range_and_non_finite(hostsim_lib, mem):
    sc.check_range(hostsim_lib, mem)


def test_reset_and_set_delay(hostsim_lib, mem):
    sc.check_reset(hostsim_lib, mem)


def test_the_same_call_twice(hostsim_lib, mem):
    sc.check_twice(hostsim_lib, mem)


def test_host_call(hostsim_lib, mem):
    sc.check_host_call(hostsim_lib, mem)


def test_small_max_delay(hostsim_lib, mem):
    """max_delay 0 (no history at all) and 6 (a history row that is no whole 16-byte word)."""
    for H, d in ((0, [0, 0, 0]), (6, [6, 5, 0])):
        s, rs = sc.scorer(hostsim_lib, 3, d, max_delay=H), sc.Restated(3, H, d)
        for call in range(2):
            r, y = sc.signals(40 + call, 3, 2)
            sc.assert_same(sc.device_call(s, mem, r, y), rs.accumulate(r, y), f"max_delay {H} call {call}")
        sc.assert_totals(s, rs)
        s.close()


def test_refusals(hostsim_lib, mem):
    """Every refusal with its text; a refused call changes nothing."""
    from nnnoiseless_amd import _ffi
    from nnnoiseless_amd.score import Scorer
    lib, L = hostsim_lib, hostsim_lib.L

    def refused(rc, text):
        assert rc != 0 and text in lib.error(), (rc, text, lib.error())

    for bad in ((0, 960), (-1, 960), (4, -1), (4, 961)):
        assert not L.nnn_score_create(bad[0], bad[1], 0)
        assert ("n_streams" if bad[0] < 1 else "max_delay") in lib.error()
    with pytest.raises(RuntimeError, match="max_delay = 961 outside"):
        Scorer(4, 961, lib=lib)
    L.nnn_score_destroy(None)
    f32 = np.zeros((4, 2, sc.FRAME), np.float32)
    p = _ffi.ptr(f32)
    d4 = np.zeros(4, np.int32)
    refused(L.nnn_score_accumulate_device(None, p, p, None, None, 2, 960, 480, None), "null scorer")
    refused(L.nnn_score_accumulate_host(None, p, p, None, None, 2), "null scorer")
    refused(L.nnn_score_set_delay(None, None, 4, _ffi.ptr(d4)), "null scorer")
    refused(L.nnn_score_get_delay(None, None, 4, _ffi.ptr(d4)), "null scorer")
    refused(L.nnn_score_reset(None, None, 0), "null scorer")
    refused(L.nnn_score_totals(None, None, None), "null scorer")
    refused(L.nnn_score_totals_device(None, None, None, None), "null scorer")
    d = np.array([3, 480, 960, 0])
    s, rs = sc.scorer(lib, 4, d, max_delay=960), sc.Restated(4, 960, d)
    r, y = sc.signals(50, 4, 2)
    sc.assert_same(sc.device_call(s, mem, r, y), rs.accumulate(r, y))
    h = s._h
    refused(L.nnn_score_accumulate_device(h, None, p, None, None, 2, 960, 480, None), "null reference signal")
    refused(L.nnn_score_accumulate_device(h, p, None, None, None, 2, 960, 480, None), "null test signal")
    refused(L.nnn_score_accumulate_host(h, None, p, None, None, 2), "null reference signal")
    refused(L.nnn_score_accumulate_host(h, p, None, None, None, 2), "null test signal")
    for n in (0, -3):
        refused(L.nnn_score_accumulate_device(h, p, p, None, None, n, 960, 480, None), f"n_frames = {n}")
        refused(L.nnn_score_accumulate_host(h, p, p, None, None, n), f"n_frames = {n}")
    refused(L.nnn_score_accumulate_device(h, f32.ctypes.data + 2, p, None, None, 2, 960, 480, None), "4-byte samples")
    refused(L.nnn_score_accumulate_device(h, p, p, None, f32.ctypes.data + 4, 2, 960, 480, None), "8-byte values")
    with pytest.raises(RuntimeError, match=r"entry 1: delay 961 outside \[0, 960\]"):
        s.set_delay([0, 1], [5, 961])
    with pytest.raises(RuntimeError, match=r"entry 0: delay -1 outside"):
        s.set_delay(None, [-1, 0, 0, 0])
    with pytest.raises(RuntimeError, match=r"stream 4 outside \[0, 4\)"):
        s.set_delay([0, 4], [5, 5])
    with pytest.raises(RuntimeError, match=r"stream -1 outside"):
        s.reset([-1])
    with pytest.raises(RuntimeError, match=r"stream 7 outside"):
        s.delay([7])
    with pytest.raises(RuntimeError, match="5 entries for 4 streams"):
        lib.check(L.nnn_score_set_delay(h, None, 5, _ffi.ptr(np.zeros(5, np.int32))))
    refused(L.nnn_score_set_delay(h, None, 4, None), "null delays")
    refused(L.nnn_score_set_delay(h, None, -1, _ffi.ptr(d4)), "n = -1")
    with pytest.raises(ValueError):
        s.set_delay([0, 1], [1, 2, 3])
    with pytest.raises(ValueError):
        s.accumulate(f32[:3], f32[:3])
    with pytest.raises(ValueError):
        s.accumulate(f32, f32, valid=np.ones((3, 4)))
    small = sc.scorer(lib, 2, max_delay=100)
    with pytest.raises(RuntimeError, match=r"delay 101 outside \[0, 100\]"):
        small.set_delay([1], 101)
    small.close()
    # nothing of that changed the object: delays, totals and history are where the first call left them
    assert np.array_equal(s.delay(), d)
    sc.assert_totals(s, rs)
    r, y = sc.signals(51, 4, 1)
    sc.assert_same(sc.device_call(s, mem, r, y), rs.accumulate(r, y), "after the refusals")
    assert L.nnn_score_set_delay(h, None, 0, None) == 0 and L.nnn_score_reset(h, (C.c_int * 1)(0), 0) == 0
    sc.assert_totals(s, rs)
    s.close()


def test_missing_symbols_are_an_error():
    """A library without nnn_score_* gives the trainer's kind of error, not an AttributeError."""
    from nnnoiseless_amd.score import Scorer

    class Old:
        class L:
            pass

    with pytest.raises(RuntimeError, match=r"has no scorer \(nnn_score_\*\)"):
        Scorer(4, lib=Old())
