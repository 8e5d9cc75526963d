"""The VAD gate (include/nnn_gate.h) under the test-only SIMT interpreter: audio, open flags and exported records
bit for bit against the NumPy restatement of the header's rule (tests/gate_cases.py), across every cut into calls, layout, alignment,
format and mask, in place and out of place, and everything the C ABI refuses."""
import os
import re
import subprocess

import pytest

import gate_cases as gc
from conftest import ROOT


@pytest.fixture(scope="module")
def mem():
    return gc.HostMem()


def test_abi_symbols():
    """The functions nnn_gate.h declares are _ffi.GATE_SYMBOLS, disjoint from every other list, and the built library exports each."""
    from nnnoiseless_amd import _ffi
    from nnnoiseless_amd.build import build_library
    src = open(os.path.join(ROOT, "include", "nnn_gate.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b((?:nnn|rnnoise)_[a-z0-9_]+)\s*\(", src))
    assert declared == set(_ffi.GATE_SYMBOLS) and len(_ffi.GATE_SYMBOLS) == 11
    out = subprocess.check_output(["nm", "-D", "--defined-only", build_library()]).decode()
    for sym in declared:
        assert re.search(rf"\bT {sym}\b", out), sym
    others = [v for k, v in vars(_ffi).items() if k.endswith("_SYMBOLS") and k != "GATE_SYMBOLS"]
    assert len(others) >= 9 and not any(set(_ffi.GATE_SYMBOLS) & set(o) for o in others)
    for name, value in (("MAX_LOOKBACK", _ffi.GATE_MAX_LOOKBACK), ("MAX_GRACE", _ffi.GATE_MAX_GRACE), ("STATE_VERSION", _ffi.GATE_STATE_VERSION)):
        assert re.search(rf"#define NNN_GATE_{name} (\d+)", src).group(1) == str(value)
    assert int(re.search(r"#define NNN_GATE_NEVER (0x[0-9a-f]+)", src).group(1), 16) == _ffi.GATE_NEVER
    assert int(re.search(r"#define NNN_GATE_STATE_MAGIC (0x[0-9A-Fa-f]+)u", src).group(1), 16) == _ffi.GATE_STATE_MAGIC
    assert _ffi.GATE_STATE_DTYPE.itemsize == _ffi.GATE_STATE_BYTES and _ffi.GATE_PARAMS_DTYPE.itemsize == 16


@pytest.mark.parametrize("S, T", gc.SHAPES)
def test_against_the_restatement(hostsim_lib, mem, S, T):
    gc.check_restatement(hostsim_lib, mem, S, T, rots=(0, 1, 2, 3) if S < 70 else (0, 3))


def test_chunking(hostsim_lib, mem):
    gc.check_chunking(hostsim_lib, mem)


def test_in_place_equals_out_of_place(hostsim_lib, mem):
    gc.check_in_place(hostsim_lib, mem)


def test_layout_and_formats(hostsim_lib, mem):
    gc.check_layout(hostsim_lib, mem)


def test_transparency_and_mute(hostsim_lib, mem):
    gc.check_transparency(hostsim_lib, mem)


def test_ramp(hostsim_lib, mem):
    gc.check_ramp(hostsim_lib, mem)


def test_live_mask(hostsim_lib, mem):
    gc.check_live(hostsim_lib, mem)


def test_reset_set_params_export_import(hostsim_lib, mem):
    gc.check_state(hostsim_lib, mem)


def test_host_call(hostsim_lib, mem):
    gc.check_host_call(hostsim_lib, mem)


def test_refusals(hostsim_lib, mem):
    gc.check_refusals(hostsim_lib, mem)


def test_missing_symbols_are_an_error():
    """A library without nnn_gate_* gives the scorer's kind of error, not an AttributeError."""
    from nnnoiseless_amd.gate import VadGate

    class Old:
        class L:
            pass

    with pytest.raises(RuntimeError, match=r"has no VAD gate \(nnn_gate_\*\)"):
        VadGate(4, lib=Old())
