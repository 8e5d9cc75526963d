"""The network trainer (include/nnn_fit.h) under the test-only SIMT interpreter: forward outputs, loss terms and
the fifteen gradient tensors against the float64 autograd restatement (tests/fit_cases.py), judged by the float32 restatement's own
error; independence from the allocation and from earlier calls; Adam and the export bit for bit against NumPy; refusals."""
import ctypes as C
import os
import re
import subprocess

import pytest

import fit_cases as fc
from conftest import ROOT

TILE = 4   # NNN_FIT_TILE: the sequences a recurrence block owns (the kernels do not chunk the window)


def test_abi_symbols():
    """The functions nnn_fit.h declares are _ffi.FIT_SYMBOLS, the built library exports each, and the constants agree."""
    from nnnoiseless_amd import _ffi
    from nnnoiseless_amd.build import build_library
    src = open(os.path.join(ROOT, "include", "nnn_fit.h")).read()
    defines = dict(re.findall(r"#define (NNN_FIT_[A-Z_]+) (\d+)", src))
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//.*", "", src)
    declared = set(re.findall(r"\b(nnn_fit_[a-z0-9_]+)\s*\(", src))
    assert declared == set(_ffi.FIT_SYMBOLS) and len(_ffi.FIT_SYMBOLS) == 18
    out = subprocess.check_output(["nm", "-D", "--defined-only", build_library()]).decode()
    for sym in declared:
        assert re.search(rf"\bT {sym}\b", out), sym
    assert C.sizeof(_ffi.FitSettings) == 24 and C.sizeof(_ffi.FitRows) == 56
    assert int(defines["NNN_FIT_PARAMS"]) == _ffi.FIT_PARAMS == fc.NP_ and int(defines["NNN_FIT_TILE"]) == _ffi.FIT_TILE == TILE
    names = {"input_dense": "IN", "vad_gru": "VAD", "noise_gru": "NOISE", "denoise_gru": "DN", "denoise_output": "OUT", "vad_output": "VOUT"}
    end = 0
    for name, (off, shape) in _ffi.FIT_TENSORS.items():
        layer, kind = name.split(".")
        assert int(defines[f"NNN_FIT_OFF_{names[layer]}_{kind.upper()}"]) == off == end, name
        end = off + (shape[0] * shape[1] if len(shape) == 2 else shape[0])
    assert end == fc.NP_
    # the saved-activation footprint the header states: D, dD, gains, their deltas, vad and its delta, and per GRU neuron P (3), z, r, c, h, dh
    assert int(defines["NNN_FIT_ROW_BYTES"]) == 4 * (2 * 24 + 2 * 22 + 2 + 8 * (24 + 48 + 96))


@pytest.mark.parametrize("S, T", [(3, 5), (TILE + 1, 3), (5, 40), (2, 1)])
def test_against_float64(hostsim_lib, S, T):
    """A partial tile; two tiles, the second almost empty; a longer window; a single step with no recurrence.  Glorot parameters."""
    fc.check_case(hostsim_lib, S, T)


@pytest.mark.parametrize("kind", ["builtin", "sh"])
def test_templates_against_float64(hostsim_lib, kind):
    """(3, 8) with the built-in model and tests/golden/sh.rnn as templates: the activations come from the header bytes."""
    fc.check_case(hostsim_lib, 3, 8, kind)


def test_template_start(hostsim_lib):
    fc.check_template_start(hostsim_lib)


def test_independence(hostsim_lib):
    fc.check_independence(hostsim_lib)


def test_optimizer_bit_for_bit(hostsim_lib):
    fc.check_optimizer(hostsim_lib)


def test_export(hostsim_lib):
    fc.check_export(hostsim_lib)


def test_end_to_end(hostsim_lib):
    fc.check_end_to_end(hostsim_lib)


def test_refusals(hostsim_lib):
    fc.check_refusals(hostsim_lib)
