"""The conference mixer (include/nnn_mix.h) under the test-only SIMT interpreter: audio and heard counts bit for
bit against the NumPy restatement of the header's rule (tests/mix_cases.py), across every cut into calls, layout, alignment, format pair
and mask, what the header says follows from the rule, and everything the C ABI refuses."""
import os
import re
import subprocess

import pytest

import mix_cases as mc
from conftest import ROOT


@pytest.fixture(scope="module")
def mem():
    return mc.HostMem()


def test_abi_symbols():
    """The functions nnn_mix.h declares are _ffi.MIX_SYMBOLS, disjoint from every other list, the built library exports each, and the
    header's constants are _ffi's."""
    from nnnoiseless_amd import _ffi
    from nnnoiseless_amd.build import build_library
    src = open(os.path.join(ROOT, "include", "nnn_mix.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b((?:nnn|rnnoise)_[a-z0-9_]+)\s*\(", src))
    assert declared == set(_ffi.MIX_SYMBOLS) and len(_ffi.MIX_SYMBOLS) == 10
    out = subprocess.check_output(["nm", "-D", "--defined-only", build_library()]).decode()
    for sym in declared:
        assert re.search(rf"\bT {sym}\b", out), sym
    others = [v for k, v in vars(_ffi).items() if k.endswith("_SYMBOLS") and k != "MIX_SYMBOLS"]
    assert len(others) >= 10 and not any(set(_ffi.MIX_SYMBOLS) & set(o) for o in others)
    for name, value in (("MAX_GAIN", _ffi.MIX_MAX_GAIN), ("TILE", _ffi.MIX_TILE), ("REG_TALKERS", _ffi.MIX_REG_TALKERS), ("FRAME", 480)):
        assert re.search(rf"#define NNN_MIX_{name} (\d+)", src).group(1) == str(value)


@pytest.mark.parametrize("S, T", mc.SHAPES)
def test_against_the_restatement(hostsim_lib, mem, S, T):
    mc.check_restatement(hostsim_lib, mem, S, T)


def test_chunking(hostsim_lib, mem):
    mc.check_chunking(hostsim_lib, mem)


def test_layout_and_formats(hostsim_lib, mem):
    mc.check_layout(hostsim_lib, mem)


def test_live_mask(hostsim_lib, mem):
    mc.check_live(hostsim_lib, mem)


def test_inaudible_inputs_do_not_leak(hostsim_lib, mem):
    mc.check_inaudible_nan(hostsim_lib, mem)


def test_consequences_of_the_rule(hostsim_lib, mem):
    mc.check_consequences(hostsim_lib, mem)


def test_non_finite_audible_samples(hostsim_lib, mem):
    mc.check_nonfinite(hostsim_lib, mem)


def test_bits_do_not_depend_on_n_streams(hostsim_lib, mem):
    mc.check_n_streams(hostsim_lib, mem)


def test_reset_and_setters(hostsim_lib, mem):
    mc.check_state(hostsim_lib, mem)


def test_host_call(hostsim_lib, mem):
    mc.check_host_call(hostsim_lib, mem)


def test_refusals(hostsim_lib, mem):
    mc.check_refusals(hostsim_lib, mem)


def test_missing_symbols_are_an_error():
    """A library without nnn_mix_* gives the gate's kind of error, not an AttributeError."""
    from nnnoiseless_amd.mix import ConferenceMixer

    class Old:
        class L:
            pass

    with pytest.raises(RuntimeError, match=r"has no mixer \(nnn_mix_\*\)"):
        ConferenceMixer(4, lib=Old())
