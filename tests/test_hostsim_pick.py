"""The talker picker (include/nnn_pick.h) under the test-only SIMT interpreter: talk, dominant and level bit for bit
against the NumPy restatement of the header's rule (tests/pick_cases.py), across every policy, cut into calls, layout, alignment, format
and mask, what the header says follows from the rule, and everything the C ABI refuses."""
import os
import re
import subprocess

import pytest

import pick_cases as pc
from conftest import ROOT


@pytest.fixture(scope="module")
def mem():
    return pc.HostMem()


def test_abi_symbols():
    """The functions nnn_pick.h declares are _ffi.PICK_SYMBOLS, disjoint from every other list, the built library exports each, and the
    header's constants are _ffi's."""
    from nnnoiseless_amd import _ffi
    from nnnoiseless_amd.build import build_library
    src = open(os.path.join(ROOT, "include", "nnn_pick.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b((?:nnn|rnnoise)_[a-z0-9_]+)\s*\(", src))
    assert declared == set(_ffi.PICK_SYMBOLS) and len(_ffi.PICK_SYMBOLS) == 12
    out = subprocess.check_output(["nm", "-D", "--defined-only", build_library()]).decode()
    for sym in declared:
        assert re.search(rf"\bT {sym}\b", out), sym
    others = [v for k, v in vars(_ffi).items() if k.endswith("_SYMBOLS") and k != "PICK_SYMBOLS"]
    assert len(others) >= 11 and not any(set(_ffi.PICK_SYMBOLS) & set(o) for o in others)
    for name, value in (("MAX_K", _ffi.PICK_MAX_K), ("MAX_STICK", _ffi.PICK_MAX_STICK), ("SEG_ROOM", _ffi.PICK_SEG_ROOM),
                        ("WAVE_ROOM", _ffi.PICK_WAVE_ROOM), ("FRAME", 480)):
        assert re.search(rf"#define NNN_PICK_{name} (\d+)", src).group(1) == str(value)


@pytest.mark.parametrize("k, decay, stick", pc.POLICIES)
@pytest.mark.parametrize("S, T", pc.SHAPES)
def test_against_the_restatement(hostsim_lib, mem, S, T, k, decay, stick):
    pc.check_restatement(hostsim_lib, mem, S, T, k, decay, stick)


def test_chunking(hostsim_lib, mem):
    pc.check_chunking(hostsim_lib, mem)


def test_layout_and_formats(hostsim_lib, mem):
    pc.check_layout(hostsim_lib, mem)


def test_live_mask(hostsim_lib, mem):
    pc.check_live(hostsim_lib, mem)


def test_unread_inputs_do_not_matter(hostsim_lib, mem):
    pc.check_unread(hostsim_lib, mem)


def test_non_finite_samples_measure_silent(hostsim_lib, mem):
    pc.check_nonfinite(hostsim_lib, mem)


def test_consequences_of_the_rule(hostsim_lib, mem):
    pc.check_consequences(hostsim_lib, mem)


def test_bits_do_not_depend_on_n_streams_or_labels(hostsim_lib, mem):
    pc.check_n_streams(hostsim_lib, mem)


def test_reset_and_setters(hostsim_lib, mem):
    pc.check_state(hostsim_lib, mem)


def test_host_call(hostsim_lib, mem):
    pc.check_host_call(hostsim_lib, mem)


def test_refusals(hostsim_lib, mem):
    pc.check_refusals(hostsim_lib, mem)


def test_missing_symbols_are_an_error():
    """A library without nnn_pick_* gives the mixer's kind of error, not an AttributeError."""
    from nnnoiseless_amd.pick import TalkerPicker

    class Old:
        class L:
            pass

    with pytest.raises(RuntimeError, match=r"has no talker picker \(nnn_pick_\*\)"):
        TalkerPicker(4, lib=Old())
