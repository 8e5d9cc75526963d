"""The rate adapter (include/nnn_rate.h) under the test-only SIMT interpreter: source-rate samples in, source-rate
samples out, bit for bit the composition resampler -> BatchDenoiser.process -> resampler at the inverse ratio (tests/rate_cases.py),
whatever the chunking, the sample format, and the resets and holds in between.  3 streams, about 5 frames."""
import os
import re
import subprocess

import numpy as np
import pytest

import rate_cases as rc
from conftest import ROOT

S = 3
RATES = [16000.0, 44100.0, 8000.0, 96000.0]


def _n(rate, frames=5):
    return int(rate * frames / 100) + 7   # about `frames` frames' worth, not a whole number of them


@pytest.mark.parametrize("rate", RATES)
def test_composition_bit_for_bit(hostsim_lib, oracle_mod, rate):
    """Cuts of 1, 7, an empty call, 250 and the rest: count, every bit of audio and VAD, and the carried partial frame."""
    r, _, _ = rc.check_composition(hostsim_lib, oracle_mod, S, _n(rate), rate, (1, 7, 0, 250))
    assert r["n_frames"][0] == 0 and r["n_frames"][2] == 0    # calls that complete no frame say so (and return no VAD row)
    assert r["n_out"][2] == 0                                  # the empty call: everything its predecessors could complete is out already
    assert sum(r["n_frames"]) == 5


@pytest.mark.parametrize("rate", [16000.0, 44100.0])
def test_one_call_equals_ticks(hostsim_lib, rate):
    x = rc.signal(S, _n(rate), rate, seed=11)
    tick = int(rate / 100)
    one = rc.run_adapter(hostsim_lib, x, rate, ())
    ticks = rc.run_adapter(hostsim_lib, x, rate, [tick] * (x.shape[1] // tick))
    assert np.array_equal(rc.bits(one["out"]), rc.bits(ticks["out"])) and np.array_equal(rc.bits(one["vad"]), rc.bits(ticks["vad"]))
    assert one["carried"][-1] == ticks["carried"][-1]


@pytest.mark.parametrize("rate", [16000.0, 44100.0])
def test_int16_is_the_f32_path_rounded(hostsim_lib, rate):
    rc.check_int16(hostsim_lib, S, _n(rate), rate, (1, 7, 250))


def test_reset_streams(hostsim_lib, oracle_mod):
    rc.check_reset(hostsim_lib, oracle_mod, S, 6, 2)


def test_hold_and_resume(hostsim_lib, oracle_mod):
    rc.check_hold(hostsim_lib, oracle_mod, S, 6, 2)


def test_hold_at_44k1(hostsim_lib, oracle_mod):
    """A held stream at a rate whose tables are built every call: accepted, and the live streams' bits are the undisturbed run's."""
    rc.check_hold(hostsim_lib, oracle_mod, S, 6, 1, rate=44100.0, tick=441)


def test_refusals_change_nothing(hostsim_lib, oracle_mod):
    import nnnoiseless_amd as nn
    from nnnoiseless_amd.pcm import RateAdapter
    rate, tick = 16000.0, 160
    x = rc.signal(S, 5 * tick, rate, seed=13)
    want, vad, _ = rc.yardstick(hostsim_lib, oracle_mod, x, rate)
    bd = nn.BatchDenoiser(S, lib=hostsim_lib)
    for bad in (0.0, 48000.0):
        with pytest.raises(RuntimeError):
            RateAdapter(bd, bad, tick)
        assert "rate" in hostsim_lib.error() or "48000" in hostsim_lib.error()
    ra = RateAdapter(bd, rate, tick)
    bd.analyze(np.zeros((S, 1, 480), np.float32))              # frames pending: refused like every processing call
    with pytest.raises(RuntimeError, match="pending"):
        ra.process(x[:, :tick])
    bd.reset()                                                 # drops them: the batch is fresh again
    outs, vads = [], []
    for k in range(5):
        if k == 1:
            with pytest.raises(RuntimeError, match="cap_out"):
                ra.process(x[:, :tick], out=np.zeros((S, ra.max_output(tick) - 1), np.float32))
        if k == 2:
            with pytest.raises(RuntimeError, match="max_in"):
                ra.process(np.zeros((S, tick + 1), np.float32))
        if k == 3:
            with pytest.raises(RuntimeError, match="cap_frames"):
                ra.process(x[:, :tick], vad=np.zeros((ra.max_frames(tick) - 1, S), np.float32))
        y, v = ra.process(x[:, k * tick:(k + 1) * tick])
        outs.append(y.copy())
        vads.append(v.copy())
    assert np.array_equal(rc.bits(np.concatenate(outs, axis=1)), rc.bits(want)) and np.array_equal(rc.bits(np.concatenate(vads)), rc.bits(vad))
    assert ra.carried() == 2
    ra.close()
    bd.close()


def test_tables_are_memoised(hostsim_lib):
    """The schedule of a leg is a pure function of (position bits, idx, credit, n_in): at 16 kHz ticks the key recurs from the third
    call on (the first differs by idx alone) and no table is built any more; on the 44.1 kHz up-leg the f64 position drifts in its last
    bits and every call builds one."""
    r = rc.run_adapter(hostsim_lib, rc.signal(S, 6 * 160, 16000.0), 16000.0, [160] * 5)
    assert r["tables"][1] == (2, 2) and all(t == (2, 2) for t in r["tables"][1:])
    r = rc.run_adapter(hostsim_lib, rc.signal(S, 6 * 441, 44100.0), 44100.0, [441] * 5)
    assert [t[0] for t in r["tables"]] == [1, 2, 3, 4, 5, 6]


def test_abi_symbols():
    """The functions nnn_rate.h declares are _ffi.RATE_SYMBOLS, and the built library exports each (as test_abi.py reads them)."""
    from nnnoiseless_amd import _ffi
    from nnnoiseless_amd.build import build_library
    src = open(os.path.join(ROOT, "include", "nnn_rate.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b((?:nnn|rnnoise)_[a-z0-9_]+)\s*\(", src))
    assert declared == set(_ffi.RATE_SYMBOLS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", build_library()]).decode()
    for sym in declared:
        assert re.search(rf"\bT {sym}\b", out), sym
