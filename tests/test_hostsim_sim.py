"""The noise simulator (include/nnn_sim.h) under the test-only SIMT interpreter: signals bit for bit against the
NumPy restatement of NoiseSimulator::next_frame (tests/sim_cases.py), rows bit for bit against the training-row call over the same
signals and within the usual bars against the oracle, and everything the C ABI refuses."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import sim_cases as sc
from conftest import ROOT


def test_abi_symbols():
    """The functions nnn_sim.h declares are _ffi.SIM_SYMBOLS, and the built library exports each (as test_abi.py reads them)."""
    from nnnoiseless_amd import _ffi
    from nnnoiseless_amd.build import build_library
    src = open(os.path.join(ROOT, "include", "nnn_sim.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b((?:nnn|rnnoise)_[a-z0-9_]+)\s*\(", src))
    assert declared == set(_ffi.SIM_SYMBOLS) and len(_ffi.SIM_SYMBOLS) == 13
    out = subprocess.check_output(["nm", "-D", "--defined-only", build_library()]).decode()
    for sym in declared:
        assert re.search(rf"\bT {sym}\b", out), sym
    assert C.sizeof(_ffi.SimParams) == 44 == _ffi.SIM_PARAMS_DTYPE.itemsize


def test_signals_against_the_restatement(hostsim_lib):
    """70 triples (a full tile and a partial one) x 26 frames, parameters changed between two calls: the three signals and the two
    labels equal the restatement bit for bit; the restatement itself is checked to reach every branch."""
    sc.check_signals_against_restatement(hostsim_lib)


def test_splitting_a_call(hostsim_lib):
    """26 frames as one call and as 1 + 24 + 1."""
    sc.check_split_calls(hostsim_lib)


@pytest.mark.parametrize("S, T", [(9, 26), (70, 7)])
def test_rows_bit_for_bit(hostsim_lib, S, T):
    """process = TrainingFeatures.process on a twin simulator's signals: more than one group, more than one tile."""
    sc.check_rows_against_twin(hostsim_lib, S, T)


def test_rows_against_the_oracle(hostsim_lib, oracle_mod, weights_bytes):
    """70 x 6 rows against oracle.training_rows on the restated signals, judged by train_fixtures.check_rows' absolute bars
    (sim_cases.check_rows_against_oracle says why those)."""
    sc.check_rows_against_oracle(hostsim_lib, oracle_mod, weights_bytes)


def test_reset(hostsim_lib):
    """reset (with the training object's) then the first call again gives the first call's bits; the parameters stay."""
    c = sc.case(9, 26)
    sim = c.simulator(hostsim_lib, c.p2)
    first = sim.process(c.sig_off[:5], c.noise_off[:5])
    sim.process(c.sig_off[5:9], c.noise_off[5:9])
    sim.reset()
    sim._features.reset()
    assert np.array_equal(sim.params().tobytes(), c.p2.tobytes())
    again = sim.process(c.sig_off[:5], c.noise_off[:5])
    assert np.array_equal(sc.bits(again), sc.bits(first))
    sim.reset()
    got = sim.signals(c.sig_off[:3], c.noise_off[:3])
    want = sc.restate(c.sig, c.noise, c.sig_off[:3], c.noise_off[:3], c.p2)[:5]
    sc.assert_equal_bits(got, want)
    sim.close()


def _device_signals(lib, sim, so, no):
    """nnn_sim_signals_device on host arrays (the interpreter's device memory is the host's)."""
    from nnnoiseless_amd import _ffi
    T, S = so.shape
    sig, noise, comb = (np.full((S, T, sc.FRAME), 7.0, np.float32) for _ in range(3))
    cut, vad = np.full((T, S), -9, np.int32), np.full((T, S), 7.0, np.float32)
    sim.signals_device(_ffi.ptr(so), _ffi.ptr(no), _ffi.ptr(sig), _ffi.ptr(noise), _ffi.ptr(comb), _ffi.ptr(cut), _ffi.ptr(vad), T,
                       T * sc.FRAME, sc.FRAME)
    return sig, noise, comb, cut, vad


def test_offsets(hostsim_lib):
    """Odd offsets, two triples on the same frame and a frame ending on the arena's last element work; one element further is refused
    by the host call with nothing changed, and through the device entry reads as zeros and sets nnn_sim_fault.  An arena that begins
    at an odd element of its buffer (adopt_device) gives the same bits."""
    from nnnoiseless_amd import _ffi, training
    c = sc.case(9, 26)
    S, T = c.S, 3
    so, no = c.sig_off[:T].copy(), c.noise_off[:T].copy()
    so[0, 0], so[0, 1], so[0, 2] = 1, 1, 3                      # odd, shared
    so[1, 3] = c.sig.size - sc.FRAME                            # ends on the last element
    no[1, 4] = c.noise.size - sc.FRAME
    so[2, 5], no[2, 6] = 0, 0                                   # begins on the first
    want = sc.restate(c.sig, c.noise, so, no, c.p2)[:5]
    sim = c.simulator(hostsim_lib, c.p2)
    sc.assert_equal_bits(sim.signals(so, no), want, "host")
    sim.reset()
    sc.assert_equal_bits(_device_signals(hostsim_lib, sim, so, no), want, "device")
    assert not sim.fault()
    # the same samples in buffers whose arenas begin 1 and 3 elements in: no 8-byte word of the arena is aligned as before
    pad_s, pad_n = np.concatenate([[11], c.sig]).astype(np.int16), np.concatenate([[5, 6, 7], c.noise]).astype(np.int16)
    sim.adopt_device(training.ARENA_SIGNAL, pad_s.ctypes.data + 2, c.sig.size, keep=pad_s)
    sim.adopt_device(training.ARENA_NOISE, pad_n.ctypes.data + 6, c.noise.size, keep=pad_n)
    sim.reset()
    sc.assert_equal_bits(sim.signals(so, no), want, "adopted")
    # one past the end: the host call refuses, state and outputs untouched
    sim.reset()
    mid = sim.signals(so[:1], no[:1])
    bad = so[1:].copy()
    bad[0, 3] += 1
    rows = np.full((2, S, 87), 3.0, np.float32)
    with pytest.raises(RuntimeError, match="leaves the arena"):
        sim.signals(bad, no[1:])
    with pytest.raises(RuntimeError, match="leaves the arena"):
        sim.process(bad, no[1:], rows)
    with pytest.raises(RuntimeError, match="noise offset"):
        sim.signals(so[1:], no[1:] + np.uint64(c.noise.size))
    assert (rows == 3.0).all() and not sim.fault()
    rest = sim.signals(so[1:], no[1:])
    sc.assert_equal_bits([np.concatenate([mid[i], rest[i]], axis=1 if i < 3 else 0) for i in range(5)], want, "after the refusals")
    # the device entry: that frame is 480 zeros, nothing else changes, the flag is set and stays
    sim.reset()
    bad_all = so.copy()
    bad_all[1, 3] += 1
    huge = no.copy()
    huge[2, 7] = np.uint64(2 ** 64 - 1)
    got = _device_signals(hostsim_lib, sim, bad_all, huge)
    zs, zn = np.concatenate([c.sig, np.zeros(sc.FRAME + 1, np.int16)]), np.concatenate([c.noise, np.zeros(sc.FRAME, np.int16)])
    zo = huge.copy()
    zo[2, 7] = c.noise.size
    zso = bad_all.copy()
    zso[1, 3] = c.sig.size + 1
    sc.assert_equal_bits(got, sc.restate(zs, zn, zso, zo, c.p2)[:5], "zeros")
    assert sim.fault()
    sim.reset()
    assert sim.fault()   # sticky
    sim.close()


def test_refusals(hostsim_lib):
    """Refused records change nothing; NULL handles and arenas, a call before both arenas are loaded, misaligned buffers."""
    from nnnoiseless_amd import _ffi, training
    from nnnoiseless_amd.training import NoiseSimulator, TrainingFeatures
    L = hostsim_lib.L
    c = sc.case(9, 26)
    assert not L.nnn_sim_create(None) and "null" in hostsim_lib.error()
    assert L.nnn_sim_reset(None) != 0 and L.nnn_sim_fault(None) < 0
    L.nnn_sim_destroy(None)
    sim = NoiseSimulator(TrainingFeatures(c.S, lib=hostsim_lib))
    assert np.array_equal(sim.params().tobytes(), training.default_params(c.S).tobytes())   # NoiseSimulator::new
    so, no = c.sig_off[:2], c.noise_off[:2]
    with pytest.raises(RuntimeError, match="signal arena is not loaded"):
        sim.signals(so, no)
    sim.load_signal(c.sig)
    with pytest.raises(RuntimeError, match="noise arena is not loaded"):
        sim.process(so, no)
    for call in (lambda: L.nnn_sim_load(sim._h, 1, None, 10), lambda: L.nnn_sim_load(sim._h, 1, _ffi.ptr(c.noise), 0),
                 lambda: L.nnn_sim_load(sim._h, 2, _ffi.ptr(c.noise), c.noise.size), lambda: L.nnn_sim_adopt_device(sim._h, 1, None, 10),
                 lambda: L.nnn_sim_adopt_device(sim._h, 1, c.noise.ctypes.data + 1, 10)):
        assert call() != 0
    with pytest.raises(ValueError):
        sim.load_noise(c.noise.astype(np.float32))
    sim.load_noise(c.noise)
    sim.set_params(None, c.p1)
    for field, value in (("signal_gain", np.nan), ("noise_gain", np.inf), ("sig_a", -np.inf), ("noise_b", np.nan), ("band_lp", 22), ("band_lp", -1)):
        recs = c.p2[:3].copy()
        recs[field][1] = value
        with pytest.raises(RuntimeError, match="not finite|band_lp"):
            sim.set_params([0, 1, 2], recs)
    with pytest.raises(RuntimeError, match="outside"):
        sim.set_params([0, c.S], c.p2[:2])
    with pytest.raises(RuntimeError, match="outside"):
        sim.params([-1])
    with pytest.raises(ValueError):
        sim.set_params([0, 1], c.p2[:3])
    assert np.array_equal(sim.params().tobytes(), c.p1.tobytes())                          # nothing changed
    sim.set_params([4, 2], c.p2[[4, 2]])
    assert np.array_equal(sim.params([2, 4]).tobytes(), c.p2[[2, 4]].tobytes())
    sim.set_params([4, 2], c.p1[[4, 2]])
    with pytest.raises(ValueError):
        sim.signals(so[:, :5], no[:, :5])
    T, S = so.shape
    buf = np.zeros(3 * S * T * sc.FRAME + 8, np.float32)
    lab_i, lab_f = np.zeros((T, S), np.int32), np.zeros((T, S), np.float32)
    n = S * T * sc.FRAME

    def dev(base=0, stream_stride=T * sc.FRAME, frame_stride=sc.FRAME, offs=_ffi.ptr(so), frames=T):
        p = buf.ctypes.data + 4 * base
        return L.nnn_sim_signals_device(sim._h, offs, _ffi.ptr(no), p, p + 4 * n, p + 8 * n, _ffi.ptr(lab_i), _ffi.ptr(lab_f), frames, stream_stride, frame_stride, None)

    for kw in ({"base": 1}, {"stream_stride": T * sc.FRAME + 2}, {"frame_stride": sc.FRAME + 1}, {"offs": None}, {"frames": -1}):
        assert dev(**kw) != 0, kw
    assert "16 bytes" in (dev(base=2) and hostsim_lib.error())
    assert L.nnn_sim_process_device(sim._h, _ffi.ptr(so), _ffi.ptr(no), None, T, None) != 0
    assert L.nnn_sim_debug_kernel(sim._h, _ffi.ptr(so), _ffi.ptr(no), 25, 1, None) != 0
    assert L.nnn_sim_debug_kernel(sim._h, _ffi.ptr(so), _ffi.ptr(no), 0, 1, None) != 0
    assert not buf.any() and not sim.fault()
    # after all of it the simulator is where it was: the first frames are the restatement's
    sc.assert_equal_bits(sim.signals(so, no), sc.restate(c.sig, c.noise, so, no, c.p1)[:5])
    assert dev(frames=0) == 0
    sim.close()


def test_debug_kernel_advances_only_the_simulator(hostsim_lib):
    """The measuring hook runs k_sim into the staging: the simulator's state moves as after a call, the rows' state does not."""
    from nnnoiseless_amd import _ffi
    c = sc.case(9, 26)
    sim, twin = c.simulator(hostsim_lib, c.p2), c.simulator(hostsim_lib, c.p2)
    so, no = c.sig_off[:4], c.noise_off[:4]
    sim.debug_kernel(_ffi.ptr(so[:2]), _ffi.ptr(no[:2]), 2, 1)
    twin.signals(so[:2], no[:2])
    sc.assert_equal_bits(sim.signals(so[2:], no[2:]), twin.signals(so[2:], no[2:]))
    sim.close(), twin.close()
