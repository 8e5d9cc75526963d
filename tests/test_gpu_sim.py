"""The noise simulator (include/nnn_sim.h) on the MI355X: the checks of tests/test_hostsim_sim.py that involve
k_sim, on the real kernel -- signals bit for bit against the NumPy restatement, rows bit for bit against the training-row call, the
oracle comparison, many tiles, and arenas, offsets and rows that are torch tensors.  (Offsets outside an arena are tested under the
interpreter only.)"""
import numpy as np
import pytest

import sim_cases as sc

pytestmark = pytest.mark.gpu


def test_signals_against_the_restatement(gpu_lib):
    sc.check_signals_against_restatement(gpu_lib)


def test_splitting_a_call(gpu_lib):
    sc.check_split_calls(gpu_lib)


@pytest.mark.parametrize("S, T", [(70, 7), (4096, 3)])
def test_rows_bit_for_bit(gpu_lib, S, T):
    """70 x 7: a partial tile; 4096 x 3: many tiles."""
    sc.check_rows_against_twin(gpu_lib, S, T)


def test_rows_across_groups(gpu_lib):
    """26 frames: the call's second group reads the staging the first one left."""
    sc.check_rows_against_twin(gpu_lib, 9, 26)


def test_rows_against_the_oracle(gpu_lib, oracle_mod, weights_bytes):
    """70 x 6 rows against the oracle on the restated signals, check_rows' absolute bars (sim_cases.check_rows_against_oracle)."""
    sc.check_rows_against_oracle(gpu_lib, oracle_mod, weights_bytes)


def test_adopt_device_with_torch_tensors(gpu_lib):
    """Arenas borrowed from torch tensors (one of them a view that begins at an odd element), offsets and rows torch tensors too, on
    torch's stream: the rows of the host call, the signals of the restatement."""
    import torch
    from nnnoiseless_amd import training
    c = sc.case(70, 7)
    dev = torch.device("cuda")
    sig = torch.from_numpy(np.concatenate([[123], c.sig]).astype(np.int16)).to(dev)[1:]
    noise = torch.from_numpy(c.noise).to(dev)
    assert sig.data_ptr() % 4 == 2
    want = c.simulator(gpu_lib, c.p2).process(c.sig_off, c.noise_off)
    sim = training.NoiseSimulator(training.TrainingFeatures(c.S, lib=gpu_lib))
    sim.adopt_device(training.ARENA_SIGNAL, sig.data_ptr(), sig.numel(), keep=sig)
    sim.adopt_device(training.ARENA_NOISE, noise.data_ptr(), noise.numel(), keep=noise)
    sim.set_params(None, c.p2)
    so = torch.from_numpy(c.sig_off.astype(np.int64)).to(dev)      # (offsets below 2^63: the same bits as uint64)
    no = torch.from_numpy(c.noise_off.astype(np.int64)).to(dev)
    rows = torch.zeros((c.T, c.S, 87), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    sim.process_device(so.data_ptr(), no.data_ptr(), rows.data_ptr(), c.T, stream)
    torch.cuda.synchronize()
    assert np.array_equal(sc.bits(rows.cpu().numpy()), sc.bits(want))
    assert not sim.fault()
    sim.reset()
    sc.assert_equal_bits(sim.signals(c.sig_off, c.noise_off), sc.restate(c.sig, c.noise, c.sig_off, c.noise_off, c.p2)[:5])
    sim.close()
