"""The network trainer (include/nnn_fit.h) on the MI355X: the checks of tests/test_hostsim_fit.py on the real
kernels, many blocks, and rows that are torch tensors on torch's stream."""
import numpy as np
import pytest

import fit_cases as fc

pytestmark = pytest.mark.gpu
TILE = 4


@pytest.mark.parametrize("S, T", [(3, 5), (TILE + 1, 3), (5, 40), (2, 1), (70, 64)])
def test_against_float64(gpu_lib, S, T):
    """The interpreter's cases, and (70, 64): many blocks of every kernel."""
    fc.check_case(gpu_lib, S, T)


@pytest.mark.parametrize("kind", ["builtin", "sh"])
def test_templates_against_float64(gpu_lib, kind):
    fc.check_case(gpu_lib, 3, 8, kind)


def test_independence(gpu_lib):
    fc.check_independence(gpu_lib)


def test_optimizer_bit_for_bit(gpu_lib):
    fc.check_optimizer(gpu_lib)


def test_export(gpu_lib):
    fc.check_export(gpu_lib)


def test_end_to_end(gpu_lib):
    fc.check_end_to_end(gpu_lib)


def test_refusals(gpu_lib):
    fc.check_refusals(gpu_lib)


def test_torch_tensors_on_torchs_stream(gpu_lib):
    """Rows, weights and outputs as torch tensors, calls enqueued on torch's stream: the bits of the host calls."""
    import torch
    c = fc.case(5, 40)
    tr = fc.trainer_for(gpu_lib, c)
    want_g, want_v = tr.forward(c.rows)
    want_l = tr.grad(c.rows, c.w)
    want_grad = tr.gradient()
    dev = torch.device("cuda")
    rows, w = torch.from_numpy(c.rows).to(dev), torch.from_numpy(c.w).to(dev)
    gains, vad = torch.zeros((c.T, c.S, 22), device=dev), torch.zeros((c.T, c.S), device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    tr.forward_device(rows.data_ptr(), c.S, c.T, gains.data_ptr(), vad.data_ptr(), hip_stream=stream)
    tr.grad_device(rows.data_ptr(), c.S, c.T, w.data_ptr(), hip_stream=stream)
    torch.cuda.synchronize()
    assert np.array_equal(fc.bits(gains.cpu().numpy()), fc.bits(want_g)) and np.array_equal(fc.bits(vad.cpu().numpy()), fc.bits(want_v))
    assert tr.losses() == want_l and np.array_equal(fc.bits(tr.gradient()), fc.bits(want_grad))
    tr.close()
