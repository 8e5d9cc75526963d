"""The VAD-only calls (include/nnn_batch.h "VAD-only calls") on the MI355X: the assertions of test_hostsim_vad.py through the product
library, and two shapes that exercise k_vad's dealing of blocks to tiles through the device entry points on torch's current stream --
576 streams (nine tiles: not a multiple of eight) x 24 frames and 4096 x 24, one VAD call of 24 frames each against the VAD rows of an
ordinary 24-frame processing call (the ordinary path's kernels give the same bits whatever the call length)."""
import numpy as np
import pytest

import test_hostsim_vad as hv
from test_hostsim_split import quiet_stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nn():
    import nnnoiseless_amd
    return nnnoiseless_amd


@pytest.mark.parametrize("name", list(hv.SHAPES))
def test_same_bits_as_the_ordinary_path(nn, gpu_lib, oracle_mod, weights_bytes, name):
    hv.check_same_bits(nn, gpu_lib, oracle_mod, weights_bytes, name)


@pytest.mark.parametrize("name", list(hv.SHAPES))
def test_records(nn, gpu_lib, name):
    hv.check_records(nn, gpu_lib, name)


def test_alternating_modes(nn, gpu_lib):
    hv.check_alternation(nn, gpu_lib)


def test_held_streams(nn, gpu_lib):
    hv.check_held(nn, gpu_lib)


def test_formats(nn, gpu_lib):
    hv.check_formats(nn, gpu_lib)


def test_models(nn, gpu_lib, oracle_mod, weights_bytes):
    hv.check_models(nn, gpu_lib, oracle_mod, weights_bytes)


def test_refusals(nn, gpu_lib):
    hv.check_refusals(nn, gpu_lib)


def test_fft_feat_against_fft_xp(nn, gpu_lib):
    hv.check_fft_feat(nn, gpu_lib)


_X576 = {}


def big_input(S, T=24):
    """make_streams_fast for 576 streams with a quiet stream; larger batches repeat it at other levels (repeat r scaled by 1 + r / 16,
    so that tiles eight or nine apart do not hold the same samples)."""
    from nnnoiseless_amd.synthetic import make_streams_fast
    if T not in _X576:
        x = make_streams_fast(576, T, seed=23)
        x[7] = quiet_stream(T, (9, 14))
        _X576[T] = x
    base = _X576[T]
    reps = (S + 575) // 576
    return np.concatenate([base * np.float32(1.0 + r / 16.0) for r in range(reps)])[:S]


@pytest.mark.parametrize("S", [576, 4096])
def test_block_dealing(nn, S):
    import torch
    from nnnoiseless_amd import _ffi
    T = 24
    x = torch.from_numpy(big_input(S, T)).cuda()
    y, want, got = torch.zeros_like(x), torch.zeros((T, S), device="cuda"), torch.full((T, S), -12345.0, device="cuda")
    a, b = nn.BatchDenoiser(S), nn.BatchDenoiser(S)
    torch.cuda.synchronize()
    st = torch.cuda.current_stream().cuda_stream
    a.process_device(x.data_ptr(), y.data_ptr(), want.data_ptr(), T, T * 480, 480, st)
    b.vad_device(x.data_ptr(), got.data_ptr(), T, _ffi.PCM_F32, 1, T * 480, 480, st)
    a.synchronize(), b.synchronize()
    torch.cuda.synchronize()
    assert not a.fault() and not b.fault()
    assert torch.equal(want.view(torch.int32), got.view(torch.int32))
    sil = want[:, 7] == 0
    assert bool(sil.any()) and not bool(sil[0]) and not bool(sil[-1])
    idx = list(range(0, S, 37))
    ra, rb = a.export_streams(idx), b.export_streams(idx)
    for k in hv.ADVANCED:
        assert np.array_equal(hv._bits(_ffi.stream_state_field(rb, k)), hv._bits(_ffi.stream_state_field(ra, k))), k
    for k in hv.UNTOUCHED:
        assert not _ffi.stream_state_field(rb, k).any(), k
