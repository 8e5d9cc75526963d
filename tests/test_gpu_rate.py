"""The rate adapter (include/nnn_rate.h) on the GPU library: the cases of test_hostsim_rate.py at 70 streams (one
full 64-stream tile and a part tile; three stream groups of k_rate_in / k_rate_out, the last one short) and about 12 frames.  Bit for
bit, because the yardstick's middle piece is the same library's own BatchDenoiser.process (tests/rate_cases.py)."""
import pytest

import rate_cases as rc

S = 70
RATES = [16000.0, 44100.0]


def _n(rate, frames=12):
    return int(rate * frames / 100) + 7


@pytest.mark.gpu
@pytest.mark.parametrize("rate", RATES)
def test_composition_bit_for_bit_gpu(gpu_lib, oracle_mod, rate):
    r, _, _ = rc.check_composition(gpu_lib, oracle_mod, S, _n(rate), rate, (1, 7, 0, 250))
    assert r["n_frames"][0] == 0 and r["n_frames"][2] == 0 and r["n_out"][2] == 0
    assert sum(r["n_frames"]) == 12


@pytest.mark.gpu
def test_long_call_gpu(gpu_lib, oracle_mod):
    """40 frames in one call: the batch pipelines calls of 32 frames or more over its internal streams, in place in the adapter's
    staging, between the two legs."""
    r, _, _ = rc.check_composition(gpu_lib, oracle_mod, S, _n(16000.0, 40), 16000.0, ())
    assert r["n_frames"] == [40]


@pytest.mark.gpu
@pytest.mark.parametrize("rate", RATES)
def test_int16_is_the_f32_path_rounded_gpu(gpu_lib, rate):
    rc.check_int16(gpu_lib, S, _n(rate), rate, (1, 7, 250))


@pytest.mark.gpu
def test_reset_streams_gpu(gpu_lib, oracle_mod):
    rc.check_reset(gpu_lib, oracle_mod, S, 12, 5, stream=65)


@pytest.mark.gpu
@pytest.mark.parametrize("rate,tick", [(16000.0, 160), (44100.0, 441)])
def test_hold_and_resume_gpu(gpu_lib, oracle_mod, rate, tick):
    rc.check_hold(gpu_lib, oracle_mod, S, 12, 4, stream=33, rate=rate, tick=tick)
