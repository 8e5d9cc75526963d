"""The scorer (include/nnn_score.h) on the MI355X: the checks of tests/test_hostsim_score.py on the real kernels,
with the signals, the mask and the frame sums as torch tensors on a stream of torch's -- bit for bit against the NumPy restatement --,
many blocks, and evaluate end to end against restatements over what the host calls return."""
import numpy as np
import pytest

import score_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mem():
    return sc.TorchMem()


@pytest.mark.parametrize("S, T", sc.SHAPES + [(6, 11), (4096, 3)])
def test_against_the_restatement(gpu_lib, mem, S, T):
    """The interpreter's shapes, 6 x 11 (three runs of frames per stream, the last one short) and 4096 x 3: many blocks."""
    sc.check_restatement(gpu_lib, mem, S, T)


def test_chunking(gpu_lib, mem):
    sc.check_chunking(gpu_lib, mem)


def test_layout_and_alignment(gpu_lib, mem):
    sc.check_layout(gpu_lib, mem)


def test_valid_mask(gpu_lib, mem):
    sc.check_valid(gpu_lib, mem)


def test_exact_identities(gpu_lib, mem):
    sc.check_identities(gpu_lib, mem)


def test_range_and_non_finite(gpu_lib, mem):
    sc.check_range(gpu_lib, mem)


def test_reset_and_set_delay(gpu_lib, mem):
    sc.check_reset(gpu_lib, mem)


def test_the_same_call_twice(gpu_lib, mem):
    sc.check_twice(gpu_lib, mem)


def test_host_call(gpu_lib, mem):
    sc.check_host_call(gpu_lib, mem)


def test_torch_tensors_on_torchs_stream(gpu_lib):
    """ref, test, valid and frame_sums are torch tensors, the call is enqueued on torch's current stream behind the kernels that made
    them, and the test signal is a view that starts at an odd element of its tensor."""
    import torch
    S, T = 70, 5
    d = sc.mixed_delays(S)
    r, y = sc.signals(61, S, T)
    valid = (np.arange(T * S).reshape(T, S) % 5 != 2).astype(np.uint8)
    dev = torch.device("cuda")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        tr = torch.from_numpy(r).to(dev).permute(1, 0, 2).contiguous()               # [T][S][480]
        ty = torch.cat([torch.zeros(1, device=dev), torch.from_numpy(y).to(dev).permute(1, 0, 2).reshape(-1)])[1:]
        tv = torch.from_numpy(valid).to(dev)
        fs = torch.full((T, S, 4), 5.0, dtype=torch.float64, device=dev)
        assert ty.data_ptr() % 16 == 4 and tr.data_ptr() % 16 == 0
        s = sc.scorer(gpu_lib, S, d)
        s.accumulate_device(tr.data_ptr(), ty.data_ptr(), T, sc.FRAME, S * sc.FRAME, d_valid=tv.data_ptr(), d_frame_sums=fs.data_ptr(),
                            hip_stream=torch.cuda.current_stream().cuda_stream)
        tot = torch.zeros((S, 4), dtype=torch.float64, device=dev)
        s.totals_device(tot.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
        seg = fs[..., 0].sum()                                                       # (torch goes on working with the table on its stream)
    st.synchronize()
    rs = sc.Restated(S, 960, d)
    want = rs.accumulate(r, y, valid)
    sc.assert_same(fs.cpu().numpy(), want)
    sc.assert_same(tot.cpu().numpy(), rs.tot)
    sc.assert_totals(s, rs)
    assert np.isclose(float(seg), want[..., 0].sum(), rtol=1e-12)
    s.close()


def test_evaluate_end_to_end(gpu_lib):
    """evaluate at 8 streams x 30 frames on synthetic clips with the built-in model: scorer A's totals equal the restatement over the
    simulator's own signals, scorer B's the restatement over the output that process returns to the host, bit for bit.  The improvement
    in dB is a measurement, not a bar: it is printed (DESIGN.md section 23 records it)."""
    import nnnoiseless_amd as nn
    from nnnoiseless_amd import score, training
    from nnnoiseless_amd.synthetic import make_streams
    S, T = 8, 30
    x = make_streams(0, 12, 20)                                    # twelve clips of 20 frames: tones in noise, one silent, one noise alone
    clean = [np.clip(np.round(c.reshape(-1)), -32768, 32767).astype(np.int16) for c in x[:6]]
    noise = [np.clip(np.round(0.3 * c.reshape(-1)), -32768, 32767).astype(np.int16) for c in x[6:]]
    res = score.evaluate(None, clean, noise, S * T, S, seed=5, lib=gpu_lib)
    sig, nz, so, no, params = score.evaluation_plan(clean, noise, S * T, S, 5)
    assert so.shape == (T, S)
    features = training.TrainingFeatures(S, lib=gpu_lib)
    sim = training.NoiseSimulator(features)
    sim.load_signal(sig), sim.load_noise(nz), sim.set_params(None, params)
    c, _, mix, _, _ = sim.signals(so, no)
    out, _ = nn.BatchDenoiser(S, lib=gpu_lib).process(mix)
    a, b = sc.Restated(S, 0), sc.Restated(S, 480, np.full(S, 480))
    a.accumulate(c, mix), b.accumulate(c, out)
    sc.assert_same(res["mix"], a.tot, "scorer A")
    sc.assert_same(res["out"], b.tot, "scorer B")
    assert np.array_equal(res["frames"], np.full(S, T, np.uint64))
    assert (a.tot[:, 0] > 0).any() and np.isfinite(b.tot).all()
    al = res["all"]
    print(f"evaluate, {S} streams x {T} frames, built-in model, synthetic clips: SNR {al['snr_mix_db']:.3f} -> {al['snr_out_db']:.3f} dB "
          f"({al['snr_gain_db']:+.3f}), SI-SDR {al['si_sdr_mix_db']:.3f} -> {al['si_sdr_out_db']:.3f} dB ({al['si_sdr_gain_db']:+.3f})")
    sim.close(), features.close()
