"""Per-stream gain floors (include/nnn_batch.h "Gain floors") on the MI355X: the assertions of test_hostsim_gain_floor.py through the
product library, and one shape of more than one round of blocks through the device entry points on a torch stream -- 4160 streams
(65 tiles: eight-tile XCD dealing plus a tail tile) x 4 frames, test_gpu_split.py's s4160: process_device under P against
analyze_device -> network_device -> torch.maximum -> synthesize_device on the same stream."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_split as gs
import test_hostsim_gain_floor as hf
from test_hostsim_split import _bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nn():
    import nnnoiseless_amd
    return nnnoiseless_amd


@pytest.mark.parametrize("sink", list(hf.SINKS))
@pytest.mark.parametrize("rows", hf.ROWS)
@pytest.mark.parametrize("name", list(hf.SHAPES))
def test_floored_call_is_the_clamped_triple(nn, gpu_lib, name, rows, sink):
    hf.check_equals_triple(nn, gpu_lib, name, rows, sink)


@pytest.mark.parametrize("sink", list(hf.SINKS))
def test_one_call_of_all_frames(nn, gpu_lib, sink):
    hf.check_one_call(nn, gpu_lib, 32, sink)


@pytest.mark.parametrize("sink", list(hf.SINKS))
@pytest.mark.parametrize("name", list(hf.SHAPES))
def test_floor_one_is_unit_gains(nn, gpu_lib, name, sink):
    hf.check_all_ones(nn, gpu_lib, name, 16 if sink == "plain" else 32, sink)


@pytest.mark.parametrize("sink", list(hf.SINKS))
@pytest.mark.parametrize("name", list(hf.SHAPES))
def test_off_is_off(nn, gpu_lib, name, sink):
    hf.check_off_is_off(nn, gpu_lib, name, 32, sink)


@pytest.mark.parametrize("sink", list(hf.SINKS))
@pytest.mark.parametrize("name", list(hf.SHAPES))
def test_changing_floors_between_calls(nn, gpu_lib, name, sink):
    hf.check_change_between_calls(nn, gpu_lib, name, 32 if sink == "plain" else 16, sink)


@pytest.mark.parametrize("sink", list(hf.SINKS))
def test_lifecycle(nn, gpu_lib, sink):
    hf.check_lifecycle(nn, gpu_lib, 32, sink)


@pytest.mark.parametrize("name", list(hf.SHAPES))
def test_other_calls_ignore_floors(nn, gpu_lib, name):
    hf.check_other_calls(nn, gpu_lib, name, 16, "fused")


@pytest.mark.parametrize("sink", list(hf.SINKS))
def test_pcm_boundary(nn, gpu_lib, sink):
    hf.check_pcm(nn, gpu_lib, 32, sink)


@pytest.mark.parametrize("sink", list(hf.SINKS))
def test_host_chunks(nn, gpu_lib, sink):
    hf.check_host_chunks(nn, gpu_lib, 16, sink)


@pytest.mark.parametrize("sink", list(hf.SINKS))
def test_grouped_models(nn, gpu_lib, weights_bytes, sink):
    hf.check_models(nn, gpu_lib, weights_bytes, 16 if sink == "plain" else 32, sink)


def test_refusals(nn, gpu_lib):
    hf.check_refusals(nn, gpu_lib, 32, "fused")


def test_node(nn, gpu_lib):
    hf.check_node(nn, gpu_lib)


@pytest.mark.parametrize("sink", list(hf.SINKS))
def test_block_dealing(nn, sink):
    """10. s4160 x 4 frames in one process_device call on a torch stream under P, through each gains sink, against the triple on the same
    stream with torch.maximum between network_device and synthesize_device: audio, VAD and sampled records, on the int32 views."""
    import torch
    from nnnoiseless_amd import _ffi
    x = torch.from_numpy(gs.make_input("s4160")).cuda()
    S, T = x.shape[:2]
    P = torch.from_numpy(hf.pattern(S)).cuda()
    own = torch.cuda.Stream()
    st = own.cuda_stream
    mode, wf = hf.SINKS[sink]
    with hf.env("NNN_RNN_WF_MIN_G", wf):
        c, d, u = nn.BatchDenoiser(S), nn.BatchDenoiser(S), nn.BatchDenoiser(S)
    c.set_back_end(mode)
    hf.set_pattern(c, S)
    F, SIL = torch.zeros((T, S, 42), device="cuda"), torch.zeros((T, S), dtype=torch.int32, device="cuda")
    g, v = torch.full((T, S, 22), gs.SENT, device="cuda"), torch.full((T, S), gs.SENT, device="cuda")
    y, yd, yu = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x)
    vc, vu = torch.full_like(v, gs.SENT), torch.full_like(v, gs.SENT)
    torch.cuda.synchronize()
    c.process_device(x.data_ptr(), y.data_ptr(), vc.data_ptr(), T, T * 480, 480, st)
    u.process_device(x.data_ptr(), yu.data_ptr(), vu.data_ptr(), T, T * 480, 480, st)
    d.analyze_device(x.data_ptr(), F.data_ptr(), SIL.data_ptr(), T, _ffi.PCM_F32, 1, T * 480, 480, st)
    d.network_device(F.data_ptr(), SIL.data_ptr(), g.data_ptr(), v.data_ptr(), T, st)
    with torch.cuda.stream(own):
        gf = torch.maximum(g, P)
    d.synthesize_device(gf.data_ptr(), v.data_ptr(), yd.data_ptr(), T, _ffi.PCM_F32, 1, T * 480, 480, hip_stream=st)
    for b in (c, d, u):
        b.synchronize()
    torch.cuda.synchronize()
    assert not c.fault() and not d.fault()
    i32 = lambda t: t.view(torch.int32)
    assert torch.equal(i32(y), i32(yd)) and torch.equal(i32(vc), i32(v)) and torch.equal(i32(vc), i32(vu))
    assert torch.equal(i32(y[0::4]), i32(yu[0::4])) and not torch.equal(i32(y[1::4]), i32(yu[1::4]))
    q = gs.SHAPES["s4160"][5]
    sil = SIL[:, q].cpu().numpy().astype(bool)
    assert sil.any() and not sil[0] and not sil[-1]
    idx = list(range(0, S, 37)) + [q, S - 1]
    assert np.array_equal(c.export_streams(idx), d.export_streams(idx))
    assert np.array_equal(_bits(c.gain_floor(idx)), _bits(hf.pattern(S)[idx]))


@pytest.mark.parametrize("sink", ["wf", "plain"])
def test_pipelined_call(nn, sink):
    """1c. A pipelined call under P: 70 streams x 40 frames in ONE process_device call (two groups of 20 spread over the batch's internal
    streams, nnn_batch_debug_schedule says so), floors set just before it on the batch's own stream, against the triple in pairs of 24 and
    16 frames: audio, VAD and records."""
    import torch
    from nnnoiseless_amd import _ffi
    from nnnoiseless_amd.synthetic import make_streams
    S, T = 70, 40
    x = torch.from_numpy(np.clip(np.round(make_streams(43, S, T)), -32768, 32767).astype(np.float32)).cuda()
    P = torch.from_numpy(hf.pattern(S)).cuda()
    own = torch.cuda.Stream()
    st = own.cuda_stream
    with hf.env("NNN_RNN_WF_MIN_G", hf.SINKS[sink][1]):
        c, d = nn.BatchDenoiser(S), nn.BatchDenoiser(S)
    sched = np.zeros(4096, np.int32)
    c._lib.check(c._lib.L.nnn_batch_debug_schedule(c._h, T, sched.ctypes.data_as(C.POINTER(C.c_int32)), sched.size))
    assert sched[1] == 2 and sched[2] == 1                                             # two groups, pipelined
    hf.set_pattern(c, S)
    y, yd = torch.zeros_like(x), torch.zeros_like(x)
    vc, vd = torch.zeros((T, S), device="cuda"), torch.zeros((T, S), device="cuda")
    F, SIL = torch.zeros((T, S, 42), device="cuda"), torch.zeros((T, S), dtype=torch.int32, device="cuda")
    g = torch.zeros((T, S, 22), device="cuda")
    torch.cuda.synchronize()
    c.process_device(x.data_ptr(), y.data_ptr(), vc.data_ptr(), T, T * 480, 480, st)
    pos = 0
    for n in (24, 16):
        o = lambda t, per: t.data_ptr() + pos * per * 4
        d.analyze_device(o(x, 480), o(F, S * 42), o(SIL, S), n, _ffi.PCM_F32, 1, T * 480, 480, st)
        d.network_device(o(F, S * 42), o(SIL, S), o(g, S * 22), o(vd, S), n, st)
        with torch.cuda.stream(own):
            g[pos:pos + n] = torch.maximum(g[pos:pos + n], P)
        d.synthesize_device(o(g, S * 22), o(vd, S), o(yd, 480), n, _ffi.PCM_F32, 1, T * 480, 480, hip_stream=st)
        pos += n
    c.synchronize(), d.synchronize()
    torch.cuda.synchronize()
    assert not c.fault() and not d.fault()
    i32 = lambda t: t.view(torch.int32)
    assert torch.equal(i32(y), i32(yd)) and torch.equal(i32(vc), i32(vd))
    assert np.array_equal(c.export_streams(range(S)), d.export_streams(range(S)))
    assert (torch.minimum(g, P) == P).all()
