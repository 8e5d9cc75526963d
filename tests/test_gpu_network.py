"""The network-only calls (include/nnn_batch.h "Network-only calls") on the MI355X: the assertions of test_hostsim_network.py through the
product library, and one shape of more than one round of blocks through the device entry points on torch's current stream -- 4160 streams
(65 tiles: eight-tile XCD dealing plus a tail tile) x 4 frames, test_gpu_split.py's s4160: the triple analyze_device -> network_device ->
synthesize_device against one-frame processing calls with the taps on, and the network alone in one call."""
import numpy as np
import pytest

import test_gpu_split as gs
import test_hostsim_network as hn
from test_hostsim_split import GRU, _bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nn():
    import nnnoiseless_amd
    return nnnoiseless_amd


@pytest.mark.parametrize("rows", hn.ROWS)
@pytest.mark.parametrize("name", list(hn.SHAPES))
def test_triple_is_the_ordinary_path(nn, gpu_lib, name, rows):
    hn.check_triple(nn, gpu_lib, name, rows)


@pytest.mark.parametrize("rows", hn.ROWS)
@pytest.mark.parametrize("name", list(hn.SHAPES))
def test_network_alone(nn, gpu_lib, name, rows):
    hn.check_alone(nn, gpu_lib, name, rows)


@pytest.mark.parametrize("rows", hn.ROWS)
@pytest.mark.parametrize("name", list(hn.SHAPES))
def test_silence_none(nn, gpu_lib, name, rows):
    hn.check_silence_none(nn, gpu_lib, name, rows)


@pytest.mark.parametrize("rows", hn.ROWS)
def test_held_streams(nn, gpu_lib, rows):
    hn.check_held(nn, gpu_lib, rows)


@pytest.mark.parametrize("rows", hn.ROWS)
def test_alternation(nn, gpu_lib, rows):
    hn.check_alternation(nn, gpu_lib, rows)


@pytest.mark.parametrize("rows", hn.ROWS)
def test_models(nn, gpu_lib, oracle_mod, weights_bytes, rows):
    hn.check_models(nn, gpu_lib, oracle_mod, weights_bytes, rows)


@pytest.mark.parametrize("rows", hn.ROWS)
def test_refusals_and_protocol(nn, gpu_lib, rows):
    hn.check_refusals(nn, gpu_lib, rows)


_BIG = {}


def big_runs(nn, torch):
    """(x, A, G, V) of s4160, made once: A = one-frame process_device calls with the taps on (test_gpu_split.run_ordinary)."""
    if not _BIG:
        x = torch.from_numpy(gs.make_input("s4160")).cuda()
        a = gs.run_ordinary(nn, torch, x, gs.SHAPES["s4160"][3])
        _BIG["r"] = (x, a, torch.from_numpy(a["g_raw"]).cuda(), torch.from_numpy(np.ascontiguousarray(a["vad"][:, :, 0])).cuda())
    return _BIG["r"]


@pytest.mark.parametrize("rows", hn.ROWS)
def test_block_dealing(nn, rows):
    import torch
    from nnnoiseless_amd import _ffi
    x, a, G, V = big_runs(nn, torch)
    S, T = x.shape[:2]
    own = torch.cuda.Stream()                # one stream of the caller's for both batches: c's call reads the rows b's analyze writes
    st = own.cuda_stream
    with hn.rnn_rows(rows):
        b, c = nn.BatchDenoiser(S), nn.BatchDenoiser(S)
    F, SIL = torch.zeros((T, S, 42), device="cuda"), torch.zeros((T, S), dtype=torch.int32, device="cuda")
    g, v, y = torch.full((T, S, 22), gs.SENT, device="cuda"), torch.full((T, S), gs.SENT, device="cuda"), torch.zeros_like(x)
    g2, v2 = torch.full_like(g, gs.SENT), torch.full_like(v, gs.SENT)
    torch.cuda.synchronize()
    # the triple, device rows resident between the three calls
    b.analyze_device(x.data_ptr(), F.data_ptr(), SIL.data_ptr(), T, _ffi.PCM_F32, 1, T * 480, 480, st)
    b.network_device(F.data_ptr(), SIL.data_ptr(), g.data_ptr(), v.data_ptr(), T, st)
    assert b.pending_frames() == T
    b.synthesize_device(g.data_ptr(), v.data_ptr(), y.data_ptr(), T, _ffi.PCM_F32, 1, T * 480, 480, hip_stream=st)
    # the network alone on a fresh batch: one call, in stream order behind b's analyze
    c.network_device(F.data_ptr(), SIL.data_ptr(), g2.data_ptr(), v2.data_ptr(), T, st)
    b.synchronize(), c.synchronize()
    torch.cuda.synchronize()
    assert not b.fault() and not c.fault()
    for got_g, got_v in ((g, v), (g2, v2)):
        assert torch.equal(got_g.view(torch.int32), G.view(torch.int32)) and torch.equal(got_v.view(torch.int32), V.view(torch.int32))
    sil = a["silence"][:, gs.SHAPES["s4160"][5], 0].astype(bool)
    assert sil.any() and not sil[0] and not sil[-1]
    assert not _bits(g[torch.from_numpy(sil).cuda(), gs.SHAPES["s4160"][5]].cpu().numpy()).any()
    assert torch.equal(y, a["out"])
    idx = list(range(0, S, 37)) + [S - 1]
    ra, rb, rc = a["records"][idx], b.export_streams(idx), c.export_streams(idx)
    assert np.array_equal(rb, ra)
    blank = nn.BatchDenoiser(64).export_streams([0])[0]
    for k in _ffi.STREAM_STATE_FIELDS:
        fc = _ffi.stream_state_field(rc, k)
        want = _ffi.stream_state_field(ra, k) if k in GRU else np.broadcast_to(_ffi.stream_state_field(blank, k), fc.shape)
        assert np.array_equal(_bits(fc), _bits(want)), k
