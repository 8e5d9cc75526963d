"""Channel-linked gains (include/nnn_batch.h "Channel link") on the MI355X: the assertions of test_hostsim_channel_link.py through the
product library -- every gains sink under every link and both NNN_RNN_ROWS -- and one shape of more than one round of blocks through the
device entry points on a torch stream: 4160 streams (65 tiles: eight-tile XCD dealing plus a tail tile) x 4 frames, test_gpu_split.py's
s4160: process_device under a link against analyze_device -> network_device -> the link formula in torch -> synthesize_device on the same
stream."""
import numpy as np
import pytest

import test_gpu_split as gs
import test_hostsim_channel_link as hl
from test_hostsim_split import _bits

pytestmark = pytest.mark.gpu
SINKS = list(hl.SINKS)


@pytest.fixture(scope="module")
def nn():
    import nnnoiseless_amd
    return nnnoiseless_amd


@pytest.mark.parametrize("link", hl.LINKS)
@pytest.mark.parametrize("sink", SINKS)
@pytest.mark.parametrize("rows", hl.ROWS)
@pytest.mark.parametrize("name", list(hl.SHAPES))
def test_linked_call_is_the_linked_triple(nn, gpu_lib, name, rows, sink, link):
    hl.check_equals_triple(nn, gpu_lib, name, rows, sink, link)


@pytest.mark.parametrize("link", hl.LINKS)
@pytest.mark.parametrize("sink", SINKS)
def test_silent_member(nn, gpu_lib, sink, link):
    hl.check_silent_member(nn, gpu_lib, 32 if sink == "plain" else 16, sink, link)


@pytest.mark.parametrize("link", hl.LINKS)
@pytest.mark.parametrize("sink,rows", hl.SINK_ROWS)
def test_held_member(nn, gpu_lib, sink, rows, link):
    hl.check_held(nn, gpu_lib, rows, sink, link)


@pytest.mark.parametrize("link", [(2, "max"), (4, "min")])
@pytest.mark.parametrize("sink,rows", hl.SINK_ROWS)
@pytest.mark.parametrize("name", list(hl.SHAPES))
def test_link_then_floor(nn, gpu_lib, name, sink, rows, link):
    hl.check_floors(nn, gpu_lib, name, rows, sink, link)


@pytest.mark.parametrize("sink", SINKS)
@pytest.mark.parametrize("name", list(hl.SHAPES))
def test_off_is_off(nn, gpu_lib, name, sink):
    hl.check_off_is_off(nn, gpu_lib, name, 32, sink)


@pytest.mark.parametrize("sink", SINKS)
@pytest.mark.parametrize("name", list(hl.SHAPES))
def test_changing_the_link_between_calls(nn, gpu_lib, name, sink):
    hl.check_change_between_calls(nn, gpu_lib, name, 32 if sink == "plain" else 16, sink)


@pytest.mark.parametrize("sink", SINKS)
def test_lifecycle(nn, gpu_lib, sink):
    hl.check_lifecycle(nn, gpu_lib, 32, sink)


@pytest.mark.parametrize("name", list(hl.SHAPES))
def test_other_calls_ignore_the_link(nn, gpu_lib, name):
    hl.check_other_calls(nn, gpu_lib, name, 16, "fused")


@pytest.mark.parametrize("sink", SINKS)
def test_pcm_boundary(nn, gpu_lib, sink):
    hl.check_pcm(nn, gpu_lib, 32, sink)


@pytest.mark.parametrize("sink", SINKS)
def test_host_chunks(nn, gpu_lib, sink):
    hl.check_host_chunks(nn, gpu_lib, 16, sink)


@pytest.mark.parametrize("sink", ["wf", "plain"])
def test_schedules(nn, gpu_lib, sink):
    hl.check_schedules(nn, gpu_lib, sink)


@pytest.mark.parametrize("sink", SINKS)
def test_grouped_models(nn, gpu_lib, weights_bytes, sink):
    hl.check_models(nn, gpu_lib, weights_bytes, 16 if sink == "plain" else 32, sink)


def test_refusals(nn, gpu_lib):
    hl.check_refusals(nn, gpu_lib, 32, "fused")


def test_node(nn, gpu_lib):
    hl.check_node(nn, gpu_lib)


def link_torch(torch, g, sil, channels, mode):
    """link_np on the device: gains [T, S, 22], silence [T, S]."""
    T, S = sil.shape
    mm = (sil == 0).reshape(T, S // channels, channels, 1)
    gg = g.reshape(T, S // channels, channels, 22)
    if mode == "max":
        r = torch.where(mm, gg, torch.full_like(gg, -float("inf"))).amax(dim=2, keepdim=True)
    else:
        r = torch.where(mm, gg, torch.full_like(gg, float("inf"))).amin(dim=2, keepdim=True)
    return torch.where(mm, r, gg).reshape(T, S, 22).contiguous()


@pytest.mark.parametrize("link", [(2, "max"), (4, "min")])
@pytest.mark.parametrize("sink", SINKS)
def test_block_dealing(nn, sink, link):
    """14. s4160 x 4 frames in one process_device call on a torch stream under a link, through each gains sink, against the triple on the
    same stream with the link formula in torch between network_device and synthesize_device: audio, VAD and sampled records, on the int32
    views; VAD is the unlinked batch's, the audio is not."""
    import torch
    from nnnoiseless_amd import _ffi
    x = torch.from_numpy(gs.make_input("s4160")).cuda()
    S, T = x.shape[:2]
    own = torch.cuda.Stream()
    st = own.cuda_stream
    mode, wf = hl.SINKS[sink]
    with hl.env("NNN_RNN_WF_MIN_G", wf):
        c, d, u = nn.BatchDenoiser(S), nn.BatchDenoiser(S), nn.BatchDenoiser(S)
    c.set_back_end(mode)
    c.set_channel_link(*link)
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
        gl = link_torch(torch, g, SIL, *link)
    d.synthesize_device(gl.data_ptr(), v.data_ptr(), yd.data_ptr(), T, _ffi.PCM_F32, 1, T * 480, 480, hip_stream=st)
    for b in (c, d, u):
        b.synchronize()
    torch.cuda.synchronize()
    assert not c.fault() and not d.fault()
    i32 = lambda t: t.view(torch.int32)
    assert torch.equal(i32(y), i32(yd)) and torch.equal(i32(vc), i32(v)) and torch.equal(i32(vc), i32(vu))
    assert not torch.equal(i32(y), i32(yu))
    q = gs.SHAPES["s4160"][5]
    sil = SIL[:, q].cpu().numpy().astype(bool)
    assert sil.any() and not sil[0] and not sil[-1]
    want = hl.link_np(g.cpu().numpy(), SIL.cpu().numpy(), *link)
    assert np.array_equal(_bits(gl.cpu().numpy()), _bits(want))                        # (torch's formula is numpy's)
    idx = list(range(0, S, 37)) + [q, q ^ 1, S - 1]
    assert np.array_equal(c.export_streams(idx), d.export_streams(idx))
    assert c.channel_link() == link
