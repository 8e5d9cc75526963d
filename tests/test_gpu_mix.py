"""The conference mixer (include/nnn_mix.h) on the MI355X: the checks of tests/test_hostsim_mix.py on the real
kernels, many blocks, torch tensors on a stream of torch's, and one server tick -- BatchDenoiser, VadGate, ConferenceMixer -- on the
golden recording against the restatements chained.  All bit for bit."""
import numpy as np
import pytest

import gate_cases as gc
import mix_cases as mc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mem():
    return mc.TorchMem()


@pytest.mark.parametrize("S, T", mc.SHAPES)
def test_against_the_restatement(gpu_lib, mem, S, T):
    mc.check_restatement(gpu_lib, mem, S, T)


def test_many_blocks(gpu_lib, mem):
    """4096 x 3 in rooms of 1, 2, 3, 5, 9 and 40 members spread over the streams: some thousand blocks of k_mix_sum, sixteen of k_mix_carry."""
    S, T = 4096, 3
    room, gain = mc.rooms_for(S), mc.gains_for(S)
    sizes = {len(g) for g in mc.groups(room)}
    assert {1, 2, 3, 5, 9, 40} <= sizes
    m, rs = mc.mixer(gpu_lib, S, room, gain), mc.Restated(S, room, gain)
    for call in range(2):
        x, talk = mc.audio(40 + call, S, T), (np.random.default_rng(call).random((T, S)) < 0.4).astype(np.uint8)
        y, h = mc.device_call(m, mem, x, talk, lin={"layout": "frames"})
        wy, wh = rs.apply(x, talk)
        mc.assert_same(y, wy, f"call {call} audio"), mc.assert_same(h, wh, f"call {call} heard")
    assert {0, 1, 2, 3} <= rs.counts and max(rs.counts) > mc.REG
    m.close()


def test_chunking(gpu_lib, mem):
    mc.check_chunking(gpu_lib, mem)


def test_layout_and_formats(gpu_lib, mem):
    mc.check_layout(gpu_lib, mem)


def test_live_mask(gpu_lib, mem):
    mc.check_live(gpu_lib, mem)


def test_inaudible_inputs_do_not_leak(gpu_lib, mem):
    mc.check_inaudible_nan(gpu_lib, mem)


def test_consequences_of_the_rule(gpu_lib, mem):
    mc.check_consequences(gpu_lib, mem)


def test_non_finite_audible_samples(gpu_lib, mem):
    mc.check_nonfinite(gpu_lib, mem)


def test_bits_do_not_depend_on_n_streams(gpu_lib, mem):
    mc.check_n_streams(gpu_lib, mem)


def test_reset_and_setters(gpu_lib, mem):
    mc.check_state(gpu_lib, mem)


def test_host_call(gpu_lib, mem):
    mc.check_host_call(gpu_lib, mem)


def test_refusals(gpu_lib, mem):
    mc.check_refusals(gpu_lib, mem)


def test_torch_tensors_on_torchs_stream(gpu_lib):
    """Audio, talk and live are torch tensors made by kernels on a stream of torch's; ConferenceMixer.apply enqueues behind them on that
    stream, reading a permuted view of the batch's [T][S][480] that starts at an odd float and writing a tensor of other strides, and
    torch goes on working with the result on the same stream."""
    import torch
    S, T = 45, 5
    room, gain = mc.rooms_for(S), mc.gains_for(S, 2)
    x, talk = mc.audio(61, S, T), mc.talk_rows(62, room, T)
    live = (np.arange(S) % 5 != 2).astype(np.uint8)
    m, rs = mc.mixer(gpu_lib, S, room, gain), mc.Restated(S, room, gain)
    dev = torch.device("cuda")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        flat = torch.cat([torch.zeros(1, device=dev), torch.from_numpy(x).to(dev).permute(1, 0, 2).reshape(-1)])[1:]
        a = flat.view(T, S, mc.FRAME).permute(1, 0, 2)                 # [S][T][480] over [T][S][480]
        tk = torch.from_numpy(talk).to(dev) * 1
        tl = torch.from_numpy(live).to(dev)
        assert a.data_ptr() % 16 == 4
        out = torch.full((S, T, mc.FRAME), float(mc.SENT), device=dev)
        res, hd = m.apply(a, talk=tk, live=tl, out=out, want_heard=True)
        assert res is out
        total = out[torch.from_numpy(live != 0).to(dev)].abs().sum()   # (torch goes on with the result on its stream)
    st.synchronize()
    wy, wh = rs.apply(x, talk, live=live)
    wh[:, live == 0] = 0                                               # (the mirror hands back zeros where nothing was written)
    mc.assert_same(out.cpu().numpy(), wy), mc.assert_same(hd.cpu().numpy(), wh)
    assert np.isclose(float(total), np.abs(wy[live != 0].astype(np.float64)).sum(), rtol=1e-5)
    # the default stream (handle 0 would mean "the object's own stream"): a side stream of torch's carries the call
    handles, device_call = [], m.apply_device
    m.apply_device = lambda *args, **kw: (handles.append(kw["hip_stream"]), device_call(*args, **kw))[1]
    x2 = torch.from_numpy(x).to(dev)
    out2 = m.apply(x2 * 1.0, talk=torch.from_numpy(talk).to(dev))
    got2 = out2.clone()
    torch.cuda.synchronize()
    assert len(handles) == 1 and handles[0] not in (0, None)
    mc.assert_same(got2.cpu().numpy(), rs.apply(x, talk)[0], "on the default stream")
    m.close()


def test_server_tick_end_to_end(gpu_lib, golden_io):
    """One tick on one stream of work, 16 streams x 6 frames derived from the golden recording: BatchDenoiser.process, VadGate.apply in
    place with its open flags, ConferenceMixer.apply(talk = open, live = !held), streams 3 and 9 held -- against the gate's restatement
    applied to the batch's own output and the mixer's restatement applied to that."""
    import nnnoiseless_amd as nn
    from nnnoiseless_amd.gate import VadGate
    from nnnoiseless_amd.mix import ConferenceMixer
    S, T = 16, 6
    inp, _ = golden_io
    x = np.stack([inp[40 + 3 * s:40 + 3 * s + 2 * T] for s in range(S)]).astype(np.float32)      # [S, 12, 480]: a warm-up call and the tick
    held = [3, 9]
    room = np.array([5, 5, 5, 2, 2, 5, 5, -1, 5, 5, 5, 5, 2, 5, 0, 0], np.int32)
    b = nn.BatchDenoiser(S, lib=gpu_lib)
    den0, vad0 = b.process(x[:, :T])
    b.hold_streams(held)
    den = np.full_like(x[:, T:], mc.SENT)
    vad = np.full((T, S), -1.0, np.float32)
    b.process(x[:, T:], out=den, vad=vad)
    live = (~b.held()).astype(np.uint8)
    b.close()
    thr = ((vad0.min(axis=0) + vad0.max(axis=0)) * np.float32(0.5)).astype(np.float32)      # halfway: every gate opens, most close too
    par = {"threshold": thr, "grace": np.arange(S) % 2, "lookback": np.zeros(S, np.int64), "level": np.zeros(S, np.float32)}
    assert live.tolist() == [0 if s in held else 1 for s in range(S)]
    g, m = VadGate(S, 0, lib=gpu_lib), ConferenceMixer(S, lib=gpu_lib)
    g.set_params(par["threshold"], par["grace"], par["lookback"], par["level"])
    m.set_rooms(room)
    rg, rm = gc.Restated(S, 0, par), mc.Restated(S, room)
    outs = []
    for call, (d, v, lv) in enumerate(((den0, vad0, None), (den, vad, live))):
        gated = d.copy()
        _, opn = g.apply(gated, v, live=lv, out=gated, want_open=True)                           # in place, as the server does
        mixed, heard = m.apply(gated, talk=opn, live=lv, out=np.full_like(gated, mc.SENT), want_heard=True)
        wg, wo = rg.apply(d, v, live=lv, base=d)
        if lv is not None:
            wo[:, lv == 0] = 0
        mc.assert_same(gated, wg, f"call {call} gate"), mc.assert_same(opn, wo, f"call {call} open")
        wy, wh = rm.apply(wg, wo, live=lv)
        if lv is not None:
            wh[:, lv == 0] = 0
        mc.assert_same(mixed, wy, f"call {call} mix"), mc.assert_same(heard, wh, f"call {call} heard")
        outs.append((mixed, wo, wh))
    assert (outs[1][0][held] == mc.SENT).all()
    opens = np.concatenate([outs[0][1], outs[1][1][:, live == 1]], axis=1)
    assert (opens == 1).any() and (opens == 0).any(), "the gates open and close"
    assert max(rm.counts) >= 3 and (outs[0][0] != 0).any()
    g.close(), m.close()
