"""The talker picker (include/nnn_pick.h) on the MI355X: the checks of tests/test_hostsim_pick.py on the real
kernels, many blocks, torch tensors on a stream of torch's, and one server tick -- BatchDenoiser, VadGate, TalkerPicker, ConferenceMixer --
on the golden recording against the restatements chained.  All bit for bit."""
import numpy as np
import pytest

import gate_cases as gc
import mix_cases as mc
import pick_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mem():
    return pc.TorchMem()


@pytest.mark.parametrize("k, decay, stick", pc.POLICIES)
@pytest.mark.parametrize("S, T", pc.SHAPES)
def test_against_the_restatement(gpu_lib, mem, S, T, k, decay, stick):
    pc.check_restatement(gpu_lib, mem, S, T, k, decay, stick)


def test_many_blocks(gpu_lib, mem):
    """4096 x 3 in rooms of 1 to 130 members spread over the streams: a thousand waves of k_pick_level, and blocks of every kind of
    k_pick_rank -- several of each but the largest rooms', of which there are as many as rooms."""
    S, T, k = 4096, 3, 3
    sizes, order = [1, 2, 3, 5, 8, 9, 40, 63, 64, 65, 130], (np.arange(S) * 37) % S
    room, at, n, lab = np.full(S, -1, np.int32), 0, 0, S - 1
    while at < S:
        m = sizes[n % len(sizes)]
        room[order[at:at + m]] = lab if m > 1 or n % 2 else -1
        at, n, lab = at + m, n + 1, lab - 1
    assert {len(g) for g in pc.groups(room)} >= set(sizes)
    pinned = (np.arange(S) % 11 == 0).astype(np.uint8)
    p, rs = pc.picker(gpu_lib, S, room, pinned, (k, 0.875, 4.0)), pc.Restated(S, room, pinned, k)
    for call in range(2):
        x, opn = pc.audio(40 + call, S, T), (np.random.default_rng(call).random((T, S)) < 0.5).astype(np.uint8)
        pc.same3(pc.device_call(p, mem, x, opn, layout="frames"), rs.select(x, opn), f"call {call}")
    assert rs.events >= {"takeover", "held_off", "none", "exactly_k", "more_than_k", "pin_over_louder"}
    p.close()


def test_chunking(gpu_lib, mem):
    pc.check_chunking(gpu_lib, mem)


def test_layout_and_formats(gpu_lib, mem):
    pc.check_layout(gpu_lib, mem)


def test_live_mask(gpu_lib, mem):
    pc.check_live(gpu_lib, mem)


def test_unread_inputs_do_not_matter(gpu_lib, mem):
    pc.check_unread(gpu_lib, mem)


def test_non_finite_samples_measure_silent(gpu_lib, mem):
    pc.check_nonfinite(gpu_lib, mem)


def test_consequences_of_the_rule(gpu_lib, mem):
    pc.check_consequences(gpu_lib, mem)


def test_bits_do_not_depend_on_n_streams_or_labels(gpu_lib, mem):
    pc.check_n_streams(gpu_lib, mem)


def test_reset_and_setters(gpu_lib, mem):
    pc.check_state(gpu_lib, mem)


def test_host_call(gpu_lib, mem):
    pc.check_host_call(gpu_lib, mem)


def test_refusals(gpu_lib, mem):
    pc.check_refusals(gpu_lib, mem)


def test_torch_tensors_on_torchs_stream(gpu_lib):
    """Audio, open and live are torch tensors made by kernels on a stream of torch's; TalkerPicker.select enqueues behind them on that
    stream, reading a permuted view of the batch's [T][S][480] that starts at an odd float, and torch goes on working with the result
    on the same stream."""
    import torch
    S, T, k = 80, 5, 3
    room, twins, sched, pins = pc.rooms_for(S, k)
    pinned = pc.pin_mask(S, pins)
    x, opn = pc.audio(61, S, T, twins, pins), pc.open_rows(62, S, T, 0, twins, sched, pins)
    live = (np.arange(S) % 5 != 2).astype(np.uint8)
    p, rs = pc.picker(gpu_lib, S, room, pinned, (k, 0.875, 4.0)), pc.Restated(S, room, pinned, k)
    dev = torch.device("cuda")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        flat = torch.cat([torch.zeros(1, device=dev), torch.from_numpy(x).to(dev).permute(1, 0, 2).reshape(-1)])[1:]
        a = flat.view(T, S, pc.FRAME).permute(1, 0, 2)                 # [S][T][480] over [T][S][480]
        to = torch.from_numpy(opn).to(dev) * 1
        tl = torch.from_numpy(live).to(dev)
        assert a.data_ptr() % 16 == 4
        talk, dom, lvl = p.select(a, open=to, live=tl, want_dominant=True, want_level=True)
        count = talk.sum()                                             # (torch goes on with the result on its stream)
    st.synchronize()
    want = [w.copy() for w in rs.select(x, opn, live=live)]
    for w in want:
        w[:, live == 0] = 0                                            # (the mirror hands back zeros where nothing was written)
    pc.same3((talk.cpu().numpy(), dom.cpu().numpy(), lvl.cpu().numpy()), want)
    assert int(count) == int(want[0].sum()) > 0
    # the default stream (handle 0 would mean "the object's own stream"): a side stream of torch's carries the call
    handles, device_call = [], p.select_device
    p.select_device = lambda *args, **kw: (handles.append(kw["hip_stream"]), device_call(*args, **kw))[1]
    talk2 = p.select(torch.from_numpy(x).to(dev) * 1.0, open=torch.from_numpy(opn).to(dev))
    got2 = talk2.clone()
    torch.cuda.synchronize()
    assert len(handles) == 1 and handles[0] not in (0, None)
    pc.same(got2.cpu().numpy(), rs.select(x, opn)[0], "on the default stream")
    p.close()


def test_server_tick_end_to_end(gpu_lib, golden_io):
    """One tick on one stream of work, 16 streams x 6 frames derived from the golden recording, after a warm-up call: BatchDenoiser.process,
    VadGate.apply in place with its open flags, TalkerPicker.select(open = open, live = !held), ConferenceMixer.apply(talk = picked),
    streams 3 and 9 held -- against the gate's, the picker's and the mixer's restatements chained on the batch's own output and VAD (the
    denoiser has no bit-exact restatement: DESIGN.md section 25).  A room of ten with gate threshold 0 and k = 2 has ten candidates in
    every frame: more than k by construction."""
    import nnnoiseless_amd as nn
    from nnnoiseless_amd.gate import VadGate
    from nnnoiseless_amd.mix import ConferenceMixer
    from nnnoiseless_amd.pick import TalkerPicker
    S, T, k = 16, 6, 2
    inp, _ = golden_io
    x = np.stack([inp[40 + 3 * s:40 + 3 * s + 2 * T] for s in range(S)]).astype(np.float32)      # [S, 12, 480]: a warm-up call and the tick
    held = [3, 9]
    room = np.array([5, 5, 5, 2, 5, 5, 5, 5, 5, 0, 5, 5, 2, 2, 0, -1], np.int32)
    ten = np.flatnonzero(room == 5)
    assert ten.size == 10 and not set(held) & set(ten.tolist())
    b = nn.BatchDenoiser(S, lib=gpu_lib)
    den0, vad0 = b.process(x[:, :T])
    b.hold_streams(held)
    den = np.full_like(x[:, T:], mc.SENT)
    vad = np.full((T, S), -1.0, np.float32)
    b.process(x[:, T:], out=den, vad=vad)
    live = (~b.held()).astype(np.uint8)
    b.close()
    thr = ((vad0.min(axis=0) + vad0.max(axis=0)) * np.float32(0.5)).astype(np.float32)      # halfway: every gate opens, most close too
    thr[ten] = 0
    par = {"threshold": thr, "grace": np.arange(S) % 2, "lookback": np.zeros(S, np.int64), "level": np.zeros(S, np.float32)}
    assert live.tolist() == [0 if s in held else 1 for s in range(S)]
    g, p, m = VadGate(S, 0, lib=gpu_lib), TalkerPicker(S, lib=gpu_lib), ConferenceMixer(S, lib=gpu_lib)
    g.set_params(par["threshold"], par["grace"], par["lookback"], par["level"])
    p.set_rooms(room), p.set_policy(k), m.set_rooms(room)
    rg, rp, rm = gc.Restated(S, 0, par), pc.Restated(S, room, None, k), mc.Restated(S, room)
    outs = []
    for call, (d, v, lv) in enumerate(((den0, vad0, None), (den, vad, live))):
        gated = d.copy()
        _, opn = g.apply(gated, v, live=lv, out=gated, want_open=True)                           # in place, as the server does
        picked, dom, lvl = p.select(gated, open=opn, live=lv, want_dominant=True, want_level=True)
        mixed, heard = m.apply(gated, talk=picked, live=lv, out=np.full_like(gated, mc.SENT), want_heard=True)
        wg, wo = rg.apply(d, v, live=lv, base=d)
        wp = [w.copy() for w in rp.select(wg, wo, live=lv)]
        if lv is not None:
            wo[:, lv == 0] = 0
            for w in wp:
                w[:, lv == 0] = 0
        mc.assert_same(gated, wg, f"call {call} gate"), mc.assert_same(opn, wo, f"call {call} open")
        pc.same3((picked, dom, lvl), wp, f"call {call} pick")
        wy, wh = rm.apply(wg, wp[0], live=lv)
        if lv is not None:
            wh[:, lv == 0] = 0
        mc.assert_same(mixed, wy, f"call {call} mix"), mc.assert_same(heard, wh, f"call {call} heard")
        assert (wo[1:, ten].sum(axis=1) == 10).all() and (wp[0][:, ten].sum(axis=1) == k).all()
        outs.append((mixed, wo, wp[0]))
    assert "more_than_k" in rp.events
    assert (outs[1][0][held] == mc.SENT).all()
    opens = np.concatenate([outs[0][1], outs[1][1][:, live == 1]], axis=1)
    assert (opens == 1).any() and (opens == 0).any(), "the gates open and close"
    assert (outs[1][2] < outs[1][1]).any(), "the picker closes open gates"
    assert max(rm.counts) >= 2 and (outs[0][0] != 0).any()
    g.close(), p.close(), m.close()
