"""Hold and resume (include/nnn_batch.h nnn_batch_hold_streams / nnn_batch_resume_streams) on the MI355X, at the sizes that take every
processing path: the one-frame tick (k_back and the riders of its launches), 24-frame groups (k_rnn_wf, chained k_pitch), pipelined
48-frame calls with the held set changed between them, two groups in flight above 16 384 streams (looped k_pitch), a batch sized for
one-frame groups, two resident models, a caller's stream without host synchronisation, and oracle parity on real audio.

Every scenario is checked the same way.  Batch A runs a list of steps, each a set of held streams and some calls; the held streams' input
is NaN and the output / VAD buffers are pre-filled with a sentinel.  Twin B holds nothing and is fed, per stream, exactly the frames that
stream was live for in A (a stream never held: every frame).  A's output and VAD equal B's bit for bit on every live frame of every
stream, the sentinel is intact on every held frame, and nnn_batch_fault stays 0."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, assert_flips_in_line, flip_stats

pytestmark = pytest.mark.gpu

SENT = -12345.0


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _noise(torch, S, T, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    amp = torch.rand((S, 1, 1), generator=g, device="cuda") * 3000.0 + 10.0
    return (torch.randn((S, T, 480), generator=g, device="cuda") * amp).contiguous()


def _calls(bd, x, y, vad, calls, t, stream):
    S, T = x.shape[0], x.shape[1]
    for n in calls:
        bd.process_device(x.data_ptr() + t * 1920, y.data_ptr() + t * 1920, vad.data_ptr() + t * S * 4, n, T * 480, 480, stream)
        t += n
    return t


def _mixed(S):
    """Scattered singles, one whole tile, every second 16-stream block of four more tiles."""
    singles = [0, 33, 64 + 17, S - 1, S // 2 + 5]
    tile = list(range(3 * 64, 4 * 64)) if S >= 1024 else list(range(64, 128))
    blocks = [s for s in range(8 * 64, 12 * 64) if (s // 16) % 2 == 0] if S >= 1024 else list(range(16, 32))
    return sorted(set(s for s in singles + tile + blocks if s < S))


def _scenario(nn, torch, S, steps, make=None, stream=0, inputs_ready=False, x=None):
    """steps: [(held streams, [call lengths])].  Nothing between the steps waits for the device."""
    T = sum(sum(c) for _, c in steps)
    x = _noise(torch, S, T, S + T) if x is None else x
    live = torch.ones((S, T), dtype=torch.bool, device="cuda")
    t = 0
    for held, calls in steps:
        if len(held):
            live[torch.tensor(list(held), device="cuda"), t:t + sum(calls)] = False
        t += sum(calls)
    xa = x.clone()
    xa[~live] = float("nan")
    ya, va = torch.full_like(x, SENT), torch.full((T, S), SENT, device="cuda")
    make = make or (lambda: nn.BatchDenoiser(S))
    a = make()
    a.set_inputs_ready(inputs_ready)
    torch.cuda.synchronize()
    now, t = set(), 0
    for held, calls in steps:
        held = set(held)
        if now - held:
            a.resume_streams(sorted(now - held))
        if held - now:
            a.hold_streams(sorted(held - now))
        now = held
        assert a.num_held() == len(now)
        t = _calls(a, xa, ya, va, calls, t, stream)
    a.synchronize()
    torch.cuda.synchronize()
    assert not a.fault()
    # twin B: every stream's live frames, packed to the front
    order = torch.argsort((~live).to(torch.uint8), dim=1, stable=True)                       # [S, T]: live frames first, in order
    flat = (torch.arange(S, device="cuda")[:, None] * T + order).reshape(-1)
    xb = x.reshape(S * T, 480)[flat].reshape(S, T, 480).contiguous()
    del xa
    yb, vb = torch.zeros_like(x), torch.zeros((T, S), device="cuda")
    b = make()
    torch.cuda.synchronize()
    _calls(b, xb, yb, vb, [c for _, calls in steps for c in calls], 0, 0)
    b.synchronize()
    torch.cuda.synchronize()
    assert not b.fault()
    del xb
    packed = torch.arange(T, device="cuda")[None, :] < live.sum(1)[:, None]                    # [S, T]: B's frames that exist in A
    ya_packed = ya.reshape(S * T, 480)[flat].reshape(S, T, 480)
    va_packed = va.t().reshape(S * T)[flat].reshape(S, T)
    assert torch.equal(ya_packed[packed], yb[packed])
    assert torch.equal(va_packed[packed], vb.t()[packed])
    assert bool((ya[~live] == SENT).all()) and bool((va.t()[~live] == SENT).all())
    del a, b, x, ya, yb, ya_packed
    torch.cuda.empty_cache()


def test_tick_path_4096_one_frame_calls(torch):
    import nnnoiseless_amd as nn
    S = 4096
    _scenario(nn, torch, S, [([], [1] * 5), (_mixed(S), [1] * 4), ([], [1] * 4)])
    _scenario(nn, torch, S, [([], [1] * 3), (list(range(1, S)), [1] * 3), ([], [1] * 3)])                  # all but one stream


def test_rnn_wf_path_4096_24_frame_calls(torch):
    import nnnoiseless_amd as nn
    S = 4096
    _scenario(nn, torch, S, [([], [24]), (_mixed(S), [24, 1]), ([], [24])])
    _scenario(nn, torch, S, [([], [24]), ([s for s in range(S) if s != 2000], [24]), ([], [3, 24])])   # all but one stream


def test_pipelined_4096_48_frame_calls_held_set_changes_between_them(torch):
    import nnnoiseless_amd as nn
    S = 4096
    h1 = _mixed(S)
    h2 = sorted(set([1, 34, 4000] + list(range(20 * 64, 22 * 64)) + [s for s in range(30 * 64, 33 * 64) if (s // 16) % 2 == 1]))
    _scenario(nn, torch, S, [([], [48]), (h1, [48]), (h2, [48]), ([], [48])], inputs_ready=True)


def test_two_groups_in_flight_20480_48_frame_calls(torch):
    import nnnoiseless_amd as nn
    S = 20480
    _scenario(nn, torch, S, [([], [5]), (_mixed(S), [48]), ([], [48])])


def test_batch_sized_for_one_frame_groups(torch):
    import nnnoiseless_amd as nn
    S = 300
    make = lambda: nn.BatchDenoiser(S, max_group_frames=1)
    _scenario(nn, torch, S, [([], [1] * 6), (_mixed(S), [1, 3, 1]), ([], [5, 1])], make=make)


def test_grouped_models_a_whole_model_group_held(torch):
    import nnnoiseless_amd as nn
    sh = nn.RnnModel.from_bytes(open(os.path.join(GOLDEN, "sh.rnn"), "rb").read())
    S = 128 + 70
    make = lambda: nn.BatchDenoiser(S, groups=[(None, 128), (sh, 70)])
    _scenario(nn, torch, S, [([], [4]), (list(range(128, S)), [1, 24, 2]), (list(range(0, 128)), [1, 5]), ([], [24])], make=make)


def test_device_calls_on_a_caller_stream_without_host_synchronisation(torch):
    """Hold and resume are enqueued (on the batch's own stream, ordered with the calls by events): the caller's stream is never waited
    for between the steps."""
    import nnnoiseless_amd as nn
    S = 1024
    s = torch.cuda.Stream()
    x = _noise(torch, S, 40, 11)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        _scenario(nn, torch, S, [([], [1, 7]), (_mixed(S), [1, 1, 6]), ([5, 6, 7, 8], [24])], stream=s.cuda_stream, x=x)


def test_held_and_resumed_streams_against_the_oracle_on_real_audio(torch, oracle_mod, weights_bytes, golden_io):
    import nnnoiseless_amd as nn
    frames = golden_io[0].reshape(-1)
    S, Tb, Th, Ta = 256, 20, 12, 40
    T = Tb + Th + Ta
    x = np.stack([np.roll(frames, -4800 * s - 480 * (s % 7))[:T * 480] for s in range(S)]).reshape(S, T, 480).astype(np.float32)
    idx = [3, 100, 255]
    bd = nn.BatchDenoiser(S)
    xd = torch.from_numpy(x).cuda()
    xd[idx, Tb:Tb + Th] = float("nan")
    yd = torch.full_like(xd, SENT)
    vd = torch.full((T, S), SENT, device="cuda")
    log = torch.zeros((T, S, 24), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    bd.set_frame_log(log.data_ptr(), T)
    _calls(bd, xd, yd, vd, [Tb], 0, 0)
    bd.hold_streams(idx)
    _calls(bd, xd, yd, vd, [1] * 4 + [Th - 4], Tb, 0)
    bd.resume_streams(idx)
    _calls(bd, xd, yd, vd, [1] * 10 + [Ta - 10], Tb + Th, 0)
    bd.synchronize()
    torch.cuda.synchronize()
    assert not bd.fault()
    live = list(range(Tb)) + list(range(Tb + Th, T))
    lg = log.cpu().numpy()[live][:, idx]
    out = yd.cpu().numpy()[idx][:, live]
    assert (yd[idx, Tb:Tb + Th] == SENT).all() and (vd[Tb:Tb + Th][:, idx] == SENT).all()
    xs = x[idx][:, live]
    ref = oracle_mod.run_streams(oracle_mod.Model(weights_bytes), xs, want=("out", "pitch", "branch", "vad"))
    ref32 = oracle_mod.run_streams(oracle_mod.Model(weights_bytes, f32_fft=True), xs, want=("out", "branch"))
    assert np.array_equal(lg[:, :, 0].T, ref["pitch"])
    branch = lg[:, :, 1].T
    st = flip_stats(branch, out, ref, ref32)
    assert_flips_in_line(st, "held and resumed streams")
    flip = branch != ref["branch"]
    excused = flip.copy()
    excused[:, 1:] |= flip[:, :-1]
    ok = ~excused[:, 1:]
    d = (out[:, 1:] - ref["out"][:, 1:]).astype(np.float64)
    rr = ref["out"][:, 1:].astype(np.float64)
    assert np.sqrt((d[ok] ** 2).sum() / (rr[ok] ** 2).sum()) <= 1e-4
    assert np.abs(vd.cpu().numpy()[live][:, idx].T - ref["vad"]).max() <= 1e-4


def test_device_record_calls_on_held_streams_on_a_caller_stream(torch):
    """export_streams_device / import_streams_device on a caller's stream meet held streams as the header's table says: the parked record
    out, a record in (the stream stays held), in lists that mix held and live streams; no host synchronisation in between."""
    import nnnoiseless_amd as nn
    S = 256
    held = [5, 200] + list(range(64, 128))
    s = torch.cuda.Stream()
    x = _noise(torch, S, 8, 21)
    y, v = torch.zeros_like(x), torch.zeros((8, S), device="cuda")
    a = nn.BatchDenoiser(S)
    torch.cuda.synchronize()
    _calls(a, x, y, v, [3], 0, s.cuda_stream)
    a.synchronize()
    ref = a.clone()
    before = a.export_streams(range(S))
    lst = [64, 7, 5, 130, 100]                                                       # held, live, held, live, held
    d_rec = torch.zeros((len(lst), nn.STREAM_STATE_BYTES), dtype=torch.uint8, device="cuda")
    d_all = torch.zeros((S, nn.STREAM_STATE_BYTES), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        a.hold_streams(held)
        _calls(a, x, y, v, [2], 3, s.cuda_stream)
        a.export_streams_device(lst, d_rec.data_ptr(), s.cuda_stream)
        a.import_streams_device([100, 7], d_rec[1:3].data_ptr(), s.cuda_stream)      # held 100 <- live 7's record, live 7 <- held 5's parked one
        a.export_streams_device(range(S), d_all.data_ptr(), s.cuda_stream)           # (the tile kernels, then the parked records over them)
        a.resume_streams(held)
        _calls(a, x, y, v, [3], 5, s.cuda_stream)
    s.synchronize()
    a.synchronize()
    assert not a.fault()
    yr, vr = torch.zeros_like(x), torch.zeros((8, S), device="cuda")
    _calls(ref, x, yr, vr, [2], 3, 0)
    ref.synchronize()
    rec = d_rec.cpu().numpy()
    assert np.array_equal(rec[[0, 2, 4]], before[[64, 5, 100]]) and np.array_equal(rec[[1, 3]], ref.export_streams([7, 130]))
    everything = d_all.cpu().numpy()
    want = ref.export_streams(range(S))
    want[held] = before[held]
    want[[100, 7]] = rec[1:3]
    assert np.array_equal(everything, want)
    ref.import_streams(range(S), want)                                               # every stream as A has it at the resume
    _calls(ref, x, yr, vr, [3], 5, 0)
    ref.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(y[:, 5:], yr[:, 5:]) and torch.equal(v[5:], vr[5:])
