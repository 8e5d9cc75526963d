"""The split calls (include/nnn_batch.h "Split calls") on the MI355X through the device entry points, features and gains resident as torch
tensors on torch's current stream: the shapes of test_hostsim_split.py (70 streams with max_group_frames = 2, pairs of 1 and 2 frames over
a ring that wraps; 3 streams, pairs of 1, 2 and 24 frames -- their rows start on 8-byte boundaries only) and one of more than one round of
blocks, 4160 streams x 4 frames.  Batch A (one-frame processing calls, taps on) and batch B (split pairs fed A's raw gains) run once per
shape and are shared by the tests."""
import numpy as np
import pytest

import test_hostsim_split as hs
from test_hostsim_split import GRU, _bits

pytestmark = pytest.mark.gpu

SHAPES = dict(hs.SHAPES, s4160=(5, 4160, 4, None, (4,), 7, (1, 3)))
SENT = -12345.0


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def make_input(name):
    if name in hs.SHAPES:
        return hs.make_input(name)
    from nnnoiseless_amd.synthetic import make_streams_fast
    seed, S, T, _, _, quiet, zeros = SHAPES[name]
    x = make_streams_fast(S, T, seed=seed)
    x[quiet] = hs.quiet_stream(T, zeros)
    return x


def _st(torch):
    return torch.cuda.current_stream().cuda_stream


def run_ordinary(nn, torch, x, mgf):
    """A: one-frame process_device calls, taps on.  out (tensor [S, T, 480]), features / silence / g_raw / vad taps as numpy [T, S, len]."""
    S, T = x.shape[:2]
    a = nn.BatchDenoiser(S, max_group_frames=mgf, taps=True)
    y, vad = torch.zeros_like(x), torch.zeros((T, S), device="cuda")
    torch.cuda.synchronize()
    taps = {k: [] for k in ("features", "silence", "g_raw", "vad")}
    for t in range(T):
        a.process_device(x.data_ptr() + t * 1920, y.data_ptr() + t * 1920, vad.data_ptr() + t * S * 4, 1, T * 480, 480, _st(torch))
        for k in taps:
            taps[k].append(a.tap(k))
    r = {k: np.stack(v) for k, v in taps.items()}
    r["out"], r["records"] = y, a.export_streams(range(S))
    assert not a.fault()
    return r


def split_pair(bd, torch, x, F, SIL, G, V, y, pos, n):
    """One analyze / synthesize pair of n frames from frame `pos` of the [.., T, ..] tensors, nothing waiting in between."""
    from nnnoiseless_amd import _ffi
    S, T = x.shape[:2]
    bd.analyze_device(x.data_ptr() + pos * 1920, F.data_ptr() + pos * S * 42 * 4, SIL.data_ptr() + pos * S * 4, n, _ffi.PCM_F32, 1, T * 480, 480, _st(torch))
    assert bd.pending_frames() == n
    bd.synthesize_device(G.data_ptr() + pos * S * 22 * 4, None if V is None else V.data_ptr() + pos * S * 4, y.data_ptr() + pos * 1920, n,
                         _ffi.PCM_F32, 1, T * 480, 480, hip_stream=_st(torch))
    assert bd.pending_frames() == 0


def run_split(nn, torch, x, mgf, pairs, G, V):
    S, T = x.shape[:2]
    b = nn.BatchDenoiser(S, max_group_frames=mgf)
    F, SIL, y = torch.zeros((T, S, 42), device="cuda"), torch.zeros((T, S), dtype=torch.int32, device="cuda"), torch.zeros_like(x)
    torch.cuda.synchronize()
    pos = 0
    for n in pairs:
        split_pair(b, torch, x, F, SIL, G, V, y, pos, n)
        pos += n
    b.synchronize()
    torch.cuda.synchronize()
    assert not b.fault()
    return {"features": F, "silence": SIL, "out": y, "records": b.export_streams(range(S))}


_CACHE = {}


@pytest.fixture(scope="module")
def runs(torch):
    import nnnoiseless_amd as nn

    def get(name):
        if name not in _CACHE:
            mgf, pairs = SHAPES[name][3], SHAPES[name][4]
            x = torch.from_numpy(make_input(name)).cuda()
            a = run_ordinary(nn, torch, x, mgf)
            G, V = torch.from_numpy(a["g_raw"]).cuda(), torch.from_numpy(np.ascontiguousarray(a["vad"][:, :, 0])).cuda()
            _CACHE[name] = (x, a, run_split(nn, torch, x, mgf, pairs, G, V), G, V)
        return _CACHE[name]
    return get


@pytest.mark.parametrize("name", list(SHAPES))
def test_features_are_the_ordinary_paths(runs, name):
    x, a, b, _, _ = runs(name)
    assert np.array_equal(_bits(b["features"].cpu().numpy()), _bits(a["features"]))
    assert np.array_equal(b["silence"].cpu().numpy(), a["silence"][:, :, 0])
    sil = a["silence"][:, SHAPES[name][5], 0]
    assert sil.any() and not sil[0] and not sil[-1], sil


@pytest.mark.parametrize("name", list(SHAPES))
def test_round_trip_is_the_ordinary_path(runs, torch, name):
    from nnnoiseless_amd import _ffi
    x, a, b, _, _ = runs(name)
    assert torch.equal(a["out"], b["out"])
    for k in _ffi.STREAM_STATE_FIELDS:
        fa, fb = _ffi.stream_state_field(a["records"], k), _ffi.stream_state_field(b["records"], k)
        if k in GRU:
            assert fa.any() and not _bits(fb).any(), k
        else:
            assert np.array_equal(_bits(fa), _bits(fb)), k


def test_round_trip_through_two_channel_int16(runs, torch):
    """2-channel int16 through the device calls against process_pcm_device (integer inputs: both boundaries see A's samples)."""
    import nnnoiseless_amd as nn
    from nnnoiseless_amd import _ffi
    x, a, _, G, _ = runs("s70")
    S, T = x.shape[:2]
    pcm = x.to(torch.int16).reshape(S // 2, 2, T * 480).permute(0, 2, 1).contiguous()      # [G, T * 480, 2]
    want, got, vad = torch.zeros_like(pcm), torch.zeros_like(pcm), torch.zeros((T, S), device="cuda")
    F, SIL = torch.zeros((T, S, 42), device="cuda"), torch.zeros((T, S), dtype=torch.int32, device="cuda")
    w, b = nn.BatchDenoiser(S, max_group_frames=2), nn.BatchDenoiser(S, max_group_frames=2)
    torch.cuda.synchronize()
    gs, fs, e = T * 960, 960, 2                                                               # strides in elements, element bytes
    w.process_pcm_device(pcm.data_ptr(), want.data_ptr(), vad.data_ptr(), T, _ffi.PCM_I16, 2, gs, fs, hip_stream=_st(torch))
    pos = 0
    for n in SHAPES["s70"][4]:
        b.analyze_device(pcm.data_ptr() + pos * fs * e, F.data_ptr() + pos * S * 168, SIL.data_ptr() + pos * S * 4, n, _ffi.PCM_I16, 2, gs, fs, _st(torch))
        b.synthesize_device(G.data_ptr() + pos * S * 88, None, got.data_ptr() + pos * fs * e, n, _ffi.PCM_I16, 2, gs, fs, hip_stream=_st(torch))
        pos += n
    w.synchronize(), b.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(want, got) and np.array_equal(_bits(F.cpu().numpy()), _bits(a["features"]))


def test_held_streams_sit_out_split_calls(runs, torch):
    """Stream 5 and the whole second tile held: sentinel-filled feature, silence and output tensors keep their sentinels in the held rows
    (input and gains NaN there), live rows are the nothing-held run's bit for bit, the held streams, resumed, continue bit for bit (a
    twin that ran only the frames they were live for); a pair with everything held launches nothing, pending_frames n -> 0."""
    import nnnoiseless_amd as nn
    x, a, b0, G, V = runs("s70")
    S, T = x.shape[:2]
    held = [5] + list(range(64, 70))
    hidx = torch.tensor(held, device="cuda")
    live = torch.ones(S, dtype=torch.bool, device="cuda")
    live[hidx] = False
    steps = [(0, 1), (1, 2), (3, 2), (5, 1), (6, 2), (8, 2), (10, 2)]                         # (first frame, frames); held for frames 3 .. 7
    xa, ga = x.clone(), G.clone()
    xa[hidx, 3:8], ga[3:8, hidx] = float("nan"), float("nan")
    F, SIL, y = torch.full((T, S, 42), SENT, device="cuda"), torch.full((T, S), -77, dtype=torch.int32, device="cuda"), torch.full_like(x, SENT)
    h = nn.BatchDenoiser(S, max_group_frames=2)
    torch.cuda.synchronize()
    for pos, n in steps:
        if pos == 3:
            h.hold_streams(held)
        if pos == 8:
            h.resume_streams(held)
        split_pair(h, torch, xa, F, SIL, ga, V, y, pos, n)
    h.synchronize()
    torch.cuda.synchronize()
    assert not h.fault()
    assert bool((F[3:8, hidx] == SENT).all()) and bool((SIL[3:8, hidx] == -77).all()) and bool((y[hidx, 3:8] == SENT).all())
    assert torch.equal(F[:, live], b0["features"][:, live]) and torch.equal(SIL[:, live], b0["silence"][:, live])
    assert torch.equal(y[live], b0["out"][live]) and torch.equal(y[hidx, :3], b0["out"][hidx, :3])
    # the twin: frames 0 .. 2 and 8 .. 11 only
    keep = [0, 1, 2, 8, 9, 10, 11]
    xt, gt, vt = x[:, keep].contiguous(), G[keep].contiguous(), V[keep].contiguous()
    Ft, St, yt = torch.zeros((7, S, 42), device="cuda"), torch.zeros((7, S), dtype=torch.int32, device="cuda"), torch.zeros_like(xt)
    twin = nn.BatchDenoiser(S, max_group_frames=2)
    torch.cuda.synchronize()
    for pos, n in ((0, 1), (1, 2), (3, 2), (5, 2)):
        split_pair(twin, torch, xt, Ft, St, gt, vt, yt, pos, n)
    twin.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(y[hidx, 8:], yt[hidx, 3:]) and torch.equal(F[8:, hidx], Ft[3:, hidx]) and torch.equal(SIL[8:, hidx], St[3:, hidx])
    # every stream held
    d = nn.BatchDenoiser(S, max_group_frames=2)
    F2, S2, y2 = torch.full((T, S, 42), SENT, device="cuda"), torch.full((T, S), -77, dtype=torch.int32, device="cuda"), torch.full_like(x, SENT)
    torch.cuda.synchronize()
    split_pair(d, torch, x, F2, S2, G, V, y2, 0, 2)
    d.hold_streams(range(S))
    nan_x, nan_g = torch.full_like(x, float("nan")), torch.full_like(G, float("nan"))
    split_pair(d, torch, nan_x, F2, S2, nan_g, None, y2, 2, 2)
    split_pair(d, torch, nan_x, F2, S2, nan_g, None, y2, 4, 1)
    d.resume_streams(range(S))
    split_pair(d, torch, x, F2, S2, G, V, y2, 5, 2)                                          # frames 5, 6 given: for the streams they follow frame 1
    e = nn.BatchDenoiser(S, max_group_frames=2)
    ye, Fe, Se = torch.zeros_like(x), torch.zeros((T, S, 42), device="cuda"), torch.zeros((T, S), dtype=torch.int32, device="cuda")
    split_pair(e, torch, x, Fe, Se, G, V, ye, 0, 2)
    xe = x.clone()
    xe[:, 2:4] = x[:, 5:7]
    ge, ve = G.clone(), V.clone()
    ge[2:4], ve[2:4] = G[5:7], V[5:7]
    split_pair(e, torch, xe, Fe, Se, ge, ve, ye, 2, 2)
    d.synchronize(), e.synchronize()
    torch.cuda.synchronize()
    assert bool((F2[2:5] == SENT).all()) and bool((S2[2:5] == -77).all()) and bool((y2[:, 2:5] == SENT).all())
    assert torch.equal(y2[:, 5:7], ye[:, 2:4]) and torch.equal(F2[5:7], Fe[2:4])


@pytest.mark.parametrize("name", ["s3", "s4160"])
def test_alternation_with_ordinary_calls(runs, torch, name):
    """Ordinary call, split pair (A's gains), ordinary call: the first call's and the pair's audio are A's bit for bit, the GRU blocks of
    the records are unchanged across the pair, and the last call's features are A's (its audio continues from the GRU state the first
    call left, which is what the split calls are for)."""
    import nnnoiseless_amd as nn
    from nnnoiseless_amd import _ffi
    x, a, _, G, V = runs(name)
    S, T = x.shape[:2]
    n1, n2 = (3, 2) if T > 4 else (1, 2)
    m = nn.BatchDenoiser(S, taps=True)
    y, vad = torch.zeros_like(x), torch.zeros((T, S), device="cuda")
    F, SIL = torch.zeros((T, S, 42), device="cuda"), torch.zeros((T, S), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    m.process_device(x.data_ptr(), y.data_ptr(), vad.data_ptr(), n1, T * 480, 480, _st(torch))
    idx = list(range(0, S, max(1, S // 64)))
    before = m.export_streams(idx)
    split_pair(m, torch, x, F, SIL, G, V, y, n1, n2)
    after = m.export_streams(idx)
    p = n1 + n2
    m.process_device(x.data_ptr() + p * 1920, y.data_ptr() + p * 1920, vad.data_ptr() + p * S * 4, 1, T * 480, 480, _st(torch))
    m.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(y[:, :p], a["out"][:, :p])
    assert np.array_equal(_bits(F[n1:p].cpu().numpy()), _bits(a["features"][n1:p]))
    for k in GRU:
        fb = _ffi.stream_state_field(before, k)
        assert fb.any() and np.array_equal(_bits(fb), _bits(_ffi.stream_state_field(after, k))), k
    assert np.array_equal(_bits(m.tap("features")), _bits(a["features"][p]))
