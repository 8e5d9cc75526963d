"""Per-stream state records (include/nnn_batch.h NNN_STREAM_STATE_*) on the MI355X: reset and migration at sizes that take every
processing path (the one-frame tick through k_back, 24-frame groups through k_rnn_wf, two groups in flight above 16 384 streams, batches
sized for one-frame groups), an import between pipelined calls, the device-pointer variants on a caller's stream, a whole-batch
migration, and oracle parity of reset streams on real audio."""
import numpy as np
import pytest

from conftest import assert_flips_in_line, flip_stats

pytestmark = pytest.mark.gpu

IDX = [0, 33, 64, 69]     # reset: one tile's first stream, one inside, the next tile's first, one more
SRC = [5, 2, 130, 67, 71]  # migrated (never reset)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _noise(torch, S, T, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    amp = torch.rand((S, 1, 1), generator=g, device="cuda") * 3000.0 + 10.0
    return (torch.randn((S, T, 480), generator=g, device="cuda") * amp).contiguous()


def _run(bd, x, y, vad, calls, t0, stream):
    """Frames t0 .. of x [S, T, 480] (device) through bd in calls of the given lengths, back to back on `stream`; out into y, VAD into vad."""
    S, T = x.shape[0], x.shape[1]
    t = t0
    for n in calls:
        bd.process_device(x.data_ptr() + t * 1920, y.data_ptr() + t * 1920, vad.data_ptr() + t * S * 4, n, T * 480, 480, stream)
        t += n
    return t


def _batch(nn, S, mgf):
    return nn.BatchDenoiser(S, max_group_frames=mgf) if mgf else nn.BatchDenoiser(S)


def _reset_and_migrate(nn, torch, S, before, after, mgf=None, target_mgf=None):
    stream = torch.cuda.current_stream().cuda_stream
    Tb, Ta = sum(before), sum(after)
    x = _noise(torch, S, Tb + Ta, S + Tb)
    ya, yb = torch.zeros_like(x), torch.zeros_like(x)
    va, vb = torch.zeros((Tb + Ta, S), device="cuda"), torch.zeros((Tb + Ta, S), device="cuda")
    a = _batch(nn, S, mgf)
    _run(a, x, ya, va, before, 0, stream)
    torch.cuda.synchronize()
    b = a.clone()
    rec = a.export_streams(SRC)
    a.reset_streams(IDX)
    _run(a, x, ya, va, after, Tb, stream)
    _run(b, x, yb, vb, after, Tb, stream)
    # the reset streams: a fresh 4-stream batch fed the same frames
    xf = x[IDX, Tb:].contiguous()
    yf, vf = torch.zeros_like(xf), torch.zeros((Ta, 4), device="cuda")
    _run(_batch(nn, 4, mgf), xf, yf, vf, after, 0, stream)
    torch.cuda.synchronize()
    assert torch.equal(ya[IDX, Tb:], yf) and torch.equal(va[Tb:, IDX], vf)
    rest = torch.tensor([s for s in range(S) if s not in IDX], device="cuda")
    assert torch.equal(ya[rest, Tb:], yb[rest, Tb:]) and torch.equal(va[Tb:][:, rest], vb[Tb:][:, rest])
    del b
    # migration: another batch size, ring phase and group length, other slots, another order
    C = 1000
    dst = [999, 0, 512, 63, 64]
    c = _batch(nn, C, target_mgf)
    xc = _noise(torch, C, 3 + Ta, 7)
    yc, vc = torch.zeros_like(xc), torch.zeros((3 + Ta, C), device="cuda")
    _run(c, xc, yc, vc, [3], 0, stream)
    torch.cuda.synchronize()
    c.import_streams(dst, rec)
    xc[dst, 3:] = x[SRC, Tb:]
    _run(c, xc, yc, vc, after, 3, stream)
    torch.cuda.synchronize()
    assert torch.equal(yc[dst, 3:], ya[SRC, Tb:]) and torch.equal(vc[3:][:, dst], va[Tb:][:, SRC])
    # and back out of it into a batch of the first kind
    back = c.export_streams([512])
    d = _batch(nn, 70, mgf)
    xd = _noise(torch, 70, 2 + Ta, 9)
    yd, vd = torch.zeros_like(xd), torch.zeros((2 + Ta, 70), device="cuda")
    _run(d, xd, yd, vd, [2], 0, stream)
    torch.cuda.synchronize()
    d.import_streams([69], back)
    xd[69, 2:] = xc[512, 3:]
    xc2 = xc.clone()
    _run(d, xd, yd, vd, after, 2, stream)
    _run(c, xc2, yc, vc, after, 3, stream)
    torch.cuda.synchronize()
    assert torch.equal(yd[69, 2:], yc[512, 3:])
    del a, c, d, x, ya, yb, xc, yc, xd, yd
    torch.cuda.empty_cache()


def test_tick_path_4096_one_frame_calls(torch):
    import nnnoiseless_amd as nn
    _reset_and_migrate(nn, torch, 4096, [1] * 11, [1] * 9)


def test_rnn_wf_path_4096_24_frame_calls(torch):
    import nnnoiseless_amd as nn
    _reset_and_migrate(nn, torch, 4096, [24], [24, 1, 3])


def test_two_groups_in_flight_32768_48_frame_calls(torch):
    import nnnoiseless_amd as nn
    _reset_and_migrate(nn, torch, 32768, [48], [48])


def test_one_frame_batches_to_and_from_default(torch):
    import nnnoiseless_amd as nn
    _reset_and_migrate(nn, torch, 300, [1] * 7, [1, 3, 5], mgf=1)          # mgf=1 -> default -> mgf=1
    _reset_and_migrate(nn, torch, 300, [5, 2], [1, 3, 5], target_mgf=1)    # default -> mgf=1 -> default


def test_import_between_pipelined_calls_and_device_variants_on_a_caller_stream(torch):
    """set_inputs_ready(True): the second call's high-pass may start before the first drains -- not across an import.  Records
    device to device on a torch stream of the caller's, no host synchronisation between the calls."""
    import nnnoiseless_amd as nn
    S, T = 4096, 96
    s = torch.cuda.Stream()
    x = _noise(torch, S, T, 1)
    donor = nn.BatchDenoiser(S)
    xd = _noise(torch, S, 40, 2)
    yd = torch.zeros_like(xd)
    vd = torch.zeros((40, S), device="cuda")
    _run(donor, xd, yd, vd, [40], 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    idx = list(range(100, 164)) + [7, 4095]
    rec_host = donor.export_streams(idx)
    a = nn.BatchDenoiser(S)
    r = a.clone()
    a.set_inputs_ready(True)
    ya, yr = torch.zeros_like(x), torch.zeros_like(x)
    va, vr = torch.zeros((T, S), device="cuda"), torch.zeros((T, S), device="cuda")
    d_rec = torch.zeros((len(idx), nn.STREAM_STATE_BYTES), dtype=torch.uint8, device="cuda")
    d_out = torch.zeros_like(d_rec)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        donor.export_streams_device(idx, d_rec.data_ptr(), s.cuda_stream)
        _run(a, x, ya, va, [48], 0, s.cuda_stream)
        a.import_streams_device(idx, d_rec.data_ptr(), s.cuda_stream)
        a.export_streams_device(idx, d_out.data_ptr(), s.cuda_stream)
        _run(a, x, ya, va, [48], 48, s.cuda_stream)
    s.synchronize()
    a.synchronize()
    _run(r, x, yr, vr, [48], 0, 0)
    r.synchronize()
    r.import_streams(idx, rec_host)
    _run(r, x, yr, vr, [48], 48, 0)
    r.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), rec_host)
    assert torch.equal(ya, yr) and torch.equal(va, vr)


def test_device_import_refusal_writes_nothing_and_is_reported(torch):
    import nnnoiseless_amd as nn
    S = 256
    a = nn.BatchDenoiser(S)
    x = _noise(torch, S, 4, 3)
    y, v = torch.zeros_like(x), torch.zeros((4, S), device="cuda")
    torch.cuda.synchronize()
    _run(a, x, y, v, [2], 0, 0)
    before = a.export_streams(range(S))
    bad = torch.from_numpy(before[:80].copy()).cuda()
    bad[79, 12] = 7                                                  # GRU sizes of another model
    torch.cuda.synchronize()
    a.import_streams_device(list(range(80)), bad.data_ptr())
    with pytest.raises(RuntimeError, match="did not match"):
        a.synchronize()
    a.synchronize()                                                  # (reported once)
    assert np.array_equal(a.export_streams(range(S)), before)


def test_whole_batch_migration_65536(torch):
    import nnnoiseless_amd as nn
    S, T = 65536, 48
    stream = torch.cuda.current_stream().cuda_stream
    x = _noise(torch, S, T, 5)
    ya, yb = torch.zeros_like(x), torch.zeros_like(x)
    va, vb = torch.zeros((T, S), device="cuda"), torch.zeros((T, S), device="cuda")
    a = nn.BatchDenoiser(S)
    _run(a, x, ya, va, [48], 0, stream)
    rec = torch.zeros((S, nn.STREAM_STATE_BYTES), dtype=torch.uint8, device="cuda")
    a.export_streams_device(range(S), rec.data_ptr(), stream)
    b = nn.BatchDenoiser(S)
    _run(b, x, yb, vb, [5], 0, stream)                               # another ring phase
    b.import_streams_device(range(S), rec.data_ptr(), stream)
    _run(a, x, ya, va, [48], 0, stream)
    _run(b, x, yb, vb, [48], 0, stream)
    torch.cuda.synchronize()
    a.synchronize()
    b.synchronize()
    assert torch.equal(ya, yb) and torch.equal(va, vb)
    del a, b, x, ya, yb, rec
    torch.cuda.empty_cache()


def test_reset_streams_against_the_oracle_on_real_audio(torch, oracle_mod, weights_bytes, golden_io):
    import nnnoiseless_amd as nn
    frames = golden_io[0].reshape(-1)
    S, Tb, Ta = 256, 20, 60
    n = (Tb + Ta) * 480
    x = np.stack([np.roll(frames, -4800 * s - 480 * (s % 7))[:n] for s in range(S)]).reshape(S, Tb + Ta, 480).astype(np.float32)
    bd = nn.BatchDenoiser(S)
    bd.process(x[:, :Tb])
    idx = [3, 100, 255]
    bd.reset_streams(idx)
    xd = torch.from_numpy(x).cuda()
    yd = torch.zeros_like(xd)
    vd = torch.zeros((Tb + Ta, S), device="cuda")
    log = torch.zeros((Ta, S, 24), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    bd.set_frame_log(log.data_ptr(), Ta)
    _run(bd, xd, yd, vd, [1] * 10 + [50], Tb, 0)
    bd.synchronize()
    torch.cuda.synchronize()
    lg = log.cpu().numpy()[:, idx]                                    # [Ta, 3, 24]
    out = yd.cpu().numpy()[idx, Tb:]
    xs = x[idx, Tb:]
    ref = oracle_mod.run_streams(oracle_mod.Model(weights_bytes), xs, want=("out", "pitch", "branch", "vad"))
    ref32 = oracle_mod.run_streams(oracle_mod.Model(weights_bytes, f32_fft=True), xs, want=("out", "branch"))
    assert np.array_equal(lg[:, :, 0].T, ref["pitch"])
    branch = lg[:, :, 1].T
    st = flip_stats(branch, out, ref, ref32)
    assert_flips_in_line(st, "reset streams")
    flip = branch != ref["branch"]
    excused = flip.copy()
    excused[:, 1:] |= flip[:, :-1]
    ok = ~excused[:, 1:]
    d = (out[:, 1:] - ref["out"][:, 1:]).astype(np.float64)
    rr = ref["out"][:, 1:].astype(np.float64)
    assert np.sqrt((d[ok] ** 2).sum() / (rr[ok] ** 2).sum()) <= 1e-4
    assert np.abs(vd.cpu().numpy()[Tb:, idx].T - ref["vad"]).max() <= 1e-4
