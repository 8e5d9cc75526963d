"""What the rate adapter's tests share (test_hostsim_rate.py under the SIMT interpreter, test_gpu_rate.py on the GPU library): the input,
the yardstick and the runs.  The yardstick is built from pieces that are pinned elsewhere -- the CPU restatement of the CLI's resampler does
both legs, the SAME library's BatchDenoiser.process goes between them in one big call ("every way of running a frame gives the same
bits") -- so every comparison is bit for bit:

    up[s]      = resample(x[s], rate / 48000);  T = len(up[s]) // 480
    out48, vad = BatchDenoiser(S).process(up[:, :T * 480])
    want[s]    = resample(out48[s], 48000 / rate)
"""
import numpy as np

SENT = np.float32(-12345.0)   # what the caller's buffers hold where a held stream would write


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def signal(S, n, rate, seed=0, loud=()):
    """S streams of a tone in noise at `rate`, float32 in the int16 range; streams in `loud` are full-scale square waves."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    f = rng.uniform(100.0, 0.2 * rate, (S, 1))
    x = 8000.0 * np.sin(2 * np.pi * f * t / rate) + 300.0 * rng.standard_normal((S, n))
    for s in loud:
        x[s] = 32767.0 * np.sign(np.sin(2 * np.pi * 220.0 * t / rate) + 1e-9)
    return x.astype(np.float32)


def yardstick(lib, oracle, x, rate, restart=None, events=()):
    """(want [S, n_out], vad [T, S], len(up)) for input x [S, n].  restart = {stream: (source samples, frame)}: from that frame on the
    stream's 48 kHz input is what its source gives with those first samples zeroed (its up-leg restarted from silence there), and its
    denoised 48 kHz signal before that frame is zeroed for the down-leg.  events = [(frame, "reset" | "hold" | "resume", streams)],
    applied to the yardstick batch before that frame."""
    import nnnoiseless_amd as nn
    x = np.asarray(x, np.float32)
    S = x.shape[0]
    up = np.stack([oracle.resample(x[s], rate / 48000.0)[:, 0] for s in range(S)])
    T = up.shape[1] // 480
    for s, (n0, f) in (restart or {}).items():
        xz = x[s].copy()
        xz[:n0] = 0.0
        up[s, f * 480:] = oracle.resample(xz, rate / 48000.0)[f * 480:, 0]
    frames = np.ascontiguousarray(up[:, :T * 480].reshape(S, T, 480))
    bd = nn.BatchDenoiser(S, lib=lib)
    out48, vad = np.zeros((S, T, 480), np.float32), np.zeros((T, S), np.float32)
    cuts = sorted({0, T} | {f for f, _, _ in events})
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        for f, what, streams in events:
            if f == lo:
                {"reset": bd.reset_streams, "hold": bd.hold_streams, "resume": bd.resume_streams}[what](streams)
        o, v = bd.process(frames[:, lo:hi])
        out48[:, lo:hi], vad[lo:hi] = o, v
    bd.close()
    out48 = out48.reshape(S, T * 480)
    for s, (_, f) in (restart or {}).items():
        out48[s, :f * 480] = 0.0
    want = np.stack([oracle.resample(out48[s], 48000.0 / rate)[:, 0] for s in range(S)])
    return want, vad, up.shape[1]


def run_adapter(lib, x, rate, cuts, before=None, max_in=None):
    """x [S, n] (float32 or int16) through a fresh batch and adapter in calls of the given sizes (the rest in a last call), into buffers
    pre-filled with the sentinel.  before = {call index: fn(batch, adapter)} runs ahead of that call.  Returns a dict: out [S, n_out]
    and vad [T, S] concatenated, per call n_out / n_frames / carried, the adapter's table counts after every call."""
    import nnnoiseless_amd as nn
    from nnnoiseless_amd.pcm import RateAdapter
    S, n = x.shape
    sizes = list(cuts) + [n - sum(cuts)]
    bd = nn.BatchDenoiser(S, lib=lib)
    ra = RateAdapter(bd, rate, max_in or max(max(sizes), 1))
    sent = SENT.astype(x.dtype) if x.dtype == np.float32 else np.int16(-12345)
    outs, vads, r = [], [], {"n_out": [], "n_frames": [], "carried": [], "tables": []}
    pos = 0
    for k, c in enumerate(sizes):
        if before and k in before:
            before[k](bd, ra)
        o = np.full((S, ra.max_output(c)), sent, x.dtype)
        v = np.full((ra.max_frames(c), S), SENT, np.float32)
        y, vd = ra.process(x[:, pos:pos + c], out=o, vad=v)
        pos += c
        outs.append(y.copy())
        vads.append(vd.copy())
        r["n_out"].append(y.shape[1])
        r["n_frames"].append(vd.shape[0])
        r["carried"].append(ra.carried())
        r["tables"].append(ra.tables_built()[0])
    r["out"], r["vad"] = np.concatenate(outs, axis=1), np.concatenate(vads, axis=0)
    ra.close()
    bd.close()
    return r


def to_i16(y):
    """round half away from zero in float64, then the clamp: what the CLI's writers do to a float sample."""
    y = np.asarray(y, np.float64)
    return np.clip(np.sign(y) * np.floor(np.abs(y) + 0.5), -32768, 32767).astype(np.int16)


# ---- the cases both test files run ---------------------------------------------------------------------------------------------------
def check_composition(lib, oracle, S, n, rate, cuts):
    x = signal(S, n, rate, seed=int(rate))
    want, vad, n_up = yardstick(lib, oracle, x, rate)
    r = run_adapter(lib, x, rate, cuts)
    assert r["out"].shape == want.shape, (rate, r["out"].shape, want.shape)
    assert np.array_equal(bits(r["out"]), bits(want)), (rate, np.abs(r["out"] - want).max())
    assert r["vad"].shape == vad.shape and np.array_equal(bits(r["vad"]), bits(vad)), rate
    assert r["carried"][-1] == n_up - 480 * vad.shape[0]
    return r, want, vad


def check_int16(lib, S, n, rate, cuts):
    x = signal(S, n, rate, seed=3, loud=(0,))
    xi = to_i16(x)
    rf = run_adapter(lib, xi.astype(np.float32), rate, cuts)
    ri = run_adapter(lib, xi, rate, cuts)
    assert ri["out"].dtype == np.int16 and ri["out"].shape == rf["out"].shape
    assert np.abs(rf["out"][0]).max() > 32768.0, "the loud stream must reach the clamp"
    assert np.array_equal(ri["out"], to_i16(rf["out"]))
    assert np.array_equal(bits(ri["vad"]), bits(rf["vad"]))


def check_reset(lib, oracle, S, ticks, k, stream=1):
    """16 kHz, 160-sample ticks: after tick k - 1 (k ticks done) `stream` is reset in the adapter and in the batch."""
    rate, tick = 16000.0, 160
    x = signal(S, ticks * tick, rate, seed=7)
    plain, vad_plain, _ = yardstick(lib, oracle, x, rate)
    want, vad, _ = yardstick(lib, oracle, x, rate, restart={stream: (tick * k, k)}, events=[(k, "reset", [stream])])

    def reset(bd, ra):
        ra.reset_streams([stream])
        bd.reset_streams([stream])
    r = run_adapter(lib, x, rate, [tick] * (ticks - 1), before={k: reset})
    assert r["n_frames"] == [1] * ticks   # a tick completes a frame: frame k is the first one behind the reset
    off = sum(r["n_out"][:k])
    others = [s for s in range(S) if s != stream]
    assert r["out"].shape == plain.shape
    assert np.array_equal(bits(r["out"][others]), bits(plain[others])) and np.array_equal(bits(r["vad"][:, others]), bits(vad_plain[:, others]))
    assert np.array_equal(bits(r["out"][stream, :off]), bits(plain[stream, :off]))
    assert np.array_equal(bits(r["out"][stream, off:]), bits(want[stream, off:]))
    assert np.array_equal(bits(r["vad"][k:, stream]), bits(vad[k:, stream]))
    assert not np.array_equal(bits(want[stream, off:]), bits(plain[stream, off:]))   # (the reset is visible at all)


def check_hold(lib, oracle, S, ticks, k, stream=2, rate=16000.0, tick=160):
    """`stream` held in the batch for ticks k and k + 1, then resumed: the held calls leave its rows alone, and from tick k + 2 on it is the
    yardstick's stream whose earlier source samples were zero and whose batch slot was held over the same frames."""
    x = signal(S, ticks * tick, rate, seed=9)
    plain, vad_plain, _ = yardstick(lib, oracle, x, rate)
    r = run_adapter(lib, x, rate, [tick] * (ticks - 1), before={k: lambda bd, ra: bd.hold_streams([stream]), k + 2: lambda bd, ra: bd.resume_streams([stream])})
    others = [s for s in range(S) if s != stream]
    assert r["out"].shape == plain.shape
    assert np.array_equal(bits(r["out"][others]), bits(plain[others])) and np.array_equal(bits(r["vad"][:, others]), bits(vad_plain[:, others]))
    o0, o1, o2 = sum(r["n_out"][:k]), sum(r["n_out"][:k + 2]), r["out"].shape[1]
    f0, f1 = sum(r["n_frames"][:k]), sum(r["n_frames"][:k + 2])
    assert o1 > o0 and f1 > f0
    assert (r["out"][stream, o0:o1] == SENT).all() and (r["vad"][f0:f1, stream] == SENT).all()
    assert np.array_equal(bits(r["out"][stream, :o0]), bits(plain[stream, :o0]))
    want, vad, _ = yardstick(lib, oracle, x, rate, restart={stream: (tick * (k + 2), f1)}, events=[(f0, "hold", [stream]), (f1, "resume", [stream])])
    assert np.array_equal(bits(r["out"][stream, o1:o2]), bits(want[stream, o1:o2]))
    assert np.array_equal(bits(r["vad"][f1:, stream]), bits(vad[f1:, stream]))
    return r, plain
