"""Parity across the f32 amplitude range, subnormal to overflow, on the MI355X: the streams of edge_streams.make_scale_streams (every
scale of SCALE_EXP, one per aligned 16-stream block, transitions, a mixed block) for 48 frames.  What the interpreter cannot say
(tests/test_hostsim_scale.py runs the same checks there): what the matrix cores do with subnormal bf16 operands, v_sqrt_f32 / v_rsq_f32
on tiny arguments, and the compiled f32 code on subnormal spectra.  The certified search against the oracle on every frame, the
production bits of every way of running a frame, the audio / VAD / gains bars against the oracle, export and import, training rows."""
import os

import numpy as np
import pytest

from edge_streams import SCALE_EXP, check_scale_outputs, diverged_frames, make_scale_streams
from test_hostsim_scale import _bits, _block, check_crossings, oracle_lags, regimes
from test_pitch_certified import _run

pytestmark = pytest.mark.gpu

T, SWITCH, C = 48, 24, 24
WANT = ("out", "pitch", "branch", "vad", "gains")
N_THREADS = min(16, os.cpu_count() or 1)   # (a command gets 16 CPUs of the machine it runs on)


@pytest.fixture(scope="module")
def sweep(oracle_mod, weights_bytes):
    x, exp, names = make_scale_streams(T, SWITCH)
    ref = oracle_mod.run_streams(oracle_mod.Model(weights_bytes), x, n_threads=N_THREADS, want=WANT)
    ref32 = oracle_mod.run_streams(oracle_mod.Model(weights_bytes, f32_fft=True), x, n_threads=N_THREADS, want=WANT)
    return x, exp, names, ref, ref32


def _calls(bd, x, chunks):
    outs, vads, t = [], [], 0
    for n in chunks:
        o, v = bd.process(x[:, t:t + n])
        outs.append(o)
        vads.append(v)
        t += n
    assert t == x.shape[1] and not bd.fault()
    return np.concatenate(outs, 1), np.concatenate(vads, 0).T


@pytest.fixture(scope="module")
def production(sweep):
    """The default batch in 24-frame calls: the bits every other way of running the sweep must give."""
    import nnnoiseless_amd as nn
    x = sweep[0]
    bd = nn.BatchDenoiser(x.shape[0])
    out, vad = _calls(bd, x, (C,) * (T // C))
    bd.close()
    return out, vad


@pytest.fixture(scope="module")
def one_frame_run(sweep):
    """One-frame calls (the tick path through k_back), with every frame's taps."""
    import nnnoiseless_amd as nn
    x = sweep[0]
    S = x.shape[0]
    bd = nn.BatchDenoiser(S)
    out, vad = np.empty_like(x), np.empty((S, T), np.float32)
    gains, pitch, branch = np.empty((S, T, 22), np.float32), np.empty((S, T), np.int32), np.empty((S, T), np.int32)
    for t in range(T):
        o, v = bd.process(x[:, t:t + 1])
        out[:, t], vad[:, t] = o[:, 0], v[0]
        gains[:, t], pitch[:, t], branch[:, t] = bd.tap("g"), bd.tap("pitch")[:, 0], bd.tap("branch")[:, 0]
    assert not bd.fault()
    bd.close()
    return out, vad, gains, pitch, branch


def test_certified_search_across_scales_gpu(oracle_mod, weights_bytes, sweep):
    """set_taps(2): the pair, every survivor's sum and the pitch index as the oracle's on every frame of every scale, both regimes with
    their crossings bracketed by adjacent scales of the grid, the mixed block on the full search."""
    import nnnoiseless_amd as nn
    x, exp, names, _, _ = sweep
    counts = _run(nn, oracle_mod, weights_bytes, x)
    lags = oracle_lags(oracle_mod, weights_bytes, x)
    reg = regimes(counts, lags, names, SCALE_EXP)
    print("certified search by scale:", reg)
    assert reg[0] == "cert" and reg[-15] == "cert", reg
    assert reg[-40] == "full" and reg[17] == "full", reg
    quiet, loud = check_crossings(reg)
    print("crossings: full at 2^%d, certified from 2^%d to 2^%d, full from 2^%d" % (quiet + loud))
    b = _block(names, "mixed")
    assert (counts[b] == lags[b]).all()
    for name in ("advisor", "sub0", "2^-110>0", "0>2^-110", "2^-130>0", "0>2^-130"):
        b = _block(names, name)
        print(f"{name}: full search on {int((counts[b] == lags[b]).all(axis=0).sum())} of {T} frames")


def test_outputs_against_the_oracle_gpu(sweep, one_frame_run, production):
    """Pitch exact, VAD and gains within the oracle's own f32 / f64 spread, audio within 1e-4 of the stream's peak on unflipped frames,
    non-finite values where the oracle has them; the one-frame calls give the bits of the 24-frame calls; the mixed block's 15 int16
    streams are those of the homogeneous block."""
    from conftest import flip_stats
    x, exp, names, ref, ref32 = sweep
    out, vad, gains, pitch, branch = one_frame_run
    # The bars hold on every stream and frame except where the oracle's own f32-FFT and f64-FFT builds are measured to be further apart
    # than the gain bar (diverged_frames; the GRU state of the loud blocks carries the FFTs' rounding on, to gains 1.0 apart at 2^40 and
    # 2^50): those frames keep the exact checks (pitch, non-finite positions, the bits of every way of running a frame).
    div = diverged_frames(ref, ref32)
    print("frames left to the exact checks, by block:", {n: int(div[16 * i].sum()) for i, n in enumerate(names) if div[16 * i].any()})
    assert div.mean() < 0.1, div.mean()   # (measured 8.8 %)
    excused, flips = check_scale_outputs(out, vad, gains, pitch, branch, ref, ref32, diverged=div)
    fin = np.isfinite(ref["out"]).all(axis=(1, 2))
    print("flipped (stream, frame, bands):", flips)
    fin &= ~div.any(axis=1)
    print("flips:", flip_stats(branch[fin], out[fin], {k: ref[k][fin] for k in ("branch", "out")}, {k: ref32[k][fin] for k in ("branch", "out")}))
    assert np.array_equal(_bits(out), _bits(production[0])) and np.array_equal(_bits(vad), _bits(production[1]))
    m, h = _block(names, "mixed"), _block(names, "2^0")
    keep = [s for s in range(16) if s != 5]
    assert np.array_equal(_bits(out[m][keep]), _bits(out[h][keep])) and np.array_equal(_bits(vad[m][keep]), _bits(vad[h][keep]))


@pytest.mark.parametrize("way", ["back_end_0", "back_end_2", "max_group_frames_1", "full_search", "tiled_4096"])
def test_every_way_of_running_a_frame_gives_the_same_bits(sweep, production, way):
    import nnnoiseless_amd as nn
    x = sweep[0]
    S = x.shape[0]
    want_out, want_vad = production
    if way == "tiled_4096":
        reps = -(-4096 // S)
        xt = np.tile(x, (reps, 1, 1))[:4096]
        bd = nn.BatchDenoiser(4096)
        out, vad = _calls(bd, xt, (C,) * (T // C))
        bd.close()
        for r in range(reps):
            n = min(S, 4096 - r * S)
            assert np.array_equal(_bits(out[r * S:r * S + n]), _bits(want_out[:n])), r
            assert np.array_equal(_bits(vad[r * S:r * S + n]), _bits(want_vad[:n])), r
        return
    bd = nn.BatchDenoiser(S, max_group_frames=1 if way == "max_group_frames_1" else None)
    chunks = (C,) * (T // C)
    if way.startswith("back_end"):
        bd.set_back_end(int(way[-1]))
        chunks = (1, 1, 22, 24)
    elif way == "full_search":
        bd.set_taps(1)
        chunks = (1,) * T
    out, vad = _calls(bd, x, chunks)
    bd.close()
    assert np.array_equal(_bits(out), _bits(want_out)), np.argwhere(_bits(out) != _bits(want_out))[:8]
    assert np.array_equal(_bits(vad), _bits(want_vad))


def test_export_import_at_scale_gpu(sweep, production):
    """Streams exported after SWITCH frames and imported into a batch of another size, group length and block layout continue bit for
    bit (import rebuilds the decimated ring, x_lp[0] and the filtered sample)."""
    import nnnoiseless_amd as nn
    x, exp, names, _, _ = sweep
    out, vad = production
    src = np.concatenate([np.arange(b.start, b.stop) for b in (_block(names, n) for n in ("2^-140", "2^-15", "2^40", "2^60", "sub0", "advisor"))])
    a = nn.BatchDenoiser(len(src))
    _calls(a, x[src, :SWITCH], (SWITCH,))
    rec = a.export_streams(range(len(src)))
    a.close()
    S2 = len(src) + 37
    dst = np.random.default_rng(7).permutation(S2)[:len(src)]
    b = nn.BatchDenoiser(S2, max_group_frames=3)
    b.process(np.zeros((S2, 2, 480), np.float32))
    b.import_streams(dst, rec)
    y = np.zeros((S2, T - SWITCH, 480), np.float32)
    y[dst] = x[src, SWITCH:]
    o, v = _calls(b, y, (5, 1, T - SWITCH - 6))
    b.close()
    assert np.array_equal(_bits(o[dst]), _bits(out[src, SWITCH:])), np.argwhere(_bits(o[dst]) != _bits(out[src, SWITCH:]))[:8]
    assert np.array_equal(_bits(v[dst]), _bits(vad[src, SWITCH:]))


@pytest.mark.parametrize("k", [-140, -15, 0, 40])
def test_training_rows_at_scale(oracle_mod, weights_bytes, k):
    """k_features / k_train_rows on (clean, noise, mix) triples scaled by 2^k against the oracle's rows, under test_training_rows' bars.
    At 2^40 the oracle's own f32-FFT and f64-FFT builds are further apart than check_rows' absolute bars (4.9e-4 on feature 41, which
    reaches ~2000; 0.017 on a gain, 0.96 on a log level): there the features are judged against 3 x that spread column by column, the gains and
    log levels as the pitch-correlation features are (check_rows)."""
    from nnnoiseless_amd.training import TrainingFeatures
    from train_fixtures import check_rows, make_training_inputs
    sig, noise, comb, cutoff, vad = make_training_inputs(9, 256, 30)
    f = 2.0 ** k
    sig, noise, comb = ((a.astype(np.float64) * f).astype(np.float32) for a in (sig, noise, comb))
    ref = oracle_mod.training_rows(oracle_mod.Model(weights_bytes), sig, noise, comb, cutoff, vad, n_threads=N_THREADS)
    ref32 = oracle_mod.training_rows(oracle_mod.Model(weights_bytes, f32_fft=True), sig, noise, comb, cutoff, vad, n_threads=N_THREADS)
    rows = TrainingFeatures(256).process(sig, noise, comb, cutoff, vad)
    check_rows(rows, ref, ref32, feature_spread=k > 8)
