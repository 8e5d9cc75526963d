"""Edge-case inputs for parity tests: each exercises a branch the synthetic sine+noise mix rarely reaches."""
import numpy as np


def make_edge_streams(n_frames):
    n = n_frames * 480
    t = np.arange(n)
    rng = np.random.default_rng(12345)
    s = []
    s.append(np.where((t // 55) % 2 == 0, 32767.0, -32768.0))                 # full-scale square wave (i16 limits)
    s.append(np.full(n, 10000.0))                                             # DC: the high-pass must kill it
    imp = np.zeros(n); imp[::4801] = 30000.0; s.append(imp)                    # sparse impulses
    s.append(rng.integers(-1, 2, n).astype(np.float64))                       # +-1 LSB noise: energies near the >= 1 clamps
    burst = np.zeros(n); on = (t // 2400) % 2 == 1                            # silence / tone bursts: onsets, e < 0.04 gate toggling
    burst[on] = 8000.0 * np.sin(2 * np.pi * 220.0 * t[on] / 48000.0); s.append(burst)
    s.append(12000.0 * np.sin(2 * np.pi * 48000.0 / 61.0 * t / 48000.0))      # period ~61 samples: the PITCH_MIN_PERIOD floor
    s.append(9000.0 * np.sin(2 * np.pi * 63.0 * t / 48000.0))                 # period ~762: the PITCH_MAX_PERIOD end
    sweep = 6000.0 * np.sin(2 * np.pi * (100.0 + 900.0 * t / n) * t / 48000.0); s.append(sweep)  # chirp: pitch doubling logic
    s.append(np.clip(40000.0 * rng.standard_normal(n), -32768, 32767))        # clipped loud noise
    s.append(np.zeros(n))                                                     # (replaced below: the ultrasonic tone)
    s.append(3000.0 * np.sin(2 * np.pi * 300.0 * t / 48000.0) + 8000.0 * np.sin(2 * np.pi * 22000.0 * t / 48000.0))   # voiced, with content above bin 400 (zero gain there)
    s.append(np.zeros(n))                                                     # digital silence
    x = np.round(np.stack(s)).astype(np.float32)
    # bin 450 alone, NOT rounded to integers (rounding noise would fill the bands): "silent" by the band energies, which end at bin
    # 399, and therefore synthesised as it came -- the only way bins 400 .. 480 reach the output
    x[-3] = (5000.0 * np.sin(2 * np.pi * 22500.0 * t / 48000.0)).astype(np.float32)
    return x.reshape(len(s), n_frames, 480)


def oracle_reference(oracle_mod, weights_bytes, x, margin=2e-3):
    """Oracle outputs plus a per-(stream, frame) mask of frames on which the REFERENCE itself is ill-conditioned.

    pitch_filter (ref: src/denoise.rs:365-402) picks r = 1 when exp > g and the closed form otherwise; when both
    are ~1 (a pure tone the network passes unattenuated) the closed form gives r ~ 0, so the branch is a jump
    discontinuity and f32 rounding noise in the FFT decides which side a frame lands on: the oracle's own f32-FFT
    and f64-FFT builds disagree by >1e-2 of full scale there.  Such a frame (and the next one, through the
    overlap-add memory) is excused from the AUDIO comparison only; pitch, vad and gains are still checked.
    """
    n_s, n_f = x.shape[:2]
    out = np.empty_like(x)
    vad = np.empty((n_s, n_f), np.float32)
    pitch = np.empty((n_s, n_f), np.int32)
    gains = np.empty((n_s, n_f, 22), np.float32)
    ill = np.zeros((n_s, n_f), bool)
    model = oracle_mod.Model(weights_bytes)
    for s in range(n_s):
        st = oracle_mod.State(model)
        for t in range(n_f):
            out[s, t], vad[s, t] = st.process_frame(x[s, t])
            tp = st.taps()
            pitch[s, t] = tp["pitch_idx"]
            gains[s, t] = tp["g"]
            e, g = tp["exp_"].astype(np.float64), tp["g"].astype(np.float64)
            jump = 1.0 - e * e * (1.0 - g * g) / (0.001 + g * g * (1.0 - e * e))   # 1 - closed form, at the branch point
            if not tp["silence"] and np.any((np.abs(e - g) < margin) & (jump > 0.01)):
                ill[s, t] = True
                if t + 1 < n_f:
                    ill[s, t + 1] = True
    return {"out": out, "vad": vad, "pitch": pitch, "g": gains, "ill": ill}


# Per-stream exponents of the advisor's case below: the stream's x4 energy (the coarse search's |x4|^2, the newest 240 values of the
# 4x-decimated buffer) lands in [2^-60, 2^-58] on the second loud frame, just above the quiet guard of the certified search
# (measured with the oracle's x_lp tap; test_hostsim_scale.py checks that it still does).  Stream 7 of make_streams is silent.
ADVISOR_EXP = (-44, -45, -45, -43, -45, -45, -43, -44, -44, -44, -45, -43, -45, -44, -42, -45)
# The scales of make_scale_streams, one aligned 16-stream block each: subnormal inputs, the 2^-120 block-energy floor, the quiet guard
# crossing, unit-range floats, int16 range, the loud guard crossing, and the overflow range (some energies inf, then all of them).
SCALE_EXP = (-140, -130, -126, -64, -40) + tuple(range(-34, -25)) + (-15, 0, 1, 2, 3, 4, 5, 6, 7, 8, 17, 24, 40, 50, 56, 58, 60, 62)


def make_scale_streams(n_frames, switch=None, scales=SCALE_EXP):
    """The 16 streams of make_streams(0, 16, T) scaled by exact powers of two, laid out as aligned 16-stream blocks (the certified pitch
    search decides per block: one extreme stream sends its 15 neighbours to the full search), one kind per block.

    Returns (x [S, T, 480] float32, exp [S] int: the exponent of the stream's first frame, names [S // 16]: what each block holds).
    Blocks: one per exponent of `scales` ("2^k"); then transitions at frame `switch` ("2^-110>0", "2^-130>0": quiet first, then int16 scale;
    "0>2^-110", "0>2^-130": the reverse); "advisor": a past at 2^-116 under an x4 just above the 2^-60 guard (ADVISOR_EXP from frame
    `switch` on); "sub0": subnormal samples (2^-140) interleaved with zeros; "mixed": the 2^0 block with its stream 5 at 2^60."""
    switch = max(3, n_frames // 2) if switch is None else switch
    assert 2 <= switch <= n_frames - 2, "the advisor's case needs two quiet frames and two loud ones"
    from nnnoiseless_amd.synthetic import make_streams
    base = make_streams(0, 16, n_frames).astype(np.float64)
    blocks, exps, names = [], [], []

    def add(name, v, e):
        blocks.append(v)
        exps.append(np.broadcast_to(np.asarray(e, np.int64), (16,)))
        names.append(name)

    for k in scales:
        add(f"2^{k}", base * 2.0 ** k, k)
    for q in (-110, -130):
        v = base.copy()
        v[:, :switch] *= 2.0 ** q
        add(f"2^{q}>0", v, q)
        v = base.copy()
        v[:, switch:] *= 2.0 ** q
        add(f"0>2^{q}", v, 0)
    v = base.copy()
    v[:, :switch] *= 2.0 ** -116
    v[:, switch:] *= (2.0 ** np.array(ADVISOR_EXP, np.float64))[:, None, None]
    add("advisor", v, -116)
    v = base * 2.0 ** -140
    v[..., 1::2] = 0.0
    add("sub0", v, -140)
    v = base.copy()
    v[5] *= 2.0 ** 60
    e = np.zeros(16, np.int64)
    e[5] = 60
    add("mixed", v, e)
    x = np.concatenate(blocks).astype(np.float32)   # exact: integers times powers of two, at worst on the subnormal grid of 2^-149
    return x, np.concatenate(exps), names


def _per_stream_max(a):
    """max over every axis but the first, NaN and infinities left out (0 where nothing is finite)."""
    a = np.where(np.isfinite(a), a, 0.0)
    return a.reshape(a.shape[0], -1).max(axis=1)


def _same_nonfinite(got, want, what):
    for f in (np.isnan, np.isposinf, np.isneginf):
        assert np.array_equal(f(got), f(want)), (what, f.__name__, np.argwhere(f(got) != f(want))[:8])


def diverged_frames(ref, ref32, thr=1e-4):
    """[S, T] bool: the frames on which the reference's own arithmetic cannot meet the gain bar, measured, not assumed -- per aligned
    16-stream block (one kind of input at one scale), every frame from the first one on which the oracle's f32-FFT and f64-FFT builds put
    some gain of some stream of the block more than `thr` (the gain bar, 1e-4) apart: the GRU state carries that rounding on.  (On the
    48-frame sweep: 2^40 and 2^50 from frame 8, on to gains 1.0 apart; 2^24 from frame 12; the loud-to-quiet switches and 2^6 on their
    last frames; 2^17 nowhere.)"""
    d = np.abs(ref["gains"].astype(np.float64) - ref32["gains"].astype(np.float64))
    d = np.where(np.isfinite(d), d, 0.0).max(axis=2)
    S, T = d.shape
    blk = d.reshape(S // 16, 16, T).max(axis=1) > thr
    return np.repeat(np.logical_or.accumulate(blk, axis=1), 16, axis=0)


def check_scale_outputs(out, vad, gains, pitch, branch, ref, ref32, excused_max=0.05, diverged=None):
    """The bars of the scale sweep against the oracle's f64-FFT (`ref`) and f32-FFT (`ref32`) builds (run_streams with "out", "pitch",
    "branch", "vad", "gains").  out [S, T, 480], vad [S, T], gains [S, T, 22], pitch / branch [S, T].
    Pitch index exact on every frame.  Non-finite values (NaN, +inf, -inf) where the oracle has them and nowhere else, on every frame.
    `diverged` [S, T] (diverged_frames): frames on which the oracle's two builds are themselves far apart; they are left out of the
    three bars below, and of the spreads those bars are scaled by.
    VAD and gains per stream within max(1e-4, 3 x the stream's |ref32 - ref|) for all but 2 % of the streams.  Those few are held
    only to max(1e-3, 20 x the spread): where the spread is small the 1e-3 floor is what binds, which is looser than
    test_edge_case_inputs.  The reason is that the oracle's two builds share everything after the FFT, so their spread does not sample
    a different f32 rounding of log10 and of the DCT of the band energies.  At 2^50 the f32 build's FFT differences vanish below an ulp
    of log10(E) ~ 35, its gains equal the f64 build's to the bit for the first frames, and the kernels' own rounding of the same
    features (one ulp apart) is "beyond" a spread near 0.  After a loud-to-quiet switch the pitch-correlation features of bands holding
    the high-pass filter's decaying memory are ill-conditioned, as in check_rows.
    Audio on the frames whose branch mask agrees with the oracle's (and the frame after each flip): |out - ref| <= 1e-4 x the stream's
    peak + 3 |ref32 - ref| + 4 x 2^-149, the excused frames under `excused_max` of all.
    Returns (excused mask [S, T], list of flips) for the caller's report."""
    from test_gpu_parity import flipped_frames
    assert np.array_equal(pitch, ref["pitch"]), np.argwhere(pitch != ref["pitch"])[:8]
    live = np.ones(pitch.shape, bool) if diverged is None else ~diverged
    for name, got in (("vad", vad), ("gains", gains)):
        want, w32 = ref[name].astype(np.float64), ref32[name].astype(np.float64)
        _same_nonfinite(got, ref[name], name)
        m = live if got.ndim == 2 else live[..., None]
        spread = _per_stream_max(np.where(m, np.abs(w32 - want), 0.0))
        err = _per_stream_max(np.where(m, np.abs(got - want), 0.0))
        over = np.argwhere(err > np.maximum(1e-4, 3.0 * spread)).ravel()
        print(f"{name}: worst error {err.max():.2e}; streams beyond max(1e-4, 3 x spread): {[(int(s), float(err[s]), float(spread[s])) for s in over]}")
        assert len(over) <= max(1, len(err) // 50), (name, over, err[over], spread[over])
        assert (err <= np.maximum(1e-3, 20.0 * spread)).all(), (name, over, err[over], spread[over])
    _same_nonfinite(out, ref["out"], "out")
    excused, flips = flipped_frames(branch, ref["branch"])
    want = ref["out"].astype(np.float64)
    spread = np.abs(ref32["out"].astype(np.float64) - want)
    spread = np.where(np.isfinite(spread), spread, np.inf)   # (the f32 build overflows where the checker does not: its arithmetic excuses it)
    peak = _per_stream_max(np.abs(want))[:, None, None]
    bound = 1e-4 * peak + 3.0 * spread + 4.0 * 2.0 ** -149
    ok = np.isfinite(want) & ~excused[..., None] & live[..., None]
    err = np.where(ok, np.abs(out - np.where(ok, want, 0.0)), 0.0)
    bad = np.argwhere(err > bound)
    assert not len(bad), (len(bad), bad[:8], err[tuple(bad[0])], bound[tuple(bad[0])])
    assert excused[live].mean() < excused_max, (excused[live].mean(), flips[:16])
    return excused, flips
