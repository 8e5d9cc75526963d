"""The two host policies of the training-data generator and its main loop (nnnoiseless_amd/training.py): pure
Python, no device -- random_params against the ranges of randomize() (src/training.rs:341-365), ClipCursor against a plain-Python
SignalReader (:171-261) walked reader by reader, generate_rows' call cutting with a stub simulator, and the command-line front-end on
three tiny WAVs (that one test runs on the interpreter build)."""
import numpy as np
import pytest

from nnnoiseless_amd import training

FRAME = 480


def test_random_params_ranges():
    n = 20000
    p = training.random_params(np.random.default_rng(3), n)
    assert p.dtype == training.SIM_PARAMS_DTYPE and p.shape == (n,)
    sg, ng = p["signal_gain"], p["noise_gain"]
    assert 0.07 < (sg == 0).mean() < 0.13                                   # gen_bool(0.1)
    db = 20 * np.log10(sg[sg > 0].astype(np.float64))
    assert np.abs(db - np.round(db)).max() < 1e-4 and set(np.round(db).astype(int)) == set(range(-40, 20))
    assert (ng > 0).all()                                                    # (it took signal_gain before that went to zero)
    ratio = 20 * np.log10(ng[sg > 0].astype(np.float64) / sg[sg > 0])
    assert np.abs(ratio - np.round(ratio)).max() < 1e-3 and set(np.round(ratio).astype(int)) == set(range(-20, 20))
    assert 10 ** (-60 / 20) * 0.999 <= ng.min() and ng.max() <= 10 ** (38 / 20) * 1.001
    for name in ("sig_a", "sig_b", "noise_a", "noise_b"):
        c = p[name]
        assert c.shape == (n, 2) and c.min() >= -0.375 and c.max() < 0.375 and c.min() < -0.37 and c.max() > 0.37
        assert abs(float(c.mean())) < 0.01
    assert set(p["band_lp"].tolist()) == set(range(12, 22))                  # lowpass >= 60 bins: band 12 (edge 64) is the lowest it reaches
    assert training.random_params(np.random.default_rng(3), 50).tobytes() == training.random_params(np.random.default_rng(3), 50).tobytes()


def test_band_lp_map():
    """Every lowpass the draw can give and beyond (481 x 3000 / 24000 x 50^U < 3007): the first band whose edge, in bins, lies above it."""
    edges = np.array(training.EBAND_5MS) << 2
    assert training.EBAND_5MS[-1] == 100 and len(training.EBAND_5MS) == 22
    for lowpass in range(0, 3008):
        want = int(np.searchsorted(edges, lowpass, side="right"))
        assert training.band_lp_for(lowpass) == (want if want < 22 else 21), lowpass
    assert training.band_lp_for(0) == 1 and training.band_lp_for(399) == 21 and training.band_lp_for(3) == 1 and training.band_lp_for(4) == 2


class PlainReader:
    """SignalReader (src/training.rs:171-261), one reader, frame by frame, over (start, length) clips; a clip without a whole frame
    is stepped over (the reference would spin on it)."""

    def __init__(self, starts, lengths, count, first, rng):
        self.starts, self.lengths, self.rng = starts, lengths, rng
        self.frames_per_file = max(count // len(starts) + 1, 100)
        self.cur_idx, self.frames_left, self.pos = first, 0, None

    def next_reader(self):
        if self.cur_idx >= len(self.starts):
            self.cur_idx = 0
        length = self.lengths[self.cur_idx]
        num_samples = FRAME * self.frames_per_file
        seek = 0
        if length > num_samples:
            seek = int(self.rng.integers(0, length - num_samples + 1))       # gen_range(0..=(len - num_samples))
            self.frames_left = self.frames_per_file
        else:
            self.frames_left = length // FRAME
        if self.frames_left > 0:
            self.pos = self.starts[self.cur_idx] + seek
        else:
            self.cur_idx += 1

    def frame(self):
        while self.pos is None:
            self.next_reader()
        off = self.pos
        self.pos += FRAME
        if self.frames_left <= 1:
            self.pos = None
            self.cur_idx += 1
        else:
            self.frames_left -= 1
        return off


def test_clip_cursor_against_a_plain_reader():
    lengths = [FRAME * 3 + 17, 100, FRAME * 150 + 3, FRAME, FRAME * 100, FRAME * 100 + 1, 479, FRAME * 7 + 479]
    starts = list(np.concatenate([[5], 5 + np.cumsum(lengths)[:-1] + 11 * np.arange(1, len(lengths))]))   # (gaps between the clips)
    S, count, T = 5, 640, 700
    cur = training.ClipCursor(starts, lengths, count, S, np.random.default_rng(7))
    assert cur.frames_per_file == 100
    got = np.concatenate([cur.next(n) for n in (1, 24, 24, 3, 648)])
    assert got.shape == (T, S) and got.dtype == np.uint64
    seeds = np.random.default_rng(7).integers(0, 2 ** 63, S)
    for s in range(S):
        r = PlainReader(starts, lengths, count, (s * len(lengths)) // S, np.random.default_rng(int(seeds[s])))
        want = [r.frame() for _ in range(T)]
        assert list(got[:, s].astype(np.int64)) == want, s
    # every frame lies inside ONE clip; the short clips (1 and 6) give nothing; the readers cycle through the list
    ends = np.array(starts) + np.array(lengths)
    clip = np.searchsorted(np.array(starts), got.astype(np.int64), side="right") - 1
    assert (got.astype(np.int64) + FRAME <= ends[clip]).all()
    assert not np.isin(clip, (1, 6)).any() and set(np.unique(clip)) == {0, 2, 3, 4, 5, 7}
    assert [int(c) for c in clip[:4, 0]] == [0, 0, 0, 2]                     # three whole frames of clip 0, then on (clip 1 skipped)
    first = clip[:, 0]
    assert (np.diff(np.flatnonzero(first == 0)) > 1).any()                   # reader 0 comes back to clip 0: the list is cyclic
    # the long clips give a slice of exactly frames_per_file frames, not from the start every time; clip 4 (exactly that long) gives itself
    run = got[clip[:, 0] == 2, 0].astype(np.int64)
    assert (np.diff(run[:100]) == FRAME).all() and run[0] - starts[2] <= lengths[2] - 100 * FRAME
    assert len({int(got[t, s]) for s in range(S) for t in range(T) if clip[t, s] == 2 and (t == 0 or clip[t - 1, s] != 2)}) > 1
    run4 = got[clip[:, 0] == 4, 0].astype(np.int64)
    assert run4[0] == starts[4] and (np.diff(run4[:100]) == FRAME).all()
    assert training.ClipCursor(starts, lengths, 8 * 1000, S, np.random.default_rng(1)).frames_per_file == 1001   # the TOTAL count
    with pytest.raises(ValueError):
        training.ClipCursor([0, 10], [100, 479], 10, 2, np.random.default_rng(1))
    with pytest.raises(ValueError):
        training.ClipCursor([], [], 10, 2, np.random.default_rng(1))


class StubSimulator:
    def __init__(self):
        self.log, self.frames = [], 0

    def load_signal(self, a):
        self.log.append(("signal", a.size))

    def load_noise(self, a):
        self.log.append(("noise", a.size))

    def set_params(self, idx, recs):
        assert idx is None and recs.shape == (2,) and recs.dtype == training.SIM_PARAMS_DTYPE
        self.log.append(("params", self.frames))

    def process(self, sig_off, noise_off, rows):
        assert sig_off.shape == noise_off.shape == rows.shape[:2] and rows.shape[2] == 87
        assert int(sig_off.max()) + FRAME <= 3 * FRAME * 40 and int(noise_off.max()) + FRAME <= 2 * FRAME * 30 + 5
        rows[:] = self.frames + np.arange(rows.shape[0])[:, None, None]
        self.log.append(("process", self.frames, rows.shape[0]))
        self.frames += rows.shape[0]


def test_generate_rows_cuts_calls_where_the_gains_change():
    """Creation parameters for the first 2821 frames, randomize() before frame 2822 and every 2822 frames from there (src/training.rs:388-393);
    no call crosses such a frame or has more than 24."""
    sig = [np.zeros(FRAME * 40, np.int16)] * 3
    noise = [np.ones(FRAME * 30, np.int16), np.ones(FRAME * 30 + 5, np.int16)]
    per_stream = 2821 + 2822 + 30
    stub = StubSimulator()
    rows = training.generate_rows(sig, noise, 2 * per_stream - 1, 2, seed=4, simulator=stub)
    assert rows.shape == (per_stream, 2, 87) and np.array_equal(rows[:, 0, 0], np.arange(per_stream))
    assert stub.log[:2] == [("signal", 3 * FRAME * 40), ("noise", 2 * FRAME * 30 + 5)]
    assert [e[1] for e in stub.log if e[0] == "params"] == [2821, 2821 + 2822]
    calls = [e for e in stub.log if e[0] == "process"]
    assert all(1 <= n <= training.GROUP_FRAMES for _, _, n in calls) and sum(n for _, _, n in calls) == per_stream
    for change in (2821, 2821 + 2822):
        assert any(t0 == change for _, t0, _ in calls) and not any(t0 < change < t0 + n for _, t0, n in calls)
        assert stub.log.index(("params", change)) + 1 == stub.log.index(next(e for e in calls if e[1] == change))
    assert training.call_cuts(30) == [(0, 24, False), (24, 6, False)]
    assert training.call_cuts(2822)[-2:] == [(2808, 13, False), (2821, 1, True)]
    assert training.GAIN_CHANGE_COUNT == 2821


def _wav(path, x, channels=1, rate=48000):
    import wave
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.ascontiguousarray(x, "<i2").tobytes())


def test_front_end(hostsim_lib, tmp_path, monkeypatch):
    """python -m nnnoiseless_amd.training on two clean clips and a noise clip the test writes: the .npy holds generate_rows' rows for the
    same clips and seed; a stereo clip and a 44.1 kHz clip are refused by name."""
    rng = np.random.default_rng(5)
    clips = {"s_a.wav": (3000 * np.sin(np.arange(FRAME * 3 + 9) * 0.05)).astype(np.int16),
             "s_b.wav": (800 * rng.standard_normal(FRAME * 2)).astype(np.int16),
             "n_a.wav": (200 * rng.standard_normal(FRAME * 4 + 1)).astype(np.int16)}
    for name, x in clips.items():
        _wav(tmp_path / name, x)
    monkeypatch.setattr(training, "library", lambda: hostsim_lib)
    out = tmp_path / "rows.npy"
    assert training.main(["--signal-glob", str(tmp_path / "s_*.wav"), "--noise-glob", str(tmp_path / "n_*.wav"), "--count", "5", "-o", str(out),
                          "--streams", "2", "--seed", "9"]) == 0
    rows = np.load(out)
    want = training.generate_rows([clips["s_a.wav"], clips["s_b.wav"]], [clips["n_a.wav"]], 5, 2, 9, lib=hostsim_lib)
    assert rows.shape == (3, 2, 87) and rows.dtype == np.float32 and np.array_equal(rows.view(np.uint32), want.view(np.uint32))
    assert np.isfinite(rows).all() and (rows[..., :42] != 0).any() and set(np.unique(rows[..., 86])) <= {0.0, 0.5, 1.0}
    _wav(tmp_path / "n_stereo.wav", np.zeros((FRAME, 2), np.int16), channels=2)
    with pytest.raises(SystemExit) as e:
        training.main(["--signal-glob", str(tmp_path / "s_*.wav"), "--noise-glob", str(tmp_path / "n_*.wav"), "--count", "5", "-o", str(out)])
    assert "n_stereo.wav" in str(e.value) and "unsupported wav format" in str(e.value)
    _wav(tmp_path / "s_c.wav", np.zeros(FRAME, np.int16), rate=44100)
    with pytest.raises(SystemExit) as e:
        training.main(["--signal-glob", str(tmp_path / "s_c.wav"), "--noise-glob", str(tmp_path / "n_a.wav"), "--count", "5", "-o", str(out)])
    assert "s_c.wav" in str(e.value)
    with pytest.raises(SystemExit):
        training.main(["--signal-glob", str(tmp_path / "nothing_*.wav"), "--noise-glob", str(tmp_path / "n_a.wav"), "--count", "5", "-o", str(out)])
