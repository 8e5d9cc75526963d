"""Batched training-feature rows: the per-frame body of the reference's training-data generator
(src/training.rs:113-160) for many (clean, noise, mix) stream triples at once, on the denoiser's own HIP kernels.

The simulator that feeds it (src/training.rs:263-422) runs on the device too: NoiseSimulator (include/nnn_sim.h) holds the clean
and the noise clips as two int16 arenas and makes the three signals, the energy-based VAD label and the band cutoff from
per-frame offsets, so only offsets go in and only rows come out.  What is policy rather than arithmetic stays on the host,
as plain Python without a device: the random gains and filters (random_params), the clip reader (ClipCursor) and the
generator's main loop over them (generate_rows; `python -m nnnoiseless_amd.training` is its front-end).
"""
import ctypes as C

import numpy as np

from . import FRAME_SIZE, NB_BANDS, NB_FEATURES, _ffi, library

ROW_WIDTH = NB_FEATURES + 2 * NB_BANDS + 1          # 87, src/training.rs:89
GAIN_CHANGE_COUNT = 2821                            # frames between two randomize() calls, src/training.rs
GROUP_FRAMES = 24                                   # max_group_frames of a training object: the frames one launch sequence covers
EBAND_5MS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24, 28, 34, 40, 48, 60, 78, 100)   # src/lib.rs:55-58
SIM_PARAMS_DTYPE = _ffi.SIM_PARAMS_DTYPE
ARENA_SIGNAL, ARENA_NOISE = 0, 1


class TrainingFeatures:
    """n_streams x (clean, noise, mix) DenoiseFeatures states."""

    def __init__(self, n_streams, device=0, lib=None):
        self._lib = lib or library()
        self.n_streams = int(n_streams)
        self._h = self._lib.L.nnn_train_create(self.n_streams, device)
        if not self._h:
            raise RuntimeError("nnnoiseless_amd: " + self._lib.error())

    def process(self, signal, noise, combined, band_gain_cutoff, vad, rows=None):
        """signal / noise / combined: float32 [n_streams, n_frames, 480] (i16 range); band_gain_cutoff int32 and vad
        float32 [n_frames, n_streams].  Returns rows float32 [n_frames, n_streams, 87]:
        42 features of the mix | 22 gains | 22 noise levels | vad.  Long calls cross the bus in 16-frame chunks beside the
        kernels; arrays from nnnoiseless_amd.pinned_empty (inputs, and `rows` handed in) go by DMA."""
        signal, noise, combined = (_ffi.as_f32(a) for a in (signal, noise, combined))
        if signal.ndim != 3 or signal.shape[0] != self.n_streams or signal.shape[2] != FRAME_SIZE or not (noise.shape == signal.shape == combined.shape):
            raise ValueError(f"process needs three arrays of shape [{self.n_streams}, n_frames, {FRAME_SIZE}]")
        S, T, F = signal.shape
        cut = np.ascontiguousarray(band_gain_cutoff, dtype=np.int32)
        vad = _ffi.as_f32(vad)
        if cut.shape != (T, S) or vad.shape != (T, S):
            raise ValueError("band_gain_cutoff and vad must have shape [n_frames, n_streams]")
        if rows is None:
            rows = np.empty((T, S, ROW_WIDTH), np.float32)
        # a caller-supplied row buffer is written by the C library: a wrong size or layout must never get that far
        if not (isinstance(rows, np.ndarray) and rows.shape == (T, S, ROW_WIDTH) and rows.dtype == np.float32 and rows.flags.c_contiguous and rows.flags.writeable):
            raise ValueError(f"rows must be a writable C-contiguous float32 array of shape [n_frames, n_streams, {ROW_WIDTH}]")
        self._lib.check(self._lib.L.nnn_train_process_host(self._h, _ffi.ptr(signal), _ffi.ptr(noise), _ffi.ptr(combined),
                                                           _ffi.ptr(cut), _ffi.ptr(vad), _ffi.ptr(rows), T))
        return rows

    def process_device(self, d_signal, d_noise, d_combined, d_cutoff, d_vad, d_rows, n_frames, stream_stride, frame_stride,
                       hip_stream=0):
        """Raw device pointers (include/nnn_train.h); asynchronous."""
        self._lib.check(self._lib.L.nnn_train_process_device(self._h, d_signal, d_noise, d_combined, d_cutoff, d_vad, d_rows,
                                                             n_frames, stream_stride, frame_stride, hip_stream))

    def reset(self):
        self._lib.check(self._lib.L.nnn_train_reset(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.L.nnn_train_destroy(self._h)
            self._h = None

    __del__ = close


def default_params(n):
    """n records of NoiseSimulator::new: gains 1, every filter coefficient 0, band_lp 21."""
    p = np.zeros(n, SIM_PARAMS_DTYPE)
    p["signal_gain"] = p["noise_gain"] = 1.0
    p["band_lp"] = NB_BANDS - 1
    return p


class NoiseSimulator:
    """n_streams NoiseSimulator instances (src/training.rs:263-422) on the device, beside a TrainingFeatures whose stream count it takes
    and whose rows it feeds (include/nnn_sim.h).  Offsets are uint64 [n_frames, n_streams]: the element of the signal / noise arena
    where that frame's 480 samples begin."""

    def __init__(self, features):
        self._features = features          # (borrowed by the C object: kept alive here)
        self._lib = features._lib
        if not hasattr(self._lib.L, "nnn_sim_create"):
            raise RuntimeError("nnnoiseless_amd: this build of the library has no noise simulator (nnn_sim_*)")
        self.n_streams = features.n_streams
        self._h = self._lib.L.nnn_sim_create(features._h)
        if not self._h:
            raise RuntimeError("nnnoiseless_amd: " + self._lib.error())
        self._adopted = {}

    def _load(self, which, pcm):
        a = np.ascontiguousarray(pcm)
        if a.dtype != np.int16 or a.ndim != 1:
            raise ValueError("an arena is a one-dimensional int16 array (48 kHz mono clips, one after the other)")
        self._lib.check(self._lib.L.nnn_sim_load(self._h, which, _ffi.ptr(a), a.size))
        self._adopted.pop(which, None)

    def load_signal(self, pcm):
        """Uploads the clean-speech arena (synchronous; the simulator owns the copy)."""
        self._load(ARENA_SIGNAL, pcm)

    def load_noise(self, pcm):
        self._load(ARENA_NOISE, pcm)

    def adopt_device(self, which, ptr, elems, keep=None):
        """Borrows a device buffer of int16 (a raw pointer, e.g. tensor.data_ptr()) as arena `which` (ARENA_SIGNAL / ARENA_NOISE);
        `keep`: an object to hold on to for as long as the arena is in use (the tensor)."""
        self._lib.check(self._lib.L.nnn_sim_adopt_device(self._h, which, ptr, elems))
        self._adopted[which] = keep

    def _idx(self, idx):
        if idx is None:
            return None, None, self.n_streams
        a, p = _ffi.stream_list(idx)
        return a, p, a.size

    def set_params(self, idx, records):
        """records: SIM_PARAMS_DTYPE [len(idx)] (idx None: one per triple).  In force from the next call's first frame."""
        a, p, n = self._idx(idx)
        r = np.ascontiguousarray(records, dtype=SIM_PARAMS_DTYPE).reshape(-1)
        if r.size != n:
            raise ValueError(f"need {n} parameter records, got {r.size}")
        self._lib.check(self._lib.L.nnn_sim_set_params(self._h, p, n, _ffi.ptr(r)))

    def params(self, idx=None):
        a, p, n = self._idx(idx)
        r = np.zeros(n, SIM_PARAMS_DTYPE)
        self._lib.check(self._lib.L.nnn_sim_get_params(self._h, p, n, _ffi.ptr(r)))
        return r

    def _offsets(self, sig_off, noise_off):
        so, no = (np.ascontiguousarray(o, dtype=np.uint64) for o in (sig_off, noise_off))
        if so.ndim != 2 or so.shape[1] != self.n_streams or no.shape != so.shape:
            raise ValueError(f"offsets must be two arrays of shape [n_frames, {self.n_streams}]")
        return so, no, so.shape[0]

    def process(self, sig_off, noise_off, rows=None):
        """Rows float32 [n_frames, n_streams, 87] for the named frames (synchronous; an offset that leaves its arena refuses the call)."""
        so, no, T = self._offsets(sig_off, noise_off)
        if rows is None:
            rows = np.empty((T, self.n_streams, ROW_WIDTH), np.float32)
        if not (isinstance(rows, np.ndarray) and rows.shape == (T, self.n_streams, ROW_WIDTH) and rows.dtype == np.float32 and rows.flags.c_contiguous and rows.flags.writeable):
            raise ValueError(f"rows must be a writable C-contiguous float32 array of shape [n_frames, n_streams, {ROW_WIDTH}]")
        self._lib.check(self._lib.L.nnn_sim_process_host(self._h, _ffi.ptr(so), _ffi.ptr(no), _ffi.ptr(rows), T))
        return rows

    def signals(self, sig_off, noise_off):
        """(signal, noise, combined) float32 [n_streams, n_frames, 480], band_gain_cutoff int32 and vad float32 [n_frames, n_streams]:
        what TrainingFeatures.process takes.  Advances the simulator as process does; the feature states are not touched."""
        so, no, T = self._offsets(sig_off, noise_off)
        S = self.n_streams
        sig, noise, comb = (np.empty((S, T, FRAME_SIZE), np.float32) for _ in range(3))
        cut, vad = np.empty((T, S), np.int32), np.empty((T, S), np.float32)
        self._lib.check(self._lib.L.nnn_sim_signals_host(self._h, _ffi.ptr(so), _ffi.ptr(no), _ffi.ptr(sig), _ffi.ptr(noise), _ffi.ptr(comb),
                                                         _ffi.ptr(cut), _ffi.ptr(vad), T))
        return sig, noise, comb, cut, vad

    def process_device(self, d_sig_off, d_noise_off, d_rows, n_frames, hip_stream=0):
        """Raw device pointers (include/nnn_sim.h); asynchronous.  A frame outside its arena reads as zeros and sets fault()."""
        self._lib.check(self._lib.L.nnn_sim_process_device(self._h, d_sig_off, d_noise_off, d_rows, n_frames, hip_stream))

    def signals_device(self, d_sig_off, d_noise_off, d_signal, d_noise, d_combined, d_cutoff, d_vad, n_frames, stream_stride, frame_stride,
                       hip_stream=0):
        self._lib.check(self._lib.L.nnn_sim_signals_device(self._h, d_sig_off, d_noise_off, d_signal, d_noise, d_combined, d_cutoff, d_vad,
                                                           n_frames, stream_stride, frame_stride, hip_stream))

    def debug_kernel(self, d_sig_off, d_noise_off, n_frames, reps, hip_stream=0):
        """Measuring hook: k_sim alone, `reps` launches into the staging."""
        self._lib.check(self._lib.L.nnn_sim_debug_kernel(self._h, d_sig_off, d_noise_off, n_frames, reps, hip_stream))

    def reset(self):
        """Filter memories and VAD counters to zero; parameters and arenas stay.  Pair with TrainingFeatures.reset."""
        self._lib.check(self._lib.L.nnn_sim_reset(self._h))

    def fault(self):
        rc = self._lib.L.nnn_sim_fault(self._h)
        if rc < 0:
            raise RuntimeError("nnnoiseless_amd: " + self._lib.error())
        return bool(rc)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.L.nnn_sim_destroy(self._h)
            self._h = None

    __del__ = close


# ---- the two host policies (pure Python, no device) ----------------------------------------------------------------------------------

def band_lp_for(lowpass):
    """The first band i with EBAND_5MS[i] << 2 > lowpass, else 21 (src/training.rs:361-364)."""
    for i, e in enumerate(EBAND_5MS):
        if e << 2 > lowpass:
            return i
    return NB_BANDS - 1


def random_params(rng, n):
    """randomize() and random_filter() (src/training.rs:291-365) for n triples, as SIM_PARAMS_DTYPE records, in f32 as there:
    signal_gain = 10^(k/20), k an integer in [-40, 20); noise_gain = 10^(k/20) x signal_gain, k in [-20, 20); signal_gain = 0 with
    probability 0.1 (after noise_gain took it); eight coefficients 0.75 x (U[0, 1) - 0.5); lowpass = int(481 x 3000/24000 x 50^U) and
    band_lp from it.  `rng` is a numpy Generator: the reference draws from thread_rng, which has no seed, so it is the
    distribution that is restated, not a sequence."""
    f32 = np.float32
    p = np.zeros(n, SIM_PARAMS_DTYPE)
    sg = np.power(f32(10.0), rng.integers(-40, 20, n).astype(f32) / f32(20.0)).astype(f32)
    ng = np.power(f32(10.0), rng.integers(-20, 20, n).astype(f32) / f32(20.0)).astype(f32) * sg
    sg[rng.random(n) < 0.1] = 0.0
    p["signal_gain"], p["noise_gain"] = sg, ng
    for name in ("sig_a", "sig_b", "noise_a", "noise_b"):   # (the reference's order: sig a, sig b, noise a, noise b)
        p[name] = f32(0.75) * (rng.random((n, 2), dtype=f32) - f32(0.5))
    lowpass = (f32(481.0) * f32(3000.0) / f32(24000.0) * np.power(f32(50.0), rng.random(n, dtype=f32))).astype(np.int64)
    p["band_lp"] = [band_lp_for(int(v)) for v in lowpass]
    return p


class ClipCursor:
    """SignalReader (src/training.rs:171-261) for n_streams readers over one arena whose clip i is lengths[i] samples at element
    starts[i]: next(n_frames) says where each reader's next frames lie.

    frames_per_file = max(count // n_files + 1, 100), with the TOTAL row count of the run.  A clip longer than 480 x frames_per_file
    gives a random slice of that many frames, a shorter one its len // 480 whole frames from its start; after a clip's last frame the
    reader moves to the next clip, cyclically.  Reader s starts at clip (s x n_files) // n_streams, so that the readers tile the list,
    and draws from a generator of its own (seeded from `rng`, reader by reader), so a reader's walk does not depend on how the calls
    are cut.  A clip shorter than one frame is skipped: the reference loops forever on one (its next_reader never advances past a
    clip that yields no frame)."""

    def __init__(self, starts, lengths, count, n_streams, rng):
        self.starts = np.asarray(starts, dtype=np.int64).reshape(-1)
        self.lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
        n = self.starts.size
        if n == 0 or self.lengths.size != n:
            raise ValueError("cannot read from an empty set of clips")
        if not (self.lengths >= FRAME_SIZE).any():
            raise ValueError("every clip is shorter than one frame")
        self.n_streams = int(n_streams)
        self.frames_per_file = max(int(count) // n + 1, 100)
        self._rngs = [np.random.default_rng(int(s)) for s in rng.integers(0, 2 ** 63, self.n_streams)]
        self._idx = [(s * n) // self.n_streams for s in range(self.n_streams)]
        self._left = [0] * self.n_streams
        self._pos = [0] * self.n_streams

    def _next_reader(self, s):
        n = self.starts.size
        while self._left[s] == 0:
            if self._idx[s] >= n:
                self._idx[s] = 0
            i = self._idx[s]
            length, want = int(self.lengths[i]), FRAME_SIZE * self.frames_per_file
            if length > want:
                self._pos[s] = int(self.starts[i]) + int(self._rngs[s].integers(0, length - want + 1))
                self._left[s] = self.frames_per_file
            else:
                self._pos[s] = int(self.starts[i])
                self._left[s] = length // FRAME_SIZE
            if self._left[s] == 0:
                self._idx[s] += 1      # (a clip shorter than one frame)

    def next(self, n_frames):
        """uint64 [n_frames, n_streams]: the arena element where each reader's next n_frames frames begin."""
        out = np.empty((n_frames, self.n_streams), np.uint64)
        for s in range(self.n_streams):
            t = 0
            while t < n_frames:
                if self._left[s] == 0:
                    self._next_reader(s)
                m = min(self._left[s], n_frames - t)
                out[t:t + m, s] = self._pos[s] + FRAME_SIZE * np.arange(m)
                self._pos[s] += FRAME_SIZE * m
                self._left[s] -= m
                t += m
                if self._left[s] == 0:
                    self._idx[s] += 1
        return out


def _arena(clips):
    clips = [np.ascontiguousarray(c).reshape(-1) for c in clips]
    if not clips or any(c.dtype != np.int16 for c in clips):
        raise ValueError("clips must be a non-empty list of int16 arrays")
    lengths = np.array([c.size for c in clips], np.int64)
    return np.concatenate(clips), np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64), lengths


def call_cuts(n_frames, group=GROUP_FRAMES):
    """The generator's calls for n_frames frames per triple: (first frame, frames, new parameters first?) with at most `group` frames a
    call, cut where gain_change_count passes GAIN_CHANGE_COUNT: the creation parameters are in force for the first 2821 frames, and
    every 2822 frames from there on randomize() runs before the frame (src/training.rs:388-393)."""
    cuts, t, nxt = [], 0, GAIN_CHANGE_COUNT
    while t < n_frames:
        change = t == nxt
        if change:
            nxt += GAIN_CHANGE_COUNT + 1
        n = min(group, n_frames - t, nxt - t)
        cuts.append((t, n, change))
        t += n
    return cuts


def generate_rows(signal_clips, noise_clips, count, n_streams, seed, simulator=None, lib=None, device=0):
    """The generator's main loop (src/training.rs:120-161) for n_streams triples side by side: `count` rows in all, i.e.
    ceil(count / n_streams) consecutive frames per triple.  signal_clips / noise_clips: lists of int16 arrays (48 kHz mono).
    Returns rows float32 [count_per_stream, n_streams, 87].  The training script (train/rnn_train.py) windows CONSECUTIVE rows, so a
    consumer takes them stream by stream (rows[:, s]), not frame by frame across streams: nnnoiseless_amd.fit.windows does, and
    nnnoiseless_amd.fit.fit trains on them.
    `simulator`: an object with load_signal / load_noise / set_params / process to use instead of a new NoiseSimulator."""
    rng = np.random.default_rng(seed)
    sig, s_starts, s_len = _arena(signal_clips)
    noise, n_starts, n_len = _arena(noise_clips)
    per_stream = -(-int(count) // int(n_streams))
    sig_cur = ClipCursor(s_starts, s_len, count, n_streams, rng)
    noise_cur = ClipCursor(n_starts, n_len, count, n_streams, rng)
    features = None
    if simulator is None:
        features = TrainingFeatures(n_streams, device, lib)
        simulator = NoiseSimulator(features)
    simulator.load_signal(sig)
    simulator.load_noise(noise)
    rows = np.empty((per_stream, n_streams, ROW_WIDTH), np.float32)
    for t, n, change in call_cuts(per_stream):
        if change:
            simulator.set_params(None, random_params(rng, n_streams))
        simulator.process(sig_cur.next(n), noise_cur.next(n), rows[t:t + n])
    if features is not None:
        simulator.close()
        features.close()
    return rows


def _read_clip(path):
    from . import files, pcm
    fmt, channels, rate, data = files.read_wav(path)
    if fmt != pcm.PCM_I16 or channels != 1 or rate != 48000:   # src/training.rs:203-213
        raise SystemExit(f"unsupported wav format in {path}: {channels} channel(s), {rate} Hz, packer format {fmt}; the generator reads "
                         "16-bit mono 48 kHz clips only")
    return np.ascontiguousarray(data.reshape(-1), dtype=np.int16)


def main(argv=None):
    import argparse
    import glob
    ap = argparse.ArgumentParser(prog="python -m nnnoiseless_amd.training",
                                 description="Training rows from clean and noise clips (16-bit mono 48 kHz WAVs), simulated and analysed on the GPU. "
                                             "Writes a NumPy .npy file [rows per stream, streams, 87]; the reference's generator writes HDF5, "
                                             "which needs a library this package does not depend on: convert with h5py where it is at hand.")
    ap.add_argument("--signal-glob", required=True, help="pattern of the clean-speech clips")
    ap.add_argument("--noise-glob", required=True, help="pattern of the noise clips")
    ap.add_argument("--count", type=int, required=True, help="rows in all (rounded up to a multiple of --streams)")
    ap.add_argument("-o", "--output", required=True, help="the .npy file to write")
    ap.add_argument("--streams", type=int, default=64, help="triples simulated side by side (default 64)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    clips = []
    for what, pattern in (("signal", args.signal_glob), ("noise", args.noise_glob)):
        paths = sorted(glob.glob(pattern))
        if not paths:
            raise SystemExit(f"--{what}-glob {pattern!r} matches no file")
        clips.append([_read_clip(p) for p in paths])
    if args.count < 1 or args.streams < 1:
        raise SystemExit("--count and --streams must be positive")
    rows = generate_rows(clips[0], clips[1], args.count, args.streams, args.seed, device=args.device)
    np.save(args.output, rows)
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
