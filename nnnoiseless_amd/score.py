"""The scorer (include/nnn_score.h): how good is the audio a model produces?

Scorer mirrors the C object: per stream the sums A = sum r^2, B = sum y^2, C = sum r y, E = sum (r - y)^2 between a reference r
(delayed by a per-stream number of samples) and a test signal y, in f64 in one fixed order, carried across calls on the device.
What is policy rather than arithmetic stays on the host as plain Python without a device: the figures in dB (snr_db, si_sdr_db,
segmental_snr_db) are functions of the sums, and evaluate is the loop a user wants -- simulate noisy speech, denoise it, score the
mix and the output against the clean signal (`python -m nnnoiseless_amd.score` is its front-end).
"""
import ctypes as C

import numpy as np

from . import FRAME_SIZE, _ffi, library

SUMS = _ffi.SCORE_SUMS              # A, B, C, E
MAX_DELAY = _ffi.SCORE_MAX_DELAY
OUTPUT_DELAY = FRAME_SIZE           # the denoiser's one frame of overlap-add latency (DESIGN.md section 23 says where it is read)
GROUP_FRAMES = 24                   # frames per call of evaluate: a batch's default max_group_frames


class Scorer:
    """n_streams running comparisons of a test signal with a reference delayed by `delay[s]` samples.

    Arrays are float32 [n_streams, n_frames, 480]; valid is uint8 / bool [n_frames, n_streams]; frame sums are float64
    [n_frames, n_streams, 4] and totals float64 [n_streams, 4], columns A, B, C, E.  The *_device methods take raw pointers."""

    def __init__(self, n_streams, max_delay=MAX_DELAY, device=0, lib=None):
        self._lib = lib or library()
        if not hasattr(self._lib.L, "nnn_score_create"):
            raise RuntimeError("nnnoiseless_amd: this build of the library has no scorer (nnn_score_*)")
        self.n_streams, self.max_delay = int(n_streams), int(max_delay)
        self._h = self._lib.L.nnn_score_create(self.n_streams, self.max_delay, device)
        if not self._h:
            raise RuntimeError("nnnoiseless_amd: " + self._lib.error())

    def _idx(self, idx):
        if idx is None:
            return None, self.n_streams
        a, p = _ffi.stream_list(idx)
        self._keep = a
        return p, a.size

    def set_delay(self, idx, delays):
        """Delays in samples of the listed streams (idx None: of every stream); a scalar serves all of them.  Also zeroes those
        streams' history, totals and count."""
        p, n = self._idx(idx)
        d = np.asarray(delays, dtype=np.int64)
        d = np.full(n, d, np.int64) if d.ndim == 0 else d.reshape(-1)
        if d.size != n:
            raise ValueError(f"need {n} delays, got {d.size}")
        if d.size and (d.min() < -2 ** 31 or d.max() >= 2 ** 31):
            raise ValueError("delay out of int32 range")
        d = np.ascontiguousarray(d, dtype=np.int32)
        self._lib.check(self._lib.L.nnn_score_set_delay(self._h, p, n, _ffi.ptr(d)))

    def delay(self, idx=None):
        p, n = self._idx(idx)
        d = np.zeros(n, np.int32)
        self._lib.check(self._lib.L.nnn_score_get_delay(self._h, p, n, _ffi.ptr(d)))
        return d

    def reset(self, idx=None):
        """History, totals and count of the listed streams (None: all) to zero; the delays stay."""
        p, n = self._idx(idx)
        self._lib.check(self._lib.L.nnn_score_reset(self._h, p, n))

    def accumulate(self, ref, test, valid=None, frame_sums=False):
        """ref / test: float32 [n_streams, n_frames, 480] on the host (synchronous).  valid: None or [n_frames, n_streams], 0 = the
        frame does not count (its reference samples still pass).  frame_sums=True returns float64 [n_frames, n_streams, 4]."""
        r, y = _ffi.as_f32(ref), _ffi.as_f32(test)
        if r.ndim != 3 or r.shape[0] != self.n_streams or r.shape[2] != FRAME_SIZE or y.shape != r.shape:
            raise ValueError(f"accumulate needs two arrays of shape [{self.n_streams}, n_frames, {FRAME_SIZE}]")
        T = r.shape[1]
        v = None
        if valid is not None:
            v = np.ascontiguousarray(np.asarray(valid) != 0, dtype=np.uint8)
            if v.shape != (T, self.n_streams):
                raise ValueError("valid must have shape [n_frames, n_streams]")
        fs = np.empty((T, self.n_streams, SUMS), np.float64) if frame_sums else None
        self._lib.check(self._lib.L.nnn_score_accumulate_host(self._h, _ffi.ptr(r), _ffi.ptr(y), _ffi.ptr(v), _ffi.ptr(fs), T))
        return fs

    def accumulate_device(self, d_ref, d_test, n_frames, stream_stride, frame_stride, d_valid=None, d_frame_sums=None, hip_stream=0):
        """Raw device pointers (include/nnn_score.h); asynchronous.  Strides in floats."""
        self._lib.check(self._lib.L.nnn_score_accumulate_device(self._h, d_ref, d_test, d_valid, d_frame_sums, n_frames, stream_stride, frame_stride,
                                                                hip_stream))

    def totals(self):
        """(totals float64 [n_streams, 4], counts uint64 [n_streams]); waits for the calls made so far."""
        t, c = np.empty((self.n_streams, SUMS), np.float64), np.empty(self.n_streams, np.uint64)
        self._lib.check(self._lib.L.nnn_score_totals(self._h, _ffi.ptr(t), _ffi.ptr(c)))
        return t, c

    def totals_device(self, d_totals, d_counts=None, hip_stream=0):
        """Asynchronous copy into device memory of the caller's: double [n_streams][4] and uint64 [n_streams] (either may be None)."""
        self._lib.check(self._lib.L.nnn_score_totals_device(self._h, d_totals, d_counts, hip_stream))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.L.nnn_score_destroy(self._h)
            self._h = None

    __del__ = close


# ---- the figures: plain float64 NumPy on the sums, no device --------------------------------------------------------------------------------
def _f64(*a):
    return [np.asarray(x, dtype=np.float64) for x in a]


def snr_db(A, E):
    """10 log10(A / E): the reference's energy over the error's.  Nothing raises: E = 0 with A > 0 gives +inf (the signals are
    equal), A = 0 with E > 0 gives -inf, A = E = 0 gives nan, as NumPy's division and logarithm do."""
    A, E = _f64(A, E)
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10.0 * np.log10(A / E)


def si_sdr_db(A, B, C):
    """The scale-invariant signal-to-distortion ratio 10 log10(C^2 / (A B - C^2)): the test signal projected on the reference, over
    what is left of it.  Nothing raises: A B = C^2 > 0 (the test is a multiple of the reference) gives +inf, C = 0 with A B > 0 gives
    -inf, A B = C = 0 (a silent signal) gives nan; A B - C^2 < 0, which rounding can produce for nearly proportional signals, gives nan."""
    A, B, C = _f64(A, B, C)
    with np.errstate(divide="ignore", invalid="ignore"):
        c2 = C * C
        return 10.0 * np.log10(c2 / (A * B - c2))


def segmental_snr_db(frame_sums, lo=-10.0, hi=35.0, active=0.0):
    """The mean over frames of clip(10 log10(A_f / E_f), lo, hi), over the frames whose reference power A_f / 480 exceeds `active`.
    frame_sums: float64 [n_frames, ..., 4] as accumulate returns them; the mean is taken over the first axis, so [n_frames, n_streams, 4]
    gives one figure per stream.  A frame with E_f = 0 counts as `hi`; a stream (column) without an active frame gives nan.  Frames marked
    invalid are all zero and never active."""
    fs = np.asarray(frame_sums, dtype=np.float64)
    A, E = fs[..., 0], fs[..., 3]
    on = A / float(FRAME_SIZE) > active
    with np.errstate(divide="ignore", invalid="ignore"):
        seg = np.clip(10.0 * np.log10(A / E), lo, hi)
        n = on.sum(axis=0)
        return np.where(on, seg, 0.0).sum(axis=0) / np.where(n > 0, n, np.nan)


# ---- the loop ---------------------------------------------------------------------------------------------------------------------------
def evaluation_plan(signal_clips, noise_clips, count, n_streams, seed):
    """What evaluate simulates, as data: the two arenas (int16), each frame's offsets into them (uint64 [frames per stream, n_streams]) and
    the simulator's parameters.  The clips are read as the generator reads them (training.ClipCursor); the parameters are one draw of
    training.random_params per stream, with the clean signal's gain put back to 1 where the draw silenced it (a silent reference has
    no SNR).  Plain Python: the same arguments give the same plan."""
    from . import training
    rng = np.random.default_rng(seed)
    sig, s_starts, s_len = training._arena(signal_clips)
    noise, n_starts, n_len = training._arena(noise_clips)
    per_stream = -(-int(count) // int(n_streams))
    sig_cur = training.ClipCursor(s_starts, s_len, count, n_streams, rng)
    noise_cur = training.ClipCursor(n_starts, n_len, count, n_streams, rng)
    params = training.random_params(rng, n_streams)
    params["signal_gain"][params["signal_gain"] == 0.0] = 1.0
    return sig, noise, sig_cur.next(per_stream), noise_cur.next(per_stream), params


def evaluate(model_bytes, signal_clips, noise_clips, count, n_streams, seed, gain_floor=None, device=0, lib=None):
    """Noisy speech simulated from the clips, denoised with the model, and both the mix and the output scored against the clean signal,
    all resident on the device: `count` frames in all, ceil(count / n_streams) consecutive frames per stream.

    model_bytes: a .rnn file's bytes, or None for the built-in model.  gain_floor: None, or what BatchDenoiser.set_gain_floor takes for
    every stream.  Scorer A takes clean against mix at delay 0; scorer B clean against output at delay 480, the output's latency.
    Returns a dict: "mix" and "out" (totals float64 [n_streams, 4]), "frames" (uint64 [n_streams]), "snr_mix_db", "snr_out_db",
    "si_sdr_mix_db", "si_sdr_out_db" and the improvements "snr_gain_db", "si_sdr_gain_db" per stream, and the same six figures over the
    sums of all streams under "all"."""
    import torch
    from . import BatchDenoiser, RnnModel, training
    lib = lib or library()
    S = int(n_streams)
    sig, noise, sig_off, noise_off, params = evaluation_plan(signal_clips, noise_clips, count, S, seed)
    T = sig_off.shape[0]
    dev = torch.device("cuda", device)
    model = None
    if model_bytes is not None:
        model = RnnModel.from_bytes(bytes(model_bytes), lib=lib)
        if model is None:
            raise ValueError("model_bytes is not a .rnn file")
    features = training.TrainingFeatures(S, device, lib)
    sim = training.NoiseSimulator(features)
    sim.load_signal(sig)
    sim.load_noise(noise)
    sim.set_params(None, params)
    bd = BatchDenoiser(S, model=model, device=device, lib=lib)
    if gain_floor is not None:
        bd.set_gain_floor(range(S), gain_floor)
    a, b = Scorer(S, 0, device, lib), Scorer(S, OUTPUT_DELAY, device, lib)
    b.set_delay(None, OUTPUT_DELAY)
    with torch.cuda.device(dev):
        st = torch.cuda.Stream()
        sp = st.cuda_stream
        G = min(GROUP_FRAMES, T)
        audio = torch.empty((4, S, G * FRAME_SIZE), device=dev)          # clean, noise, mix, output: [S][G * 480] each
        cut, lab = torch.empty((G, S), device=dev, dtype=torch.int32), torch.empty((G, S), device=dev)
        vad = torch.empty((G, S), device=dev)
        so = torch.from_numpy(sig_off.astype(np.int64)).to(dev)          # (offsets below 2^63: the same bits as uint64)
        no = torch.from_numpy(noise_off.astype(np.int64)).to(dev)
        clean, nz, mix, out = (audio[k].data_ptr() for k in range(4))
        ss, fs = G * FRAME_SIZE, FRAME_SIZE
        torch.cuda.synchronize(dev)                                      # (the uploads above ran on torch's own stream)
        for t in range(0, T, G):
            n = min(G, T - t)
            sim.signals_device(so[t].data_ptr(), no[t].data_ptr(), clean, nz, mix, cut.data_ptr(), lab.data_ptr(), n, ss, fs, sp)
            bd.process_device(mix, out, vad.data_ptr(), n, ss, fs, sp)
            a.accumulate_device(clean, mix, n, ss, fs, hip_stream=sp)
            b.accumulate_device(clean, out, n, ss, fs, hip_stream=sp)
        st.synchronize()
    (ta, frames), (tb, _) = a.totals(), b.totals()
    res = {"mix": ta, "out": tb, "frames": frames}
    res.update(_figures(ta, tb))
    res["all"] = _figures(ta.sum(axis=0), tb.sum(axis=0))
    for o in (a, b, bd, sim, features):
        o.close()
    return res


def _figures(ta, tb):
    f = {"snr_mix_db": snr_db(ta[..., 0], ta[..., 3]), "snr_out_db": snr_db(tb[..., 0], tb[..., 3]),
         "si_sdr_mix_db": si_sdr_db(ta[..., 0], ta[..., 1], ta[..., 2]), "si_sdr_out_db": si_sdr_db(tb[..., 0], tb[..., 1], tb[..., 2])}
    f["snr_gain_db"] = f["snr_out_db"] - f["snr_mix_db"]
    f["si_sdr_gain_db"] = f["si_sdr_out_db"] - f["si_sdr_mix_db"]
    return f


def main(argv=None):
    import argparse
    import glob
    import json
    from . import training
    ap = argparse.ArgumentParser(prog="python -m nnnoiseless_amd.score",
                                 description="SNR and SI-SDR of a model's output against the clean signal, and their improvement over the noisy "
                                             "mix, on noisy speech simulated from clean and noise clips (16-bit mono 48 kHz WAVs) on the GPU.")
    ap.add_argument("--model", help="the .rnn file to score (default: the built-in model)")
    ap.add_argument("--signal-glob", required=True, help="pattern of the clean-speech clips")
    ap.add_argument("--noise-glob", required=True, help="pattern of the noise clips")
    ap.add_argument("--count", type=int, required=True, help="frames in all (rounded up to a multiple of --streams)")
    ap.add_argument("--streams", type=int, default=64, help="streams simulated side by side (default 64)")
    ap.add_argument("--gain-floor", type=float, help="a gain floor for every stream and band (e.g. 0.126 = never more than 18 dB down)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--json", help="write the result, per-stream figures included, to this file")
    args = ap.parse_args(argv)
    clips = []
    for what, pattern in (("signal", args.signal_glob), ("noise", args.noise_glob)):
        paths = sorted(glob.glob(pattern))
        if not paths:
            raise SystemExit(f"--{what}-glob {pattern!r} matches no file")
        clips.append([training._read_clip(p) for p in paths])
    if args.count < 1 or args.streams < 1:
        raise SystemExit("--count and --streams must be positive")
    model = open(args.model, "rb").read() if args.model else None
    res = evaluate(model, clips[0], clips[1], args.count, args.streams, args.seed, gain_floor=args.gain_floor, device=args.device)
    al = res["all"]
    print(f"{int(res['frames'].sum())} frames on {args.streams} streams")
    print(f"SNR    mix {al['snr_mix_db']:8.3f} dB   output {al['snr_out_db']:8.3f} dB   improvement {al['snr_gain_db']:+8.3f} dB")
    print(f"SI-SDR mix {al['si_sdr_mix_db']:8.3f} dB   output {al['si_sdr_out_db']:8.3f} dB   improvement {al['si_sdr_gain_db']:+8.3f} dB")
    if args.json:
        def plain(v):
            return {k: plain(x) for k, x in v.items()} if isinstance(v, dict) else np.asarray(v).tolist()
        with open(args.json, "w") as f:
            json.dump(plain(res), f)
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
