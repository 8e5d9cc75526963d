"""The reference's multi-channel callers of process_frame, as batched calls on packed PCM.

  denoise_raw_i16   the CLI's raw-PCM loop: interleaved int16 in, interleaved int16 out, trailing partial frame
                    dropped, first frame not written (src/nnnoiseless.rs:301-331, RawFrameWriter :147-160)
  DenoiseSignal     the dasp adapter: unit-range float frames in and out, one state per channel, first frame
                    discarded (src/signal.rs:31-137)

Sample conversion, channel (de)interleave and the dropped first frame happen inside the first and last HIP kernels
(include/nnn_batch.h, nnn_batch_process_pcm_*); nothing here computes on the host beyond slicing.
"""
import ctypes as C

import numpy as np

from . import FRAME_SIZE, BatchDenoiser, _ffi

PCM_F32, PCM_I16, PCM_F32_UNIT = _ffi.PCM_F32, _ffi.PCM_I16, _ffi.PCM_F32_UNIT


def denoise_raw_i16(pcm, channels=1, model=None, block_frames=512, device=0, lib=None):
    """pcm: int16, either [n, channels] (one file) or [n_files, n, channels] (equal-length files denoised together).
    Returns int16 of the same rank with (n // 480 - 1) * 480 sample frames per file."""
    pcm = np.asarray(pcm, dtype=np.int16)
    single = pcm.ndim == 2
    if pcm.ndim == 1:
        pcm, single = pcm.reshape(-1, channels), True
    if single:
        pcm = pcm[None]
    G, n, C = pcm.shape
    if C != channels:
        raise ValueError("last axis must be the channel axis")
    T = n // FRAME_SIZE                                    # src/nnnoiseless.rs:303-311: a short read ends the loop
    bd = BatchDenoiser(G * channels, model, device, lib)
    outs = []
    for t0 in range(0, T, block_frames):
        t1 = min(T, t0 + block_frames)
        o, _ = bd.process_pcm(pcm[:, t0 * FRAME_SIZE:t1 * FRAME_SIZE], PCM_I16, channels, discard_first=True)
        outs.append(o)
    bd.close()
    out = np.concatenate(outs, axis=1) if outs else np.zeros((G, 0, channels), np.int16)
    return out[0] if single else out


class DenoiseSignal:
    """DenoiseSignal over an in-memory signal: `input` float32 [n, channels] in [-1, 1] (src/signal.rs:31-137).

    Iterating yields denoised sample frames (arrays of `channels` floats); `collect()` returns them all as [n_out,
    channels].  End of signal follows dasp_signal 0.11's `from_iter` source, which reports exhaustion as soon as its
    last frame has been taken: the refill that consumes the last input samples returns false, so its frame is never
    handed out (src/signal.rs:90-106, :129-134)."""

    def __init__(self, input, model=None, channels=None, device=0, lib=None):
        x = np.asarray(input, dtype=np.float32)
        if x.ndim == 1:
            x = x[:, None]
        self.channels = channels or x.shape[1]
        if x.shape[1] != self.channels:
            raise ValueError("last axis must be the channel axis")
        n = len(x)
        # refill k reads samples [480 k, 480 k + 480), zero ("equilibrium") padded, while any input is left
        n_proc = -(-n // FRAME_SIZE)
        pad = np.zeros((n_proc * FRAME_SIZE, self.channels), np.float32)
        pad[:n] = x
        if n_proc:
            bd = BatchDenoiser(self.channels, model, device, lib)
            y, _ = bd.process_pcm(pad[None], PCM_F32_UNIT, self.channels, discard_first=False)
            bd.close()
            y = y[0].reshape(n_proc, FRAME_SIZE, self.channels)
        else:
            y = np.zeros((0, FRAME_SIZE, self.channels), np.float32)
        zeros = np.zeros((FRAME_SIZE, self.channels), np.float32)

        def held(k):   # out_bufs after refills 0..k (a refill on an exhausted input leaves them untouched)
            k = min(k, n_proc - 1)
            return y[k] if k >= 0 else zeros

        frames = [held(1)]                                  # the constructor refills twice, :83-87
        k = 2
        while FRAME_SIZE * k < n and FRAME_SIZE * (k + 1) < n:   # refill k: input left before, and after
            frames.append(held(k))
            k += 1
        self._out = np.concatenate(frames, axis=0)

    def collect(self):
        return self._out

    def __iter__(self):
        return iter(self._out)

    def __len__(self):
        return len(self._out)


class Resampler:
    """n_streams mono streams of one common sample rate -> 48 kHz with the CLI's 16-tap windowed sinc
    (src/nnnoiseless.rs:19-32, 106-131), batched on the GPU (include/nnn_resample.h).  Feed the streams in chunks of any
    size: the output does not depend on the chunking."""

    def __init__(self, n_streams, source_rate, device=0, lib=None):
        from . import library
        self._lib = lib or library()
        self.n_streams = int(n_streams)
        self.ratio = float(source_rate) / 48000.0
        self._h = self._lib.L.nnn_resampler_create(self.n_streams, self.ratio, device)
        if not self._h:
            raise RuntimeError("nnnoiseless_amd: " + self._lib.error())

    def process(self, x):
        """x: float32 [n_streams, n] source samples -> float32 [n_streams, n_out]."""
        import ctypes as C
        x = _ffi.as_f32(x)
        S, n = x.shape
        assert S == self.n_streams
        cap = self._lib.L.nnn_resampler_max_output(self._h, n)
        out = np.zeros((S, cap), np.float32)
        n_out = C.c_long(0)
        self._lib.check(self._lib.L.nnn_resampler_process_host(self._h, _ffi.ptr(x), n, _ffi.ptr(out), cap, C.byref(n_out)))
        return np.ascontiguousarray(out[:, :n_out.value])

    def reset(self):
        self._lib.check(self._lib.L.nnn_resampler_reset(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.L.nnn_resampler_destroy(self._h)
            self._h = None

    __del__ = close


class RateAdapter:
    """Streams at `source_rate` in and out of a 48 kHz batch (include/nnn_rate.h): the CLI's resampler in front of the batch, the
    batch's ordinary call over the whole frames, and the same interpolator at the inverse ratio behind it, in one asynchronous call
    on the GPU.  The adapter carries the partial frame and both legs' 16-sample histories from call to call: feed chunks of any size
    (up to `max_in` samples per stream), the output does not depend on the chunking.  It borrows `batch`, which must outlive it;
    reset, hold and resume streams on the batch as always -- a reset call also takes `reset_streams` here, a held stream sits the
    adapter's calls out and restarts its two resampler legs from silence when it resumes."""

    def __init__(self, batch, source_rate, max_in):
        self._lib = batch._lib
        if not hasattr(self._lib.L, "nnn_rate_create"):
            raise RuntimeError("nnnoiseless_amd: this build of the library has no rate adapter")
        self.batch = batch
        self.n_streams = batch.n_streams
        self.source_rate = float(source_rate)
        self.max_in = int(max_in)
        self._h = self._lib.L.nnn_rate_create(batch._h, self.source_rate, self.max_in)
        if not self._h:
            raise RuntimeError("nnnoiseless_amd: " + self._lib.error())

    def max_output(self, n_in):
        """Bound of the source-rate samples a call of n_in samples per stream can return."""
        return int(self._lib.L.nnn_rate_max_output(self._h, int(n_in)))

    def max_frames(self, n_in):
        """Bound of the frames (VAD rows) such a call can complete."""
        return int(self._lib.L.nnn_rate_max_frames(self._h, int(n_in)))

    def carried(self):
        """48 kHz samples of the partial frame now held."""
        return int(self._lib.L.nnn_rate_carried(self._h))

    def process(self, x, out=None, vad=None):
        """x: [n_streams, n] source-rate samples, float32 (i16 range) or int16 -> (y [n_streams, n_out] of x's dtype, vad [n_frames,
        n_streams]).  `out` ([n_streams, >= max_output(n)]) and `vad` ([>= max_frames(n), n_streams]), when handed in, are written in
        place -- what held streams own in them stays as it was -- and views of their filled parts are returned."""
        import ctypes as C
        x = np.asarray(x)
        fmt = PCM_I16 if x.dtype == np.int16 else PCM_F32
        x = np.ascontiguousarray(x, dtype=_ffi.PCM_DTYPE[fmt])
        if x.ndim != 2 or x.shape[0] != self.n_streams:
            raise ValueError(f"process needs x of shape [{self.n_streams}, n], got {x.shape}")
        n = x.shape[1]
        out = np.zeros((self.n_streams, self.max_output(n)), x.dtype) if out is None else out
        vad = np.zeros((self.max_frames(n), self.n_streams), np.float32) if vad is None else vad
        if not (isinstance(out, np.ndarray) and out.ndim == 2 and out.shape[0] == self.n_streams and out.dtype == x.dtype
                and out.flags.c_contiguous and out.flags.writeable):
            raise ValueError("process: `out` must be a writable C-contiguous [n_streams, cap] array of x's dtype")
        if not (isinstance(vad, np.ndarray) and vad.ndim == 2 and vad.shape[1] == self.n_streams and vad.dtype == np.float32
                and vad.flags.c_contiguous and vad.flags.writeable):
            raise ValueError("process: `vad` must be a writable C-contiguous float32 [cap_frames, n_streams] array")
        n_out, n_frames = C.c_long(0), C.c_int(0)
        self._lib.check(self._lib.L.nnn_rate_process_host(self._h, _ffi.ptr(x), n, _ffi.ptr(out), out.shape[1], C.byref(n_out), _ffi.ptr(vad),
                                                          vad.shape[0], C.byref(n_frames), fmt))
        self.batch.frames_done += n_frames.value
        return out[:, :n_out.value], vad[:n_frames.value]

    def process_device(self, d_in, n_in, in_stride, d_out, cap_out, out_stride, d_vad, cap_frames, fmt=PCM_F32, hip_stream=0):
        """Raw device pointers (ints), strides in elements of `fmt`; asynchronous on hip_stream (0 = the batch's own stream).  Returns
        (n_out, n_frames), which are host arithmetic and known at once."""
        import ctypes as C
        n_out, n_frames = C.c_long(0), C.c_int(0)
        self._lib.check(self._lib.L.nnn_rate_process_device(self._h, d_in, int(n_in), int(in_stride), d_out, int(cap_out), int(out_stride),
                                                            C.byref(n_out), d_vad, int(cap_frames), C.byref(n_frames), fmt, hip_stream))
        self.batch.frames_done += n_frames.value
        return n_out.value, n_frames.value

    def reset(self):
        """The adapter alone back to its fresh state (the batch has its own reset)."""
        self._lib.check(self._lib.L.nnn_rate_reset(self._h))

    def reset_streams(self, idx):
        """The listed streams' histories and carried samples cleared from the next call on (beside batch.reset_streams(idx))."""
        a, p = _ffi.stream_list(idx)
        self._lib.check(self._lib.L.nnn_rate_reset_streams(self._h, p, a.size))

    def tables_built(self):
        """(up-leg, down-leg) schedule tables built so far, and the host microseconds spent on them: ((n, n), (us, us))."""
        import ctypes as C
        n, us = (C.c_long * 2)(), (C.c_double * 2)()
        self._lib.check(self._lib.L.nnn_rate_debug_tables(self._h, n, us))
        return (n[0], n[1]), (us[0], us[1])

    def close(self):
        if getattr(self, "_h", None):
            self._lib.L.nnn_rate_destroy(self._h)
            self._h = None

    __del__ = close


PACK_I24, PACK_I32, PACK_F32_WAV = _ffi.PACK_I24, _ffi.PACK_I32, _ffi.PACK_F32_WAV
PACK_SUMMARY = ("steps", "useful", "padded", "held_steps", "launched", "held_frames", "files", "max_pad")
_PACK_IN_DTYPE = {PCM_F32: np.float32, PCM_I16: np.int16, PACK_I24: np.uint8, PACK_I32: np.int32, PACK_F32_WAV: np.float32}


def pack_plan(n_slots, step_frames, frames, lib=None):
    """The plan of a packer run (include/nnn_pack.h, nnn_pack_plan: pure host arithmetic) for files of `frames` WHOLE frames:
    (slot_of_file, first_step_of_file, summary dict in slot units)."""
    import ctypes as C
    from . import library
    lib = lib or library()
    f = np.ascontiguousarray(frames, dtype=np.uint64).reshape(-1)
    slot, first, s = np.zeros(f.size, np.int32), np.zeros(f.size, np.int32), (C.c_int64 * 8)()
    lib.check(lib.L.nnn_pack_plan(int(n_slots), int(step_frames), f.ctypes.data_as(C.POINTER(C.c_uint64)), f.size,
                                  slot.ctypes.data_as(C.POINTER(C.c_int32)), first.ctypes.data_as(C.POINTER(C.c_int32)), s))
    return slot, first, dict(zip(PACK_SUMMARY, [int(v) for v in s]))


class FilePacker:
    """Files of unequal length through one batch, slots refilled (include/nnn_pack.h): every file gets, bit for bit, what it gets alone
    from a fresh batch of `channels` streams and process_pcm(..., discard_first=True) -- the reference CLI's loop -- while the batch
    runs full.  A slot is `channels` consecutive streams; a step is one ordinary call of at most `step_frames` frames (default: the
    batch's max_group_frames).  Borrows `batch`, which must outlive it, have one model and nothing held; floors and the channel link
    set on the batch apply.  A run leaves the batch with every stream it used reset and nothing held."""

    def __init__(self, batch, channels=1, step_frames=None):
        self._lib = batch._lib
        if not hasattr(self._lib.L, "nnn_pack_create"):
            raise RuntimeError("nnnoiseless_amd: this build of the library has no file packer")
        self.batch = batch
        self.channels = int(channels)
        self._h = self._lib.L.nnn_pack_create(batch._h, self.channels, int(step_frames or 0))
        if not self._h:
            raise RuntimeError("nnnoiseless_amd: " + self._lib.error())
        self.n_slots = batch.n_streams // self.channels
        self.step_frames = int(step_frames or batch.max_group_frames())

    def plan(self, frames):
        """(slot_of_file, first_step_of_file, summary) for files of `frames` whole frames on this packer's slots and step."""
        return pack_plan(self.n_slots, self.step_frames, frames, self._lib)

    def last_summary(self):
        """The most recent run's summary, in stream units."""
        import ctypes as C
        s = (C.c_int64 * 8)()
        self._lib.check(self._lib.L.nnn_pack_last_summary(self._h, s))
        return dict(zip(PACK_SUMMARY, [int(v) for v in s]))

    def _table(self, files):
        t = (_ffi.PackFile * max(len(files), 1))()
        for i, f in enumerate(files):
            t[i] = _ffi.PackFile(*[int(v) for v in f])
        return t

    def run_arena(self, in_arena, in_format, out_arena, vad_arena, files):
        """One run over host arenas: in_arena (a C-contiguous array whose bytes are in_format elements), out_arena (int16 or float32,
        written in place), vad_arena (float32 or None), files = [(in_off, n_sample_frames, out_off, vad_off)] in elements.  Bytes of
        the output arenas outside the files' ranges stay as they were.  Returns the summary."""
        in_arena = np.ascontiguousarray(in_arena)
        if not (isinstance(out_arena, np.ndarray) and out_arena.dtype in (np.int16, np.float32) and out_arena.flags.c_contiguous and out_arena.flags.writeable):
            raise ValueError("run_arena: out_arena must be a writable C-contiguous int16 or float32 array")
        if vad_arena is not None and not (isinstance(vad_arena, np.ndarray) and vad_arena.dtype == np.float32 and vad_arena.flags.c_contiguous
                                          and vad_arena.flags.writeable):
            raise ValueError("run_arena: vad_arena must be a writable C-contiguous float32 array or None")
        out_format = PCM_I16 if out_arena.dtype == np.int16 else PCM_F32
        es = _ffi.PACK_ELEM_BYTES.get(in_format, 1)
        self._lib.check(self._lib.L.nnn_pack_run_host(self._h, _ffi.ptr(in_arena), in_arena.nbytes // es, int(in_format), _ffi.ptr(out_arena),
                                                      out_arena.size, out_format, _ffi.ptr(vad_arena), 0 if vad_arena is None else vad_arena.size,
                                                      self._table(files), len(files)))
        s = self.last_summary()
        self.batch.frames_done += s["launched"] // self.batch.n_streams
        return s

    def run_device(self, d_in, in_elems, in_format, d_out, out_elems, out_format, d_vad, vad_elems, files, hip_stream=0):
        """Raw device pointers (ints; d_vad 0 = no VAD), arena sizes in elements, files as run_arena takes them (or a ready
        _ffi.PackFile array); asynchronous on hip_stream (0 = the batch's own stream).  Returns the summary, which is host arithmetic."""
        table = files if isinstance(files, C.Array) else self._table(files)
        self._lib.check(self._lib.L.nnn_pack_run_device(self._h, d_in, int(in_elems), int(in_format), d_out, int(out_elems), int(out_format),
                                                        d_vad or None, int(vad_elems), table, len(files), hip_stream))
        s = self.last_summary()
        self.batch.frames_done += s["launched"] // self.batch.n_streams
        return s

    def debug_kernels(self, which, d_in, in_format, d_out, out_format, n_frames, reps, hip_stream=0):
        """Measuring hook: `reps` launches of k_pack_in (which = 0) or k_pack_out (1) alone over dense arenas (nnn_pack_debug_kernels)."""
        self._lib.check(self._lib.L.nnn_pack_debug_kernels(self._h, int(which), d_in or None, int(in_format), d_out or None, int(out_format),
                                                           int(n_frames), int(reps), hip_stream))

    def run(self, files, in_format=None, out_format=PCM_I16):
        """files: a list of arrays, each [n, channels] (or [n] for mono) -- int16 (PCM_I16), float32 (PCM_F32 in i16 range, or
        PACK_F32_WAV in [-1, 1] when in_format says so), int32 (PACK_I32) --, or for PACK_I24 uint8 [n * channels * 3] (packed
        little-endian); one format per run.  Returns (outputs, vads, summary): outputs[i] [(F_i - 1) * 480, channels] of out_format's
        dtype ([0, channels] for F_i <= 1), vads[i] [F_i, channels]."""
        Cc = self.channels
        if in_format is None:
            dt = np.asarray(files[0]).dtype if len(files) else np.dtype(np.int16)
            in_format = {np.dtype(np.int16): PCM_I16, np.dtype(np.float32): PCM_F32, np.dtype(np.int32): PACK_I32, np.dtype(np.uint8): PACK_I24}.get(dt)
            if in_format is None:
                raise ValueError(f"run: no input format for dtype {dt}")
        if in_format not in _PACK_IN_DTYPE:
            raise ValueError(f"run: unknown input format {in_format}")
        if out_format not in (PCM_I16, PCM_F32):
            raise ValueError("run: out_format must be PCM_I16 or PCM_F32")
        es = 3 if in_format == PACK_I24 else 1
        flat = [np.ascontiguousarray(f, dtype=_PACK_IN_DTYPE[in_format]).reshape(-1) for f in files]
        for f in flat:
            if f.size % (Cc * es):
                raise ValueError("run: a file is not a whole number of sample frames of all channels")
        n = [f.size // (Cc * es) for f in flat]
        F = [k // FRAME_SIZE for k in n]
        in_off = np.concatenate([[0], np.cumsum([f.size // es for f in flat])]).astype(np.int64)
        out_off = np.concatenate([[0], np.cumsum([max(k - 1, 0) * FRAME_SIZE * Cc for k in F])]).astype(np.int64)
        vad_off = np.concatenate([[0], np.cumsum([k * Cc for k in F])]).astype(np.int64)
        in_arena = np.concatenate(flat) if flat else np.zeros(0, _PACK_IN_DTYPE[in_format])
        out_arena = np.zeros(max(int(out_off[-1]), 1), _ffi.PCM_DTYPE[out_format])
        vad_arena = np.zeros(max(int(vad_off[-1]), 1), np.float32)
        if in_arena.size == 0:
            in_arena = np.zeros(4, _PACK_IN_DTYPE[in_format])
        s = self.run_arena(in_arena, in_format, out_arena, vad_arena, [(in_off[i], n[i], out_off[i], vad_off[i]) for i in range(len(flat))])
        outs = [out_arena[out_off[i]:out_off[i] + max(F[i] - 1, 0) * FRAME_SIZE * Cc].reshape(-1, Cc).copy() for i in range(len(flat))]
        vads = [vad_arena[vad_off[i]:vad_off[i] + F[i] * Cc].reshape(-1, Cc).copy() for i in range(len(flat))]
        return outs, vads, s

    def close(self):
        if getattr(self, "_h", None):
            self._lib.L.nnn_pack_destroy(self._h)
            self._h = None

    __del__ = close


def denoise_files(arrays, channels=1, model=None, n_streams=None, order="longest_first", in_format=None, out_format=PCM_I16, device=0, lib=None):
    """The reference CLI over a corpus: `arrays` (as FilePacker.run takes them, any mix of lengths) denoised in one packer run on a batch
    of `n_streams` streams (default: one slot per file that has a whole frame, 4096 streams at the most).  order = "longest_first"
    sorts the files by length, longest first, before they are packed -- the short ones then fill the slots the long ones leave, and
    the idle tail is shortest --, "given" keeps the list order.  Results come back in the caller's order whatever the packing order:
    (outputs, vads, summary); every file's bits are those of denoise_raw_i16(file, channels) for int16 in and out."""
    if order not in ("longest_first", "given"):
        raise ValueError('order must be "longest_first" or "given"')
    es = 3 if in_format == PACK_I24 else 1
    sizes = [np.asarray(a).size // (channels * es) for a in arrays]
    idx = sorted(range(len(arrays)), key=lambda i: -sizes[i]) if order == "longest_first" else list(range(len(arrays)))
    if n_streams is None:
        n_streams = channels * max(1, min(sum(1 for k in sizes if k >= FRAME_SIZE), max(1, 4096 // channels)))
    bd = BatchDenoiser(int(n_streams), model, device, lib)
    fp = FilePacker(bd, channels)
    try:
        outs, vads, s = fp.run([arrays[i] for i in idx], in_format, out_format)
    finally:
        fp.close()
        bd.close()
    back = {j: k for k, j in enumerate(idx)}
    return [outs[back[i]] for i in range(len(arrays))], [vads[back[i]] for i in range(len(arrays))], s
