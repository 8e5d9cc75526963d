"""nnnoiseless_amd -- MI355X-native batched backend for nnnoiseless' DenoiseState::process_frame.

Host-side mirror of the reference's public interface for this path (jneem/nnnoiseless v0.5.1):

  RnnModel      from_bytes / from_static_bytes / default          (src/rnn.rs:72-94, 235-240)
  DenoiseState  FRAME_SIZE, new / from_model / with_model, process_frame(output, input) -> vad
                                                                    (src/denoise.rs:44-116)
  BatchDenoiser n independent DenoiseStates advanced in lock-step (the per-channel loop of
                src/signal.rs:102-104 and src/nnnoiseless.rs:318-320 as one call)

All arithmetic runs in hand-written HIP kernels (csrc/nnn_kernels.hip and the stage files it
includes, one per stage: nnn_hp.hip ... nnn_synth.hip) behind the C ABI of
include/nnn_batch.h and include/rnnoise.h.  There is no CPU fallback: importing works anywhere,
but creating a state without the built library or without a GPU raises.
"""
import ctypes as C
import os

import numpy as np

# (Several batches ticking side by side overlap only when their streams land on different hardware queues; the HIP runtime has four unless
# GPU_MAX_HW_QUEUES says otherwise when it initialises.  That is the HOST's setting -- INTEGRATION.md -- and neither this package nor the
# library touches the environment: until round 4 both exported it silently.  bench.py and the tick tools export it themselves.)

from . import _ffi
from .build import LIB_PATH, build_library

FRAME_SIZE = 480
FREQ_SIZE = 481
NB_BANDS = 22
NB_FEATURES = 42
from ._ffi import STREAM_STATE_BYTES, STREAM_STATE_VERSION, stream_state_field  # noqa: E402  (per-stream state records)

_lib = None


def attenuation_limit_db(db):
    """The gain floor of an attenuation limit: "never take a band down by more than `db` dB" = 10 ** (-db / 20)
    (BatchDenoiser.set_gain_floor)."""
    return 10.0 ** (-float(db) / 20.0)


def library():
    """The hipcc-built gfx950 library (loaded on first use)."""
    global _lib
    if _lib is None:
        import os
        import sys
        # A process that also uses PyTorch holds two HIP runtimes (torch ships its own): torch's does not come up once the
        # system one is running ("No HIP GPUs are available"), the other order works.  If torch is already imported, bring its
        # device up first; a host that imports torch later has to do the same itself (torch.cuda.init()) before its first batch.
        t = sys.modules.get("torch")
        if t is not None:
            try:
                if t.cuda.is_available():
                    t.cuda.init()
            except Exception:
                pass
        _lib = _ffi.Library(os.environ.get("NNN_LIBRARY", LIB_PATH))   # developer override: an experimental build
    return _lib


class _Pinned:
    """Owner of one nnn_host_alloc block (freed with the last array that views it)."""

    def __init__(self, lib, nbytes):
        self._lib, self.nbytes = lib, int(nbytes)
        self.ptr = lib.L.nnn_host_alloc(self.nbytes)
        if not self.ptr:
            raise MemoryError("nnnoiseless_amd: " + lib.error())

    def __del__(self):
        if getattr(self, "ptr", None):
            self._lib.L.nnn_host_free(self.ptr)
            self.ptr = None


def pinned_empty(shape, dtype=np.float32, lib=None):
    """A numpy array in page-locked host memory (include/nnn_batch.h nnn_host_alloc): what BatchDenoiser.process /
    process_pcm transfer by DMA, uploads and downloads at the same time."""
    lib = lib or library()
    dt = np.dtype(dtype)
    n = int(np.prod(shape))
    own = _Pinned(lib, max(1, n * dt.itemsize))
    buf = (C.c_char * own.nbytes).from_address(own.ptr)
    buf._owner = own   # the ctypes view is the array's base: the block lives as long as any view of the array
    return np.frombuffer(buf, dtype=dt, count=n).reshape(shape)


class RnnModel:
    """Model parameters (reference: src/rnn.rs:54-62).  Constructors return None on malformed input
    exactly where the reference returns None."""

    def __init__(self, handle, lib):
        self._h, self._lib = handle, lib

    @classmethod
    def from_bytes(cls, data, lib=None):
        lib = lib or library()
        data = bytes(data)
        h = lib.L.nnn_model_from_bytes(data, len(data))
        return cls(h, lib) if h else None

    from_static_bytes = from_bytes

    @classmethod
    def from_rnnoise_text(cls, text, lib=None):
        """An RNNoise / rnnoise-nu text model (what train/convert_rnnoise.py turns into a .rnn file first)."""
        lib = lib or library()
        data = text.encode() if isinstance(text, str) else bytes(text)
        h = lib.L.nnn_model_from_rnnoise_text(data, len(data))
        return cls(h, lib) if h else None

    @classmethod
    def default(cls, lib=None):
        lib = lib or library()
        return cls(lib.L.nnn_model_default(), lib)

    def clone(self):
        """`RnnModel: Clone` (src/rnn.rs:54): an independent copy."""
        h = self._lib.L.nnn_model_clone(self._h)
        if not h:
            raise RuntimeError(self._lib.error())
        return RnnModel(h, self._lib)

    __copy__ = clone

    def shape(self):
        s = (C.c_int32 * 12)()
        self._lib.L.nnn_model_shape(self._h, s)
        return list(s)

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.L.nnn_model_free(self._h)
            self._h = None


class BatchDenoiser:
    """n_streams DenoiseStates in lock-step on one GPU."""

    def __init__(self, n_streams, model=None, device=0, lib=None, groups=None, taps=False, max_group_frames=None, _handle=None):
        """max_group_frames: the longest run of frames the kernels take at once (default 24).  A real-time host that ticks one frame
        per call passes 1: the batch then holds 33 KB per stream instead of 360 (`device_bytes()`); longer calls still work on it,
        cut into groups of that many frames.
        groups: [(model_or_None, n_streams), ...] keeps several models resident, one per run of streams (every run
        but the last a multiple of 64); it replaces `model` and must add up to n_streams.  taps=True also stores the
        intermediate quantities the kernels otherwise keep on chip (parity tests: everything inside the pitch kernel -- tap("xlp"),
        "xcorr1", "best1", "xcorr2c", "pitch_search" --, "P" beyond bin 399, "features")."""
        self._lib = lib or library()
        self._model = model
        self.n_streams = int(n_streams)
        self.frames_done = 0
        if _handle is not None:   # clone()
            self._h = _handle
            return
        if max_group_frames is not None and int(max_group_frames) < 1:
            raise ValueError("max_group_frames must be at least 1")
        if groups or max_group_frames is not None:
            groups_ = groups or [(model, self.n_streams)]
            if sum(n for _, n in groups_) != self.n_streams:
                raise ValueError("group sizes must add up to n_streams")
            if groups:
                self._model = [m for m, _ in groups_]
            hs = (C.c_void_p * len(groups_))(*[m._h if m is not None else None for m, _ in groups_])
            ns = (C.c_int * len(groups_))(*[int(n) for _, n in groups_])
            if max_group_frames is not None:
                opts = _ffi.BatchOpts(max_group_frames=int(max_group_frames))
                self._h = self._lib.L.nnn_batch_create_opts(hs, ns, len(groups_), device, C.byref(opts))
            else:
                self._h = self._lib.L.nnn_batch_create_grouped(hs, ns, len(groups_), device)
        else:
            self._h = self._lib.L.nnn_batch_create(model._h if model is not None else None, self.n_streams, device)
        if not self._h:
            raise RuntimeError("nnnoiseless_amd: " + self._lib.error())
        if taps:
            self.set_taps(True)

    def device_bytes(self):
        """Device memory the batch holds (state, scratch, tables, weights)."""
        return int(self._lib.L.nnn_batch_device_bytes(self._h))

    def max_group_frames(self):
        return int(self._lib.L.nnn_batch_max_group_frames(self._h))

    def clone(self):
        """A second batch with the same models and a copy of every stream's state (DenoiseState: Clone, src/denoise.rs:36)."""
        h = self._lib.L.nnn_batch_clone(self._h)
        if not h:
            raise RuntimeError("nnnoiseless_amd: " + self._lib.error())
        c = BatchDenoiser(self.n_streams, model=self._model, lib=self._lib, _handle=h)
        c.frames_done = self.frames_done
        return c

    def save_state(self):
        """The streams' state as bytes (a raw image: loads only into a batch of the same shape made by the same build)."""
        buf = np.empty(self._lib.L.nnn_batch_state_bytes(self._h), np.uint8)
        self._lib.check(self._lib.L.nnn_batch_save_state(self._h, _ffi.ptr(buf), buf.nbytes))
        return buf.tobytes()

    def load_state(self, data):
        buf = np.frombuffer(data, np.uint8)
        self._lib.check(self._lib.L.nnn_batch_load_state(self._h, _ffi.ptr(buf), buf.nbytes))

    def reset_streams(self, idx):
        """The listed streams back to DenoiseState::new() (include/nnn_batch.h nnn_batch_reset_streams); the others carry on untouched.
        Enqueued in order with the processing calls; returns at once."""
        a, p = _ffi.stream_list(idx)
        self._lib.check(self._lib.L.nnn_batch_reset_streams(self._h, p, a.size))

    def export_streams(self, idx):
        """The listed streams' state as portable records: uint8 [len(idx), STREAM_STATE_BYTES] (record i belongs to idx[i]), importable
        into any slot of any batch whose stream runs a model of the same GRU sizes."""
        a, p = _ffi.stream_list(idx)
        out = np.zeros((a.size, STREAM_STATE_BYTES), np.uint8)
        self._lib.check(self._lib.L.nnn_batch_export_streams(self._h, p, a.size, _ffi.ptr(out), out.nbytes))
        return out

    def import_streams(self, idx, records):
        """Stream idx[i] takes record i's state (from export_streams of this or any other batch, or DenoiseState.export_state)."""
        a, p = _ffi.stream_list(idx)
        r = _ffi.stream_records(records, a.size)
        self._lib.check(self._lib.L.nnn_batch_import_streams(self._h, p, a.size, _ffi.ptr(r), r.nbytes))

    def hold_streams(self, idx):
        """From the next processing call on the listed streams do not take part: their state is parked, their input is not read, their
        rows of `out` and `vad` are left as they were, and work that would serve only held streams is not done (include/nnn_batch.h
        nnn_batch_hold_streams).  Enqueued in order with the processing calls; returns at once."""
        a, p = _ffi.stream_list(idx)
        self._lib.check(self._lib.L.nnn_batch_hold_streams(self._h, p, a.size))

    def resume_streams(self, idx):
        """The listed held streams take part again from the next processing call on, exactly as if the calls in between had not
        happened for them."""
        a, p = _ffi.stream_list(idx)
        self._lib.check(self._lib.L.nnn_batch_resume_streams(self._h, p, a.size))

    def held(self):
        """bool [n_streams]: which streams are held."""
        m = np.zeros(self.n_streams, np.uint8)
        self._lib.check(self._lib.L.nnn_batch_held_mask(self._h, _ffi.ptr(m), m.size))
        return m.astype(bool)

    def num_held(self):
        return int(self._lib.L.nnn_batch_num_held(self._h))

    def set_gain_floor(self, idx, floors):
        """Gain floors of the listed streams (include/nnn_batch.h nnn_batch_set_gain_floor): in every processing call a non-silent frame's
        raw network gain becomes max(gain, floor) before the pitch filter and the smoothing see it.  floors: a scalar (every listed
        stream, all 22 bands), [len(idx)] (one value per stream) or [len(idx), 22]; 0 = off; attenuation_limit_db(18) = "never more than
        18 dB down".  Configuration, not state: floors survive resets, imports, hold / resume and load_state, and clone() copies them.
        Enqueued in order with the processing calls; returns at once."""
        a, p = _ffi.stream_list(idx)
        f, bands = _ffi.gain_floors(floors, a.size)
        self._lib.check(self._lib.L.nnn_batch_set_gain_floor(self._h, p, a.size, f.ctypes.data_as(C.POINTER(C.c_float)), bands))

    def gain_floor(self, idx=None):
        """float32 [len(idx), 22]: the listed streams' floors (idx=None: every stream's).  Waits for the batch's work."""
        a, p = _ffi.stream_list(range(self.n_streams) if idx is None else idx)
        out = np.zeros((a.size, NB_BANDS), np.float32)
        self._lib.check(self._lib.L.nnn_batch_get_gain_floor(self._h, p, a.size, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def num_floored(self):
        """Streams with any floor above 0."""
        return int(self._lib.L.nnn_batch_num_floored(self._h))

    def set_channel_link(self, channels, mode="max"):
        """Link the channels of every stream group (include/nnn_batch.h nnn_batch_set_channel_link): streams s with the same s // channels
        -- the channels of one stereo or four-channel group at the PCM boundary -- get one common gain per band, the largest ("max": a
        band is kept if any channel's network keeps it) or the smallest ("min") of their network outputs, before the floor, the pitch
        filter and the smoothing see it; silent frames and held streams neither give nor take.  channels 2 or 4; channels 1 or mode "off"
        switches it off.  Configuration, not state: it survives resets, imports, hold / resume and load_state, and clone() copies it.
        Takes effect from the next processing call; returns at once."""
        self._lib.check(self._lib.L.nnn_batch_set_channel_link(self._h, int(channels), _ffi.link_mode(mode)))

    def channel_link(self):
        """(channels, mode) the next processing call runs under: (1, "off") while off."""
        ch, md = C.c_int32(0), C.c_int32(0)
        self._lib.check(self._lib.L.nnn_batch_get_channel_link(self._h, C.byref(ch), C.byref(md)))
        return ch.value, _ffi.link_mode_name(md.value)

    def export_streams_device(self, idx, d_dst, hip_stream=0):
        """Records into device memory at d_dst (an int, len(idx) * STREAM_STATE_BYTES bytes); asynchronous on hip_stream."""
        a, p = _ffi.stream_list(idx)
        self._lib.check(self._lib.L.nnn_batch_export_streams_device(self._h, p, a.size, d_dst, hip_stream))

    def import_streams_device(self, idx, d_src, hip_stream=0):
        """Records from device memory at d_src; asynchronous.  The records are checked on the device: a list with a bad record
        writes nothing, and the next synchronize() raises."""
        a, p = _ffi.stream_list(idx)
        self._lib.check(self._lib.L.nnn_batch_import_streams_device(self._h, p, a.size, d_src, hip_stream))

    def set_taps(self, on):
        self._lib.check(self._lib.L.nnn_batch_set_taps(self._h, int(on)))

    def set_schedule(self, mode, lanes=0):
        """mode: "seq" | "lanes" | "stages" (include/nnn_batch.h nnn_batch_set_schedule)."""
        self._lib.check(self._lib.L.nnn_batch_set_schedule(self._h, {"seq": 0, "lanes": 1, "stages": 2}[mode], int(lanes)))

    def process(self, x, out=None, vad=None):
        """x: float32 [n_streams, n_frames, 480] on the host -> (out same shape, vad [n_frames, n_streams]).  Arrays from
        pinned_empty (x, and out / vad handed in) cross the bus by DMA."""
        x = _ffi.as_f32(x)
        if x.ndim != 3 or x.shape[0] != self.n_streams or x.shape[2] != FRAME_SIZE:
            raise ValueError(f"process needs x of shape [{self.n_streams}, n_frames, {FRAME_SIZE}], got {x.shape}")
        S, T, F = x.shape
        out = np.empty_like(x) if out is None else out
        vad = np.empty((T, S), np.float32) if vad is None else vad
        # caller-supplied buffers are written by the C library: a wrong size or layout must never get that far
        if not (isinstance(out, np.ndarray) and out.shape == x.shape and out.dtype == np.float32 and out.flags.c_contiguous and out.flags.writeable):
            raise ValueError("process: `out` must be a writable C-contiguous float32 array of x's shape")
        if not (isinstance(vad, np.ndarray) and vad.shape == (T, S) and vad.dtype == np.float32 and vad.flags.c_contiguous and vad.flags.writeable):
            raise ValueError("process: `vad` must be a writable C-contiguous float32 array of shape [n_frames, n_streams]")
        self._lib.check(self._lib.L.nnn_batch_process_host(self._h, _ffi.ptr(x), _ffi.ptr(out), _ffi.ptr(vad), T,
                                                           T * FRAME_SIZE, FRAME_SIZE))
        self.frames_done += T
        return out, vad

    def process_pcm(self, x, fmt, channels=1, discard_first=False, out=None, vad=None):
        """Packed PCM in the reference callers' formats, x: [n_groups, n_frames * 480, channels] (int16 for PCM_I16,
        float32 otherwise), n_groups * channels == n_streams.  Returns (out [n_groups, n_out_frames * 480, channels],
        vad [n_frames, n_streams]); n_out_frames = n_frames - 1 if discard_first drops the first frame after a reset.  `out` (x's shape
        and dtype) and `vad`, when handed in, are written in place: what held streams own in them stays as it was."""
        x = np.ascontiguousarray(x, dtype=_ffi.PCM_DTYPE[fmt])
        if x.ndim != 3 or x.shape[2] != channels or x.shape[0] * channels != self.n_streams or x.shape[1] % FRAME_SIZE:
            raise ValueError(f"process_pcm needs x of shape [n_streams / channels, n_frames * {FRAME_SIZE}, channels], got {x.shape}")
        G, N, Cc = x.shape
        T = N // FRAME_SIZE
        out = np.zeros_like(x) if out is None else out
        vad = np.empty((T, self.n_streams), np.float32) if vad is None else vad
        if not (isinstance(out, np.ndarray) and out.shape == x.shape and out.dtype == x.dtype and out.flags.c_contiguous and out.flags.writeable):
            raise ValueError("process_pcm: `out` must be a writable C-contiguous array of x's shape and dtype")
        if not (isinstance(vad, np.ndarray) and vad.shape == (T, self.n_streams) and vad.dtype == np.float32 and vad.flags.c_contiguous and vad.flags.writeable):
            raise ValueError("process_pcm: `vad` must be a writable C-contiguous float32 array of shape [n_frames, n_streams]")
        L = _ffi.PcmLayout(fmt, channels, int(bool(discard_first)), 0, N * channels, FRAME_SIZE * channels)
        fresh = self.frames_done == 0
        self._lib.check(self._lib.L.nnn_batch_process_pcm_host(self._h, _ffi.ptr(x), _ffi.ptr(out), _ffi.ptr(vad), T, C.byref(L)))
        self.frames_done += T
        n_out = T - 1 if (discard_first and fresh) else T
        return out[:, :n_out * FRAME_SIZE], vad

    def process_device(self, d_in, d_out, d_vad, n_frames, stream_stride, frame_stride, hip_stream=0):
        """Raw device pointers (ints); asynchronous on hip_stream (0 = the batch's own stream)."""
        self._lib.check(self._lib.L.nnn_batch_process_device(self._h, d_in, d_out, d_vad, n_frames, stream_stride,
                                                             frame_stride, hip_stream))
        self.frames_done += n_frames

    def process_pcm_device(self, d_in, d_out, d_vad, n_frames, fmt, channels, group_stride, frame_stride, discard_first=False,
                           hip_stream=0):
        """Raw device pointers, strides in elements of the format (include/nnn_batch.h); asynchronous."""
        L = _ffi.PcmLayout(fmt, channels, int(bool(discard_first)), 0, group_stride, frame_stride)
        self._lib.check(self._lib.L.nnn_batch_process_pcm_device(self._h, d_in, d_out, d_vad, n_frames, C.byref(L), hip_stream))
        self.frames_done += n_frames

    # ---- split calls: features out, the caller's gains in (include/nnn_batch.h "Split calls") ----
    def _pcm_shape(self, what, x, fmt, channels):
        """The audio conventions of process (fmt None: float32 [n_streams, n_frames, 480]) and process_pcm (packed
        [n_streams / channels, n_frames * 480, channels]): (array, format, channels, frames, group stride)."""
        if fmt is None:
            x = _ffi.as_f32(x)
            if x.ndim != 3 or x.shape[0] != self.n_streams or x.shape[2] != FRAME_SIZE:
                raise ValueError(f"{what} needs audio of shape [{self.n_streams}, n_frames, {FRAME_SIZE}], got {x.shape}")
            return x, _ffi.PCM_F32, 1, x.shape[1], x.shape[1] * FRAME_SIZE
        x = np.ascontiguousarray(x, dtype=_ffi.PCM_DTYPE[fmt])
        if x.ndim != 3 or x.shape[2] != channels or x.shape[0] * channels != self.n_streams or x.shape[1] % FRAME_SIZE:
            raise ValueError(f"{what} needs audio of shape [n_streams / channels, n_frames * {FRAME_SIZE}, channels], got {x.shape}")
        return x, fmt, channels, x.shape[1] // FRAME_SIZE, x.shape[1] * channels

    def analyze(self, x, fmt=None, channels=1, features=None, silence=None):
        """The first half of process_frame for up to max_group_frames() frames: x as process takes it (fmt None) or as process_pcm does
        (fmt, channels) -> (features float32 [n_frames, n_streams, 42], silence int32 [n_frames, n_streams]).  The frames are pending
        until synthesize() is given their gains.  `features` / `silence`, when handed in, are written in place: held streams' rows stay."""
        x, fmt, channels, T, gstride = self._pcm_shape("analyze", x, fmt, channels)
        S = self.n_streams
        features = np.zeros((T, S, NB_FEATURES), np.float32) if features is None else features
        silence = np.zeros((T, S), np.int32) if silence is None else silence
        for a, shp, dt, name in ((features, (T, S, NB_FEATURES), np.float32, "features"), (silence, (T, S), np.int32, "silence")):
            if not (isinstance(a, np.ndarray) and a.shape == shp and a.dtype == dt and a.flags.c_contiguous and a.flags.writeable):
                raise ValueError(f"analyze: `{name}` must be a writable C-contiguous {np.dtype(dt).name} array of shape {list(shp)}")
        L = _ffi.PcmLayout(fmt, channels, 0, 0, gstride, FRAME_SIZE * channels)
        self._lib.check(self._lib.L.nnn_batch_analyze_host(self._h, _ffi.ptr(x), _ffi.ptr(features), _ffi.ptr(silence), T, C.byref(L)))
        return features, silence

    def synthesize(self, gains, vad=None, fmt=None, channels=1, discard_first=False, out=None):
        """The second half for the pending frames: gains float32 [n_frames, n_streams, 22] (vad [n_frames, n_streams], optional: the
        network's VAD, kept for tap("vad")) -> audio in the convention analyze read it in (process's for fmt None, process_pcm's
        otherwise, discard_first as there).  `out`, when handed in, is written in place: what held streams own in it stays."""
        gains = _ffi.as_f32(gains)
        S = self.n_streams
        if gains.ndim != 3 or gains.shape[1:] != (S, NB_BANDS):
            raise ValueError(f"synthesize needs gains of shape [n_frames, {S}, {NB_BANDS}], got {gains.shape}")
        T = gains.shape[0]
        if vad is not None:
            vad = _ffi.as_f32(vad)
            if vad.shape != (T, S):
                raise ValueError(f"synthesize: `vad` must have shape [{T}, {S}], got {vad.shape}")
        if fmt is None:
            fmt_, channels, shape, dt = _ffi.PCM_F32, 1, (S, T, FRAME_SIZE), np.float32
        else:
            if channels < 1 or S % channels:
                raise ValueError("n_streams must be a multiple of channels")
            fmt_, shape, dt = fmt, (S // channels, T * FRAME_SIZE, channels), _ffi.PCM_DTYPE[fmt]
        out = np.zeros(shape, dt) if out is None else out
        if not (isinstance(out, np.ndarray) and out.shape == shape and out.dtype == dt and out.flags.c_contiguous and out.flags.writeable):
            raise ValueError(f"synthesize: `out` must be a writable C-contiguous {np.dtype(dt).name} array of shape {list(shape)}")
        L = _ffi.PcmLayout(fmt_, channels, int(bool(discard_first)), 0, T * FRAME_SIZE * channels, FRAME_SIZE * channels)
        fresh = self.frames_done == 0
        self._lib.check(self._lib.L.nnn_batch_synthesize_host(self._h, _ffi.ptr(gains), _ffi.ptr(vad), _ffi.ptr(out), T, C.byref(L)))
        self.frames_done += T
        if fmt is None:
            return out
        return out[:, :(T - 1 if (discard_first and fresh) else T) * FRAME_SIZE]

    def analyze_device(self, d_in, d_features, d_silence, n_frames, fmt, channels, group_stride, frame_stride, hip_stream=0):
        """Raw device pointers (ints), strides in elements of the format; asynchronous on hip_stream (0 = the batch's own stream)."""
        L = _ffi.PcmLayout(fmt, channels, 0, 0, group_stride, frame_stride)
        self._lib.check(self._lib.L.nnn_batch_analyze_device(self._h, d_in, d_features, d_silence, n_frames, C.byref(L), hip_stream))

    def synthesize_device(self, d_gains, d_vad, d_out, n_frames, fmt, channels, group_stride, frame_stride, discard_first=False, hip_stream=0):
        """Raw device pointers (d_vad may be None); asynchronous."""
        L = _ffi.PcmLayout(fmt, channels, int(bool(discard_first)), 0, group_stride, frame_stride)
        self._lib.check(self._lib.L.nnn_batch_synthesize_device(self._h, d_gains, d_vad, d_out, n_frames, C.byref(L), hip_stream))
        self.frames_done += n_frames

    def pending_frames(self):
        """Frames analysed and not yet synthesised (0 = none)."""
        return int(self._lib.L.nnn_batch_pending_frames(self._h))

    # ---- VAD only: the speech probability without the denoiser (include/nnn_batch.h "VAD-only calls") ----
    def vad(self, x, fmt=None, channels=1, vad=None):
        """The VAD of up to max_group_frames() frames and nothing else: x as process takes it (fmt None) or as process_pcm does (fmt,
        channels) -> float32 [n_frames, n_streams], the values process would return.  No audio is produced; synthesis_mem, lastg and the
        noise / denoise GRU states stay as they are.  `vad`, when handed in, is written in place: held streams' entries stay."""
        x, fmt, channels, T, gstride = self._pcm_shape("vad", x, fmt, channels)
        S = self.n_streams
        vad = np.zeros((T, S), np.float32) if vad is None else vad
        if not (isinstance(vad, np.ndarray) and vad.shape == (T, S) and vad.dtype == np.float32 and vad.flags.c_contiguous and vad.flags.writeable):
            raise ValueError(f"vad: `vad` must be a writable C-contiguous float32 array of shape [{T}, {S}]")
        L = _ffi.PcmLayout(fmt, channels, 0, 0, gstride, FRAME_SIZE * channels)
        self._lib.check(self._lib.L.nnn_batch_vad_host(self._h, _ffi.ptr(x), _ffi.ptr(vad), T, C.byref(L)))
        self.frames_done += T
        return vad

    def vad_device(self, d_in, d_vad, n_frames, fmt, channels, group_stride, frame_stride, hip_stream=0):
        """Raw device pointers (ints), strides in elements of the format; asynchronous on hip_stream (0 = the batch's own stream)."""
        L = _ffi.PcmLayout(fmt, channels, 0, 0, group_stride, frame_stride)
        self._lib.check(self._lib.L.nnn_batch_vad_device(self._h, d_in, d_vad, n_frames, C.byref(L), hip_stream))
        self.frames_done += n_frames

    # ---- network only: features in, raw gains and VAD out (include/nnn_batch.h "Network-only calls") ----
    def network(self, features, silence=None, gains=None, vad=None):
        """RnnState::compute of every stream's resident model on feature rows: features float32 [n_frames, n_streams, 42] (silence int32
        [n_frames, n_streams] as analyze returns it, None: no frame is silent) -> (raw gains float32 [n_frames, n_streams, 22], vad
        [n_frames, n_streams]).  Any n_frames >= 1; allowed between analyze and synthesize; moves the three GRU states and nothing else.
        `gains` / `vad`, when handed in, are written in place: held streams' rows stay."""
        features = _ffi.as_f32(features)
        S = self.n_streams
        if features.ndim != 3 or features.shape[0] < 1 or features.shape[1:] != (S, NB_FEATURES):
            raise ValueError(f"network needs features of shape [n_frames >= 1, {S}, {NB_FEATURES}], got {features.shape}")
        T = features.shape[0]
        if silence is not None:
            silence = np.ascontiguousarray(silence, dtype=np.int32)
            if silence.shape != (T, S):
                raise ValueError(f"network: `silence` must have shape [{T}, {S}], got {silence.shape}")
        gains = np.zeros((T, S, NB_BANDS), np.float32) if gains is None else gains
        vad = np.zeros((T, S), np.float32) if vad is None else vad
        for a, shp, name in ((gains, (T, S, NB_BANDS), "gains"), (vad, (T, S), "vad")):
            if not (isinstance(a, np.ndarray) and a.shape == shp and a.dtype == np.float32 and a.flags.c_contiguous and a.flags.writeable):
                raise ValueError(f"network: `{name}` must be a writable C-contiguous float32 array of shape {list(shp)}")
        self._lib.check(self._lib.L.nnn_batch_network_host(self._h, _ffi.ptr(features), _ffi.ptr(silence), _ffi.ptr(gains), _ffi.ptr(vad), T))
        return gains, vad

    def network_device(self, d_features, d_silence, d_gains, d_vad, n_frames, hip_stream=0):
        """Raw device pointers (ints; d_silence and d_vad may be None); asynchronous on hip_stream (0 = the batch's own stream)."""
        self._lib.check(self._lib.L.nnn_batch_network_device(self._h, d_features, d_silence, d_gains, d_vad, n_frames, hip_stream))

    def synchronize(self):
        self._lib.check(self._lib.L.nnn_batch_synchronize(self._h))

    def reset(self):
        self._lib.check(self._lib.L.nnn_batch_reset(self._h))
        self.frames_done = 0

    def tap(self, name):
        """Intermediate quantity of the most recent frame as [n_streams, len] (parity checks)."""
        t = _ffi.TAPS.index(name)
        ln, isint = C.c_int(), C.c_int()
        self._lib.check(self._lib.L.nnn_tap_info(t, C.byref(ln), C.byref(isint)))
        a = np.empty((self.n_streams, ln.value), np.int32 if isint.value else np.float32)
        self._lib.check(self._lib.L.nnn_batch_read_tap(self._h, t, _ffi.ptr(a), a.nbytes))
        return a

    def set_profiling(self, on):
        self._lib.check(self._lib.L.nnn_batch_set_profiling(self._h, int(on)))

    def set_graph(self, on):
        self._lib.check(self._lib.L.nnn_batch_set_graph(self._h, int(on)))

    def set_back_end(self, mode):
        """-1 (default): by batch size, as measured -- one-frame groups take the fused back end (k_back) up to 8192 streams and its RNN
        stretch alone above that or with other batches ticking on the same device, longer groups three launches; 0: transforms -> RNN ->
        synthesis as three launches; 1: one-frame groups take the fused back end; 2: every group; 3 / 4: the fused kernel's RNN stretch
        alone as the RNN kernel for one-frame / all groups (include/nnn_batch.h nnn_batch_set_back_end).  Every choice gives the same bits."""
        self._lib.check(self._lib.L.nnn_batch_set_back_end(self._h, int(mode)))

    def set_pipeline(self, on):
        self._lib.check(self._lib.L.nnn_batch_set_pipeline(self._h, int(on)))

    def set_inputs_ready(self, on):
        """Promise that the input of every process_device call is final when the call is made: consecutive calls may then
        overlap at their boundary (include/nnn_batch.h).  Outputs stay ordered on the caller's stream; same bits."""
        self._lib.check(self._lib.L.nnn_batch_set_inputs_ready(self._h, int(on)))

    def set_frame_log(self, d_log, frames):
        """Record (pitch index, branch mask, 22 smoothed gains) of the next `frames` frames into device memory at `d_log`
        (an int: [frames][n_streams][24] 32-bit words; include/nnn_batch.h nnn_batch_set_frame_log).  Parity tests."""
        self._lib.check(self._lib.L.nnn_batch_set_frame_log(self._h, d_log, int(frames)))

    def fault(self):
        """True once a pitch workgroup has given up waiting for the previous frame's hand-off (include/nnn_batch.h nnn_batch_fault):
        sticky until reset() / load_state().  A cheap host-memory read; no synchronisation."""
        fn = getattr(self._lib.L, "nnn_batch_fault", None)   # (absent from experimental builds of older sources: NNN_LIBRARY)
        return bool(fn(self._h)) if fn else False

    def kernel_times(self):
        """{kernel: (total_ms, launches)} accumulated while profiling; resets the counters."""
        n = self._lib.L.nnn_batch_num_kernels()
        ms = (C.c_double * n)()
        cnt = (C.c_int64 * n)()
        self._lib.check(self._lib.L.nnn_batch_read_kernel_times(self._h, ms, cnt, n))
        return {self._lib.L.nnn_batch_kernel_name(k).decode(): (ms[k], cnt[k]) for k in range(n)}

    def close(self):
        if getattr(self, "_h", None):
            self._lib.L.nnn_batch_destroy(self._h)
            self._h = None

    __del__ = close


class DenoiseState:
    """One stream (reference: src/denoise.rs:36-116); a batch of one on the GPU."""

    FRAME_SIZE = FRAME_SIZE

    def __init__(self, model=None, device=0, lib=None, _batch=None):
        # process_frame takes one frame per call: a batch sized for one-frame groups
        self._b = _batch if _batch is not None else BatchDenoiser(1, model, device, lib, max_group_frames=1)

    def clone(self):
        """`impl Clone for DenoiseState` (src/denoise.rs:36)."""
        return DenoiseState(_batch=self._b.clone())

    def export_state(self):
        """This state as a portable record (uint8 [STREAM_STATE_BYTES], include/nnn_batch.h): importable into a batch slot."""
        return self._b.export_streams([0])[0]

    @classmethod
    def from_state(cls, record, model=None, device=0, lib=None):
        """A state that continues from `record` (a batch slot's export_streams row, or export_state)."""
        st = cls(model, device=device, lib=lib)
        st._b.import_streams([0], np.asarray(record, np.uint8).reshape(1, -1))
        return st

    @classmethod
    def new(cls, **kw):
        return cls(None, **kw)

    @classmethod
    def from_model(cls, model, **kw):
        return cls(model, **kw)

    with_model = from_model

    def process_frame(self, output, input):
        """Writes 480 samples into `output`, returns the VAD probability (src/denoise.rs:95-116)."""
        input = _ffi.as_f32(input)
        if input.shape != (FRAME_SIZE,) or output.shape != (FRAME_SIZE,):
            raise ValueError("process_frame needs slices of length DenoiseState.FRAME_SIZE")  # src/features.rs:98
        out, vad = self._b.process(input.reshape(1, 1, FRAME_SIZE))
        output[:] = out[0, 0]
        return float(vad[0, 0])


from .node import NodeDenoiser  # noqa: E402  (all the GPUs of a node behind one object, include/nnn_node.h)
