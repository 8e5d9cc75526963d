"""The VAD gate (include/nnn_gate.h): the step a voice server puts behind the denoiser.

VadGate mirrors the C object: per stream a threshold on the speech probability, a grace period that keeps the gate open after speech, a
look-back that delays the audio a few frames so the onset that made the VAD fire is not cut, and a gain for the closed gate (0 = mute).
The rule is exact (integer counters, comparisons, at most one f32 subtract, multiply and add per sample) and stated in the header.
"""
import numpy as np

from . import FRAME_SIZE, _ffi, library

MAX_LOOKBACK = _ffi.GATE_MAX_LOOKBACK
MAX_GRACE = _ffi.GATE_MAX_GRACE
NEVER = _ffi.GATE_NEVER
STATE_BYTES = _ffi.GATE_STATE_BYTES


def _is_torch(a):
    return type(a).__module__.split(".")[0] == "torch"


class VadGate:
    """n_streams gates.  Audio is float32 [n_streams, n_frames, 480], vad float32 [n_frames, n_streams] as BatchDenoiser.process returns
    them; live is uint8 / bool [n_streams] (0 = the stream sits the call out); open flags are uint8 [n_frames, n_streams].  The delivered
    audio is the input `lookback` frames late; to drain a stream feed it `lookback` more frames with vad below its threshold."""

    def __init__(self, n_streams, max_lookback=0, device=0, lib=None):
        self._lib = lib or library()
        if not hasattr(self._lib.L, "nnn_gate_create"):
            raise RuntimeError("nnnoiseless_amd: this build of the library has no VAD gate (nnn_gate_*)")
        self.n_streams, self.max_lookback, self.device = int(n_streams), int(max_lookback), int(device)
        self._h = self._lib.L.nnn_gate_create(self.n_streams, self.max_lookback, self.device)
        if not self._h:
            raise RuntimeError("nnnoiseless_amd: " + self._lib.error())
        self._side = None   # a torch stream for calls made on torch's default stream (made on first use)

    def _idx(self, idx):
        if idx is None:
            return None, self.n_streams
        a, p = _ffi.stream_list(idx)
        self._keep = a
        return p, a.size

    def set_params(self, threshold, grace, lookback, level, idx=None):
        """The parameters of the listed streams (idx None: of every stream); each a scalar for all of them or one value per listed stream.
        Also resets those streams.  threshold and level in [0, 1], grace 0 .. MAX_GRACE frames, lookback 0 .. max_lookback frames."""
        p, n = self._idx(idx)
        rec = np.zeros(n, _ffi.GATE_PARAMS_DTYPE)
        for name, v, dt in (("threshold", threshold, np.float32), ("grace", grace, np.int64), ("lookback", lookback, np.int64), ("level", level, np.float32)):
            v = np.asarray(v, dtype=dt)
            v = np.full(n, v, dt) if v.ndim == 0 else v.reshape(-1)
            if v.size != n:
                raise ValueError(f"need {n} values of {name}, got {v.size}")
            if dt is np.int64 and v.size and (v.min() < -2 ** 31 or v.max() >= 2 ** 31):
                raise ValueError(f"{name} out of int32 range")
            rec[name] = v
        self._lib.check(self._lib.L.nnn_gate_set_params(self._h, p, n, _ffi.ptr(rec)))

    def params(self, idx=None):
        """A structured array (threshold, grace, lookback, level) of the listed streams."""
        p, n = self._idx(idx)
        rec = np.zeros(n, _ffi.GATE_PARAMS_DTYPE)
        self._lib.check(self._lib.L.nnn_gate_get_params(self._h, p, n, _ffi.ptr(rec)))
        return rec

    def reset(self, idx=None):
        """The listed streams (None: all) back to "never voiced, closed, no history"; the parameters stay."""
        p, n = self._idx(idx)
        self._lib.check(self._lib.L.nnn_gate_reset(self._h, p, n))

    def apply(self, audio, vad, live=None, out=None, want_open=False):
        """One call over n_frames frames of every stream.

        NumPy arrays: audio float32 [n_streams, n_frames, 480] on the host, synchronous; returns a new array, or writes `out` (which may
        be `audio` itself).  torch tensors on the object's device: enqueued behind the kernels that made them on torch's current stream,
        and what torch enqueues there afterwards comes behind the call (on the default stream, whose handle the C ABI reads as "the
        object's own stream", through a side stream that waits for it and that it waits for);
        audio must be dense in its last axis ([n_streams, n_frames, 480] with any strides that are whole floats, e.g. a permuted view of
        the batch's [n_frames, n_streams, 480]); out None means in place.  Returns out, or (out, open) with want_open."""
        if _is_torch(audio):
            return self._apply_torch(audio, vad, live, out, want_open)
        x = _ffi.as_f32(audio)
        if x.ndim != 3 or x.shape[0] != self.n_streams or x.shape[2] != FRAME_SIZE:
            raise ValueError(f"apply needs audio of shape [{self.n_streams}, n_frames, {FRAME_SIZE}], got {x.shape}")
        T = x.shape[1]
        v = _ffi.as_f32(vad)
        if v.shape != (T, self.n_streams):
            raise ValueError("vad must have shape [n_frames, n_streams]")
        out = np.empty_like(x) if out is None else out
        if not (isinstance(out, np.ndarray) and out.shape == x.shape and out.dtype == np.float32 and out.flags.c_contiguous and out.flags.writeable):
            raise ValueError("apply: `out` must be a writable C-contiguous float32 array of the audio's shape")
        lv = None
        if live is not None:
            lv = np.ascontiguousarray(np.asarray(live) != 0, dtype=np.uint8)
            if lv.shape != (self.n_streams,):
                raise ValueError("live must have shape [n_streams]")
        op = np.zeros((T, self.n_streams), np.uint8) if want_open else None
        self._lib.check(self._lib.L.nnn_gate_apply_host(self._h, _ffi.ptr(x), _ffi.ptr(out), _ffi.ptr(v), _ffi.ptr(lv), _ffi.ptr(op), T))
        return (out, op) if want_open else out

    def _apply_torch(self, audio, vad, live, out, want_open):
        import torch
        S = self.n_streams
        if audio.dtype != torch.float32 or audio.dim() != 3 or audio.shape[0] != S or audio.shape[2] != FRAME_SIZE or audio.stride(2) != 1:
            raise ValueError(f"apply needs a float32 tensor [{S}, n_frames, {FRAME_SIZE}] that is dense in its last axis")
        T = audio.shape[1]
        out = audio if out is None else out
        if out is not audio and (out.dtype != torch.float32 or out.shape != audio.shape or out.stride() != audio.stride()):
            raise ValueError("apply: `out` must be a float32 tensor of the audio's shape and strides")
        if vad.dtype != torch.float32 or tuple(vad.shape) != (T, S) or not vad.is_contiguous():
            raise ValueError("vad must be a contiguous float32 tensor [n_frames, n_streams]")
        if T > 1 and audio.stride(1) < FRAME_SIZE:
            raise ValueError("apply: the audio's frames overlap")
        lv = None
        if live is not None:
            lv = torch.as_tensor(live, device=audio.device)
            lv = (lv != 0).to(torch.uint8).contiguous()
            if tuple(lv.shape) != (S,):
                raise ValueError("live must have shape [n_streams]")
        op = torch.zeros((T, S), dtype=torch.uint8, device=audio.device) if want_open else None
        cur = torch.cuda.current_stream(audio.device)
        run = cur
        if cur.cuda_stream == 0:
            # torch's default stream has handle 0, which the C ABI reads as "the object's own stream" -- a non-blocking stream that is
            # ordered with nothing of torch's.  So the call goes on a stream of torch's that this object keeps, behind everything
            # enqueued on the default stream so far, and the default stream waits for it.
            if self._side is None:
                self._side = torch.cuda.Stream(device=audio.device)
            run = self._side
            run.wait_stream(cur)
        self.apply_device(audio.data_ptr(), out.data_ptr(), vad.data_ptr(), T, audio.stride(0), max(audio.stride(1), FRAME_SIZE),
                          d_live=None if lv is None else lv.data_ptr(), d_open=None if op is None else op.data_ptr(), hip_stream=run.cuda_stream)
        if run is not cur:
            cur.wait_stream(run)
        for t in (audio, out, vad, lv, op):            # (the caching allocator must not hand their memory on before the call has run)
            if t is not None:
                t.record_stream(run)
        return (out, op) if want_open else out

    def apply_device(self, d_in, d_out, d_vad, n_frames, stream_stride, frame_stride, d_live=None, d_open=None, hip_stream=0):
        """Raw device pointers (include/nnn_gate.h); asynchronous.  Strides in floats; d_out == d_in is in place."""
        self._lib.check(self._lib.L.nnn_gate_apply_device(self._h, d_in, d_out, d_vad, d_live, d_open, n_frames, stream_stride, frame_stride, hip_stream))

    def apply_pcm_device(self, d_in, d_out, d_vad, n_frames, fmt, channels, group_stride, frame_stride, d_live=None, d_open=None, hip_stream=0):
        """The packed boundary of BatchDenoiser.process_pcm_device: PCM_F32, PCM_F32_UNIT or PCM_I16, strides in elements."""
        import ctypes as C
        L = _ffi.PcmLayout(fmt, channels, 0, 0, group_stride, frame_stride)
        self._lib.check(self._lib.L.nnn_gate_apply_pcm_device(self._h, d_in, d_out, d_vad, d_live, d_open, n_frames, C.byref(L), hip_stream))

    def process(self, batch, x, out=None, vad=None, want_open=False):
        """One BatchDenoiser.process call on x (float32 [n_streams, n_frames, 480] on the host; out and vad as process takes them), then
        the gate in place on its output with the batch's held mask as `live`: what held streams own in out and vad is left as it was.
        Returns (out, vad), or (out, vad, open) with want_open.  A convenience for host arrays, not the device path: the audio crosses
        the bus for the batch and once more for the gate.  A server keeps it resident: process_device, then apply_device on the same
        buffers and stream."""
        out, vad = batch.process(x, out=out, vad=vad)
        held = batch.held()
        res = self.apply(out, vad, live=None if not held.any() else ~held, out=out, want_open=want_open)
        return (out, vad, res[1]) if want_open else (out, vad)

    def export_streams(self, idx):
        """The listed streams' records: uint8 [len(idx), STATE_BYTES] (parameters, since, was_open, history; view them with
        _ffi.GATE_STATE_DTYPE).  Waits for the calls made so far."""
        p, n = self._idx(range(self.n_streams) if idx is None else idx)
        rec = np.zeros((n, STATE_BYTES), np.uint8)
        self._lib.check(self._lib.L.nnn_gate_export_streams(self._h, p, n, _ffi.ptr(rec), rec.nbytes))
        return rec

    def import_streams(self, idx, records):
        """Records of export_streams (of any gate object) into the listed streams: they continue bit for bit."""
        p, n = self._idx(range(self.n_streams) if idx is None else idx)
        rec = np.ascontiguousarray(records, dtype=np.uint8)
        if rec.size != n * STATE_BYTES:
            raise ValueError(f"need {n} records of {STATE_BYTES} bytes, got {rec.size} bytes")
        self._lib.check(self._lib.L.nnn_gate_import_streams(self._h, p, n, _ffi.ptr(rec), rec.nbytes))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.L.nnn_gate_destroy(self._h)
            self._h = None

    __del__ = close
