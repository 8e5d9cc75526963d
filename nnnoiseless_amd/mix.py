"""The conference mixer (include/nnn_mix.h): the step a voice server puts behind the VAD gate.

ConferenceMixer mirrors the C object: per stream a room and a gain; every live member of a room receives the sum of the room's other
talkers, its own voice left out (mix-minus).  The rule is exact (one-frame gain ramps in float32, the terms and the room's total in
float64 in ascending stream index, one rounding to float32) and stated in the header.
"""
import numpy as np

from . import FRAME_SIZE, _ffi, library

MAX_GAIN = _ffi.MIX_MAX_GAIN
TILE = _ffi.MIX_TILE
REG_TALKERS = _ffi.MIX_REG_TALKERS


def _is_torch(a):
    return type(a).__module__.split(".")[0] == "torch"


class ConferenceMixer:
    """n_streams conference legs.  Audio is float32 [n_streams, n_frames, 480]; talk is uint8 / bool [n_frames, n_streams], exactly the open
    flags VadGate.apply returns (None: everybody talks); live is uint8 / bool [n_streams] (0 = the stream sits the call out: it is no
    member of its room for that call); heard is int32 [n_frames, n_streams], the number of other audible members each stream was sent."""

    def __init__(self, n_streams, device=0, lib=None):
        self._lib = lib or library()
        if not hasattr(self._lib.L, "nnn_mix_create"):
            raise RuntimeError("nnnoiseless_amd: this build of the library has no mixer (nnn_mix_*)")
        self.n_streams, self.device = int(n_streams), int(device)
        self._h = self._lib.L.nnn_mix_create(self.n_streams, self.device)
        if not self._h:
            raise RuntimeError("nnnoiseless_amd: " + self._lib.error())
        self._side = None   # a torch stream for calls made on torch's default stream (made on first use)

    def _idx(self, idx):
        if idx is None:
            return None, self.n_streams
        a, p = _ffi.stream_list(idx)
        self._keep = a
        return p, a.size

    @staticmethod
    def _values(v, n, dtype, name):
        v = np.asarray(v)
        if dtype is np.int32:
            v = v.astype(np.int64)
            if v.size and (v.min() < -2 ** 31 or v.max() >= 2 ** 31):
                raise ValueError(f"{name} out of int32 range")
        v = v.astype(dtype)
        v = np.full(n, v, dtype) if v.ndim == 0 else np.ascontiguousarray(v.reshape(-1))
        if v.size != n:
            raise ValueError(f"need {n} values of {name}, got {v.size}")
        return v

    def set_rooms(self, room, idx=None):
        """The rooms of the listed streams (idx None: of every stream): a scalar for all of them or one label per listed stream, each in
        -1 .. n_streams - 1 (-1: alone).  In force from the next call.  Does not touch the ramp state: mute a stream before moving it."""
        p, n = self._idx(idx)
        v = self._values(room, n, np.int32, "room")
        self._lib.check(self._lib.L.nnn_mix_set_rooms(self._h, p, n, _ffi.ptr(v)))

    def set_gains(self, gain, idx=None):
        """The gains of the listed streams, each in [0, MAX_GAIN]; a change reaches the audio through a one-frame ramp."""
        p, n = self._idx(idx)
        v = self._values(gain, n, np.float32, "gain")
        self._lib.check(self._lib.L.nnn_mix_set_gains(self._h, p, n, _ffi.ptr(v)))

    def rooms(self, idx=None):
        p, n = self._idx(idx)
        v = np.zeros(n, np.int32)
        self._lib.check(self._lib.L.nnn_mix_get_rooms(self._h, p, n, _ffi.ptr(v)))
        return v

    def gains(self, idx=None):
        p, n = self._idx(idx)
        v = np.zeros(n, np.float32)
        self._lib.check(self._lib.L.nnn_mix_get_gains(self._h, p, n, _ffi.ptr(v)))
        return v

    def reset(self, idx=None):
        """The listed streams (None: all) back to "silent so far": the next audible frame fades in.  Rooms and gains stay."""
        p, n = self._idx(idx)
        self._lib.check(self._lib.L.nnn_mix_reset(self._h, p, n))

    def _mask(self, a, shape, name):
        if a is None:
            return None
        m = np.ascontiguousarray(np.asarray(a) != 0, dtype=np.uint8)
        if m.shape != shape:
            raise ValueError(f"{name} must have shape {list(shape)}")
        return m

    def apply(self, audio, talk=None, live=None, out=None, want_heard=False):
        """One call over n_frames frames of every stream; never in place (an output needs every member's input).

        NumPy arrays: audio float32 [n_streams, n_frames, 480] on the host, synchronous; returns a new array (zeros where a masked stream
        owns the rows), or writes `out`.  torch tensors on the object's device: enqueued behind the kernels that made them on torch's
        current stream, and what torch enqueues there afterwards comes behind the call (on the default stream, whose handle the C ABI reads
        as "the object's own stream", through a side stream that waits for it and that it waits for); audio and out must be dense in
        their last axis, with any strides that are whole floats otherwise (e.g. a permuted view of the batch's [n_frames, n_streams, 480]),
        each its own.  Returns out, or (out, heard) with want_heard."""
        if _is_torch(audio):
            return self._apply_torch(audio, talk, live, out, want_heard)
        x = _ffi.as_f32(audio)
        if x.ndim != 3 or x.shape[0] != self.n_streams or x.shape[2] != FRAME_SIZE:
            raise ValueError(f"apply needs audio of shape [{self.n_streams}, n_frames, {FRAME_SIZE}], got {x.shape}")
        T = x.shape[1]
        out = np.zeros_like(x) if out is None else out
        if not (isinstance(out, np.ndarray) and out.shape == x.shape and out.dtype == np.float32 and out.flags.c_contiguous and out.flags.writeable):
            raise ValueError("apply: `out` must be a writable C-contiguous float32 array of the audio's shape")
        tk, lv = self._mask(talk, (T, self.n_streams), "talk"), self._mask(live, (self.n_streams,), "live")
        hd = np.zeros((T, self.n_streams), np.int32) if want_heard else None
        self._lib.check(self._lib.L.nnn_mix_apply_host(self._h, _ffi.ptr(x), _ffi.ptr(out), _ffi.ptr(tk), _ffi.ptr(lv), _ffi.ptr(hd), T))
        return (out, hd) if want_heard else out

    def _apply_torch(self, audio, talk, live, out, want_heard):
        import torch
        S = self.n_streams

        def strides(a, name):
            if a.dtype != torch.float32 or a.dim() != 3 or a.shape[0] != S or a.shape[2] != FRAME_SIZE or a.stride(2) != 1:
                raise ValueError(f"apply needs {name} as a float32 tensor [{S}, n_frames, {FRAME_SIZE}] that is dense in its last axis")
            if a.shape[1] > 1 and a.stride(1) < FRAME_SIZE:
                raise ValueError(f"apply: the frames of {name} overlap")
            return a.stride(0), max(a.stride(1), FRAME_SIZE)

        iss, ifs = strides(audio, "audio")
        T = audio.shape[1]
        out = torch.zeros_like(audio) if out is None else out
        if out.shape != audio.shape or out.device != audio.device:
            raise ValueError("apply: `out` must have the audio's shape and device")
        oss, ofs = strides(out, "out")

        def mask(a, shape, name):
            if a is None:
                return None
            m = (torch.as_tensor(a, device=audio.device) != 0).to(torch.uint8).contiguous()
            if tuple(m.shape) != shape:
                raise ValueError(f"{name} must have shape {list(shape)}")
            return m

        tk, lv = mask(talk, (T, S), "talk"), mask(live, (S,), "live")
        hd = torch.zeros((T, S), dtype=torch.int32, device=audio.device) if want_heard else None
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
        self.apply_device(audio.data_ptr(), out.data_ptr(), T, iss, ifs, oss, ofs, d_talk=None if tk is None else tk.data_ptr(),
                          d_live=None if lv is None else lv.data_ptr(), d_heard=None if hd is None else hd.data_ptr(), hip_stream=run.cuda_stream)
        if run is not cur:
            cur.wait_stream(run)
        for t in (audio, out, tk, lv, hd):             # (the caching allocator must not hand their memory on before the call has run)
            if t is not None:
                t.record_stream(run)
        return (out, hd) if want_heard else out

    def apply_device(self, d_in, d_out, n_frames, in_stream_stride, in_frame_stride, out_stream_stride, out_frame_stride, d_talk=None, d_live=None,
                     d_heard=None, hip_stream=0):
        """Raw device pointers (include/nnn_mix.h); asynchronous.  Strides in floats, a pair per side; d_out must not be d_in."""
        self._lib.check(self._lib.L.nnn_mix_apply_device(self._h, d_in, d_out, d_talk, d_live, d_heard, n_frames, in_stream_stride, in_frame_stride,
                                                         out_stream_stride, out_frame_stride, hip_stream))

    def apply_pcm_device(self, d_in, d_out, n_frames, in_layout, out_layout, d_talk=None, d_live=None, d_heard=None, hip_stream=0):
        """The packed boundary of BatchDenoiser.process_pcm_device, a layout per side: (format, channels, group_stride, frame_stride) with
        PCM_F32, PCM_F32_UNIT or PCM_I16 and the strides in elements."""
        import ctypes as C
        Li = _ffi.PcmLayout(in_layout[0], in_layout[1], 0, 0, in_layout[2], in_layout[3])
        Lo = _ffi.PcmLayout(out_layout[0], out_layout[1], 0, 0, out_layout[2], out_layout[3])
        self._lib.check(self._lib.L.nnn_mix_apply_pcm_device(self._h, d_in, d_out, d_talk, d_live, d_heard, n_frames, C.byref(Li), C.byref(Lo), hip_stream))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.L.nnn_mix_destroy(self._h)
            self._h = None

    __del__ = close
