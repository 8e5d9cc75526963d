"""The talker picker (include/nnn_pick.h): the step a conference bridge puts between the VAD gate and the mixer.

TalkerPicker mirrors the C object: per stream a room and a pin, per object the policy (k, decay, stick); of every room's open gates the k
loudest talk, an incumbent keeps its place until a challenger is `stick` times louder, and the room's dominant speaker is reported.  The
rule is exact (frame energies in float64 in the scorer's summation order, one multiplication and one comparison for the level, a ranking
on bit patterns) and stated in the header.
"""
import ctypes as C

import numpy as np

from . import FRAME_SIZE, _ffi, library

MAX_K = _ffi.PICK_MAX_K
MAX_STICK = _ffi.PICK_MAX_STICK


def _is_torch(a):
    return type(a).__module__.split(".")[0] == "torch"


class TalkerPicker:
    """n_streams conference legs.  Audio is float32 [n_streams, n_frames, 480]; open is uint8 / bool [n_frames, n_streams], exactly the
    open flags VadGate.apply returns (None: every gate is open); live is uint8 / bool [n_streams] (0 = the stream sits the call out: it is
    no member of its room for that call).  talk is uint8 [n_frames, n_streams], exactly what ConferenceMixer.apply takes as talk; dominant
    is int32 [n_frames, n_streams], the room's first-ranked candidate or -1; level is float64 [n_frames, n_streams]."""

    def __init__(self, n_streams, device=0, lib=None):
        self._lib = lib or library()
        if not hasattr(self._lib.L, "nnn_pick_create"):
            raise RuntimeError("nnnoiseless_amd: this build of the library has no talker picker (nnn_pick_*)")
        self.n_streams, self.device = int(n_streams), int(device)
        self._h = self._lib.L.nnn_pick_create(self.n_streams, self.device)
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
        v = np.asarray(v).astype(np.int64)
        lo, hi = (0, 256) if dtype is np.uint8 else (-2 ** 31, 2 ** 31)
        if v.size and (v.min() < lo or v.max() >= hi):
            raise ValueError(f"{name} out of range")
        v = v.astype(dtype)
        v = np.full(n, v, dtype) if v.ndim == 0 else np.ascontiguousarray(v.reshape(-1))
        if v.size != n:
            raise ValueError(f"need {n} values of {name}, got {v.size}")
        return v

    def set_rooms(self, room, idx=None):
        """The rooms of the listed streams (idx None: of every stream): a scalar for all of them or one label per listed stream, each in
        -1 .. n_streams - 1 (-1: alone) -- the labels the mixer has.  In force from the next call."""
        p, n = self._idx(idx)
        v = self._values(room, n, np.int32, "room")
        self._lib.check(self._lib.L.nnn_pick_set_rooms(self._h, p, n, _ffi.ptr(v)))

    def set_pinned(self, pinned, idx=None):
        """The pins of the listed streams, each 0 or 1: a pinned stream with an open gate ranks ahead of every unpinned one."""
        p, n = self._idx(idx)
        v = self._values(pinned, n, np.uint8, "pinned")
        self._lib.check(self._lib.L.nnn_pick_set_pinned(self._h, p, n, _ffi.ptr(v)))

    def set_policy(self, k=3, decay=0.875, stick=4.0):
        """k in 1 .. MAX_K talkers per room; decay in [0, 1]: what a frame leaves of a level; stick in [1, MAX_STICK]: by how much a
        challenger's level must exceed an incumbent's."""
        self._lib.check(self._lib.L.nnn_pick_set_policy(self._h, int(k), float(decay), float(stick)))

    def rooms(self, idx=None):
        p, n = self._idx(idx)
        v = np.zeros(n, np.int32)
        self._lib.check(self._lib.L.nnn_pick_get_rooms(self._h, p, n, _ffi.ptr(v)))
        return v

    def pinned(self, idx=None):
        p, n = self._idx(idx)
        v = np.zeros(n, np.uint8)
        self._lib.check(self._lib.L.nnn_pick_get_pinned(self._h, p, n, _ffi.ptr(v)))
        return v

    def policy(self):
        """(k, decay, stick) as the object holds them (decay and stick as the float32 values they were rounded to)."""
        k, d, s = C.c_int(), C.c_float(), C.c_float()
        self._lib.check(self._lib.L.nnn_pick_get_policy(self._h, C.byref(k), C.byref(d), C.byref(s)))
        return k.value, d.value, s.value

    def reset(self, idx=None):
        """The listed streams (None: all) back to "silent and not selected so far".  Rooms, pins and policy stay."""
        p, n = self._idx(idx)
        self._lib.check(self._lib.L.nnn_pick_reset(self._h, p, n))

    def _mask(self, a, shape, name):
        if a is None:
            return None
        m = np.ascontiguousarray(np.asarray(a) != 0, dtype=np.uint8)
        if m.shape != shape:
            raise ValueError(f"{name} must have shape {list(shape)}")
        return m

    @staticmethod
    def _result(talk, dom, lvl, want_dominant, want_level):
        if not (want_dominant or want_level):
            return talk
        return (talk,) + ((dom,) if want_dominant else ()) + ((lvl,) if want_level else ())

    def select(self, audio, open=None, live=None, want_dominant=False, want_level=False):   # noqa: A002 -- the gate's name for these rows
        """One call over n_frames frames of every stream; the audio is only read.

        NumPy arrays: audio float32 [n_streams, n_frames, 480] on the host, synchronous.  torch tensors on the object's device: enqueued
        behind the kernels that made them on torch's current stream, and what torch enqueues there afterwards comes behind the call (on the
        default stream, whose handle the C ABI reads as "the object's own stream", through a side stream that waits for it and that it
        waits for); the audio must be dense in its last axis, with any strides that are whole floats otherwise (e.g. a permuted view of the
        batch's [n_frames, n_streams, 480]).  Returns talk, or (talk, dominant), (talk, level), (talk, dominant, level) as asked; what a
        stream marked 0 in live owns in them is zeros."""
        if _is_torch(audio):
            return self._select_torch(audio, open, live, want_dominant, want_level)
        x = _ffi.as_f32(audio)
        if x.ndim != 3 or x.shape[0] != self.n_streams or x.shape[2] != FRAME_SIZE:
            raise ValueError(f"select needs audio of shape [{self.n_streams}, n_frames, {FRAME_SIZE}], got {x.shape}")
        T = x.shape[1]
        op, lv = self._mask(open, (T, self.n_streams), "open"), self._mask(live, (self.n_streams,), "live")
        talk = np.zeros((T, self.n_streams), np.uint8)
        dom = np.zeros((T, self.n_streams), np.int32) if want_dominant else None
        lvl = np.zeros((T, self.n_streams), np.float64) if want_level else None
        self._lib.check(self._lib.L.nnn_pick_select_host(self._h, _ffi.ptr(x), _ffi.ptr(op), _ffi.ptr(lv), _ffi.ptr(talk), _ffi.ptr(dom), _ffi.ptr(lvl), T))
        return self._result(talk, dom, lvl, want_dominant, want_level)

    def _select_torch(self, audio, open_, live, want_dominant, want_level):
        import torch
        S = self.n_streams
        if audio.dtype != torch.float32 or audio.dim() != 3 or audio.shape[0] != S or audio.shape[2] != FRAME_SIZE or audio.stride(2) != 1:
            raise ValueError(f"select needs audio as a float32 tensor [{S}, n_frames, {FRAME_SIZE}] that is dense in its last axis")
        T = audio.shape[1]
        if T > 1 and audio.stride(1) < FRAME_SIZE:
            raise ValueError("select: the frames of audio overlap")
        ss, fs = audio.stride(0), max(audio.stride(1), FRAME_SIZE)

        def mask(a, shape, name):
            if a is None:
                return None
            m = (torch.as_tensor(a, device=audio.device) != 0).to(torch.uint8).contiguous()
            if tuple(m.shape) != shape:
                raise ValueError(f"{name} must have shape {list(shape)}")
            return m

        op, lv = mask(open_, (T, S), "open"), mask(live, (S,), "live")
        talk = torch.zeros((T, S), dtype=torch.uint8, device=audio.device)
        dom = torch.zeros((T, S), dtype=torch.int32, device=audio.device) if want_dominant else None
        lvl = torch.zeros((T, S), dtype=torch.float64, device=audio.device) if want_level else None
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
        self.select_device(audio.data_ptr(), talk.data_ptr(), T, ss, fs, d_open=None if op is None else op.data_ptr(),
                           d_live=None if lv is None else lv.data_ptr(), d_dominant=None if dom is None else dom.data_ptr(),
                           d_level=None if lvl is None else lvl.data_ptr(), hip_stream=run.cuda_stream)
        if run is not cur:
            cur.wait_stream(run)
        for t in (audio, op, lv, talk, dom, lvl):      # (the caching allocator must not hand their memory on before the call has run)
            if t is not None:
                t.record_stream(run)
        return self._result(talk, dom, lvl, want_dominant, want_level)

    def select_device(self, d_in, d_talk, n_frames, stream_stride, frame_stride, d_open=None, d_live=None, d_dominant=None, d_level=None, hip_stream=0):
        """Raw device pointers (include/nnn_pick.h); asynchronous.  Strides in floats; d_talk may be d_open itself."""
        self._lib.check(self._lib.L.nnn_pick_select_device(self._h, d_in, d_open, d_live, d_talk, d_dominant, d_level, n_frames, stream_stride,
                                                           frame_stride, hip_stream))

    def select_pcm_device(self, d_in, d_talk, n_frames, layout, d_open=None, d_live=None, d_dominant=None, d_level=None, hip_stream=0):
        """The packed boundary of BatchDenoiser.process_pcm_device: layout = (format, channels, group_stride, frame_stride) with PCM_F32,
        PCM_F32_UNIT or PCM_I16 and the strides in elements."""
        L = _ffi.PcmLayout(layout[0], layout[1], 0, 0, layout[2], layout[3])
        self._lib.check(self._lib.L.nnn_pick_select_pcm_device(self._h, d_in, d_open, d_live, d_talk, d_dominant, d_level, n_frames, C.byref(L), hip_stream))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.L.nnn_pick_destroy(self._h)
            self._h = None

    __del__ = close
