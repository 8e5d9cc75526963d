"""The route of a host-buffer call (nnn_batch_host.hip plan_host_call, read through nnn_batch_debug_host_plan): zero-copy through mapped
memory, staged in one piece, or staged in chunks over two copy streams -- and the chunk length.  Plans only: no frame runs here.

The expected values are worked out by hand from the rule (include/nnn_batch.h, nnn_batch_process_host):
  * a call whose bounding span, VAD rows and 16 bytes fit one MiB is zero-copy, unless NNN_HOST_CHUNK is set (then it is always staged);
  * NNN_HOST_CHUNK = n > 0 is the chunk length, 0 asks for one piece; unset the chunk is n_frames / 16, at least 1 -- at least 4 up to
    8192 streams --, at most 16, doubled (up to 16) while a chunk of every stream is under one MiB, and one piece if it still is;
  * chunks need a call longer than one chunk, gap-free frames and no held stream; everything else runs in one piece."""
import ctypes as C

import pytest

ZERO_COPY, ONE_PIECE, CHUNKED = 0, 1, 2
F32, I16 = 0, 1


def host_plan(lib, bd, n_frames, fmt=F32, channels=1, frame_stride=None, discard_first=False, has_vad=True):
    from nnnoiseless_amd import _ffi
    fs = 480 * channels if frame_stride is None else frame_stride
    lay = _ffi.PcmLayout(fmt, channels, int(discard_first), 0, n_frames * fs, fs)
    out = (C.c_int64 * 8)()
    lib.check(lib.L.nnn_batch_debug_host_plan(bd._h, n_frames, C.byref(lay), int(has_vad), out))
    return dict(zip(("route", "chunk", "n_chunks", "span", "vbytes", "vofs", "drop", "vad_masked"), out))


def batch(lib, monkeypatch, streams, env=None):
    import nnnoiseless_amd as nn
    if env is None:
        monkeypatch.delenv("NNN_HOST_CHUNK", raising=False)
    else:
        monkeypatch.setenv("NNN_HOST_CHUNK", env)
    return nn.BatchDenoiser(streams, lib=lib)


# streams, frames, NNN_HOST_CHUNK, layout, (route, chunk, chunks)
CASES = [
    (1, 1, None, {}, (ZERO_COPY, 1, 1)),
    (1, 544, None, {}, (ZERO_COPY, 544, 1)),          # 1924 * 544 + 16 = 1 046 672 <= 2^20
    (1, 545, None, {}, (ONE_PIECE, 545, 1)),          # 1 048 596 > 2^20; 16 frames of one stream stay under the megabyte floor
    (4, 7, None, {}, (ZERO_COPY, 7, 1)),
    (4, 7, "3", {}, (CHUNKED, 3, 3)),
    (4, 7, "0", {}, (ONE_PIECE, 7, 1)),
    (64, 48, None, {}, (CHUNKED, 16, 3)),             # 3 -> 4 -> 8 -> 16; 16 * 1920 * 64 >= 2^20
    (32, 48, None, {}, (ONE_PIECE, 48, 1)),           # 16 * 1920 * 32 = 983 040 < 2^20
    (64, 48, None, {"fmt": I16}, (ONE_PIECE, 48, 1)),   # 16 * 960 * 64: the same product
    (64, 16, None, {}, (ONE_PIECE, 16, 1)),           # a call must be longer than its chunk
    (64, 17, None, {}, (CHUNKED, 16, 2)),
    (64, 48, "5", {}, (CHUNKED, 5, 10)),
    (64, 48, None, {"frame_stride": 2 * 480}, (ONE_PIECE, 48, 1)),
]


@pytest.mark.parametrize("streams,frames,env,layout,want", CASES)
def test_route_and_chunk_length(hostsim_lib, monkeypatch, streams, frames, env, layout, want):
    bd = batch(hostsim_lib, monkeypatch, streams, env)
    p = host_plan(hostsim_lib, bd, frames, **layout)
    assert (p["route"], p["chunk"], p["n_chunks"]) == want, p
    elem, fs = (2 if layout.get("fmt") == I16 else 4), layout.get("frame_stride", 480)
    span = ((streams - 1) * frames * fs + (frames - 1) * fs + 480) * elem          # the last frame of the last stream ends the span
    assert (p["span"], p["vbytes"], p["vofs"]) == (span, 4 * frames * streams, (span + 15) // 16 * 16), p
    assert (p["drop"], p["vad_masked"]) == (0, 0), p
    q = host_plan(hostsim_lib, bd, frames, has_vad=False, **layout)
    assert (q["span"], q["vbytes"], q["vad_masked"]) == (span, 0, 0), q


def test_a_held_stream_means_one_piece(hostsim_lib, monkeypatch):
    """The chunks' downloads write whole rows of every stream into the caller's buffers; a held stream's bytes are not the call's to write."""
    bd = batch(hostsim_lib, monkeypatch, 64)
    assert host_plan(hostsim_lib, bd, 48)["route"] == CHUNKED
    bd.hold_streams([5])
    p = host_plan(hostsim_lib, bd, 48)
    assert (p["route"], p["chunk"], p["n_chunks"], p["vad_masked"]) == (ONE_PIECE, 48, 1, 1), p
    assert host_plan(hostsim_lib, bd, 48, has_vad=False)["vad_masked"] == 0
    bd.resume_streams([5])
    assert host_plan(hostsim_lib, bd, 48)["route"] == CHUNKED


def test_first_frame_is_dropped_on_a_fresh_batch_only(hostsim_lib, monkeypatch):
    import numpy as np
    from nnnoiseless_amd import _ffi
    bd = batch(hostsim_lib, monkeypatch, 4, "3")
    stereo = dict(fmt=I16, channels=2, discard_first=True)
    p = host_plan(hostsim_lib, bd, 7, **stereo)
    assert (p["route"], p["chunk"], p["n_chunks"], p["drop"]) == (CHUNKED, 3, 3, 1), p
    assert (p["span"], p["vbytes"]) == (2 * 7 * 480 * 2 * 2, 4 * 7 * 4), p
    assert host_plan(hostsim_lib, bd, 7, fmt=I16, channels=2)["drop"] == 0
    bd.process_pcm(np.zeros((2, 480, 2), np.int16), _ffi.PCM_I16, 2)
    p = host_plan(hostsim_lib, bd, 7, **stereo)
    assert (p["route"], p["chunk"], p["n_chunks"], p["drop"]) == (CHUNKED, 3, 3, 0), p
