"""k_synth's software-pipelined frame loop (nnn_synth.hip): inside frame f of a group the wave requests frame f + 1's spectra, band
quantities, silence flag and VAD.  The smallest shapes at which that can go wrong, on the MI355X and under the test-only SIMT
interpreter: 70 streams (a full tile and a ragged one whose last block of four has two padding streams) x 27 frames through the three
launches (back end 0), as one call (groups of 24 + 3), as calls of 1, 2 and 24 frames (a group of one: no request at all; a group of
two: one request, none in the last frame) and as 27 calls of one frame, the loop that never pipelines.  Audio, VAD and the per-frame
record agree bit for bit -- as f32 and as packed int16 with two interleaved channels (k_synth<true> and k_synth<false>)."""
import numpy as np
import pytest

S, T = 70, 27
CALLS = {"one": (27,), "mixed": (1, 2, 24), "ticks": (1,) * 27}
GAP = 9          # all-zero input in frames 5-9 only: `live` flips while the next frame's inputs are in flight
MUTE = 23        # silent throughout: exact zeros out
HELD = 66        # held (nnn_batch_hold_streams) during frames 1-2: the middle call of "mixed"; in the ragged tile's last block
TWIN = 12        # HELD's input without frames 1-2, never held: what HELD must give around its pause
HOLD = (1, 3)    # frames [1, 3)
SENT = 12345.0   # what the caller's buffers hold where a held stream writes nothing


def _input():
    from nnnoiseless_amd.synthetic import make_streams
    x = make_streams(41, S, T).copy()
    x[GAP] *= 1e-3                               # (quiet enough that the high-pass filter's tail is below the silence threshold a frame into the gap)
    x[GAP, 5:10] = 0.0
    x[MUTE] = 0.0
    x[HELD] = make_streams(42, 1, T)[0]          # (whatever the synthetic mix put there: a stream with audio)
    x[TWIN, :T - 2] = np.delete(x[HELD], (1, 2), axis=0)
    return x


class _Log:
    """[T][S][24] words where the library's kernels can write them: device memory on the GPU, host memory under the interpreter."""
    def __init__(self, gpu):
        if gpu:
            import torch
            self.t = torch.zeros((T, S, 24), dtype=torch.int32, device=torch.device("cuda", 0))
            self.ptr = self.t.data_ptr()
        else:
            self.a = np.zeros((T, S, 24), np.uint32)
            self.ptr = self.a.ctypes.data

    def get(self):
        return self.t.cpu().numpy().view(np.uint32) if hasattr(self, "t") else self.a


def _run(nn, lib, gpu, x, calls, hold, pcm):
    """-> audio [S, T, 480] (f32, or i16 for pcm), vad [T, S], record [T, S, 24]; HELD held for the calls inside frames HOLD if `hold`."""
    from nnnoiseless_amd import _ffi
    bd = nn.BatchDenoiser(S, lib=lib)
    bd.set_back_end(0)
    log = _Log(gpu)
    bd.set_frame_log(log.ptr, T)
    if pcm:
        xin = np.clip(np.rint(x.reshape(S // 2, 2, T * 480).transpose(0, 2, 1)), -32768, 32767).astype(np.int16)
    outs, vads, t = [], [], 0
    for n in calls:
        if hold and t == HOLD[0]:
            bd.hold_streams([HELD])
        if hold and t == HOLD[1]:
            bd.resume_streams([HELD])
        v = np.full((n, S), SENT, np.float32)
        if pcm:
            o = np.full((S // 2, n * 480, 2), int(SENT), np.int16)
            bd.process_pcm(xin[:, t * 480:(t + n) * 480], _ffi.PCM_I16, channels=2, out=o, vad=v)
            o = o.transpose(0, 2, 1).reshape(S, n, 480)
        else:
            o = np.full((S, n, 480), SENT, np.float32)
            bd.process(x[:, t:t + n], out=o, vad=v)
        outs.append(o)
        vads.append(v)
        t += n
    assert not bd.fault()
    return np.concatenate(outs, 1), np.concatenate(vads, 0), log.get().copy()


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b, streams=slice(None)):
    return (np.array_equal(_bits(a[0][streams]), _bits(b[0][streams])) and np.array_equal(_bits(a[1][:, streams]), _bits(b[1][:, streams]))
            and np.array_equal(a[2][:, streams], b[2][:, streams]))


def _check(nn, lib, gpu, pcm):
    x = _input()
    one = _run(nn, lib, gpu, x, CALLS["one"], False, pcm)        # (a call cannot hold a stream for two of its frames: HELD runs through)
    mixed = _run(nn, lib, gpu, x, CALLS["mixed"], True, pcm)
    ticks = _run(nn, lib, gpu, x, CALLS["ticks"], True, pcm)
    others = np.arange(S) != HELD
    assert _same(mixed, ticks)                                    # every stream, the held one with its pause
    assert _same(one, ticks, others)
    out, vad, log = mixed
    sent = np.int16(SENT) if pcm else np.float32(SENT)
    # the held stream: nothing written during its pause, and around it what the same audio gives without the pause -- in every run
    p0, p1 = HOLD
    assert (out[HELD, p0:p1] == sent).all() and (vad[p0:p1, HELD] == np.float32(SENT)).all() and not log[p0:p1, HELD].any()
    keep = np.r_[0:p0, p1:T]
    for run in (one, mixed, ticks):
        assert np.array_equal(_bits(out[HELD, keep]), _bits(run[0][TWIN, :T - 2]))
        assert np.array_equal(_bits(vad[keep, HELD]), _bits(run[1][:T - 2, TWIN]))
        assert np.array_equal(log[keep, HELD], run[2][:T - 2, TWIN])
    # silence in, exact zeros out; the gap is seen as silence (bit 22 of the branch mask) inside frames 5-9 and nowhere else
    assert not out[MUTE].any() and not vad[:, MUTE].any()
    gate = (log[:, GAP, 1] >> 22) & 1
    assert gate[6:10].all() and not gate[:5].any() and not gate[10:].any()
    assert out[GAP, 12:].any() and np.abs(out.astype(np.float64)).max() > 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("pcm", [False, True], ids=["f32", "i16x2"])
def test_pipelined_synthesis_on_the_gpu(gpu_lib, pcm):
    import nnnoiseless_amd as nn
    _check(nn, gpu_lib, True, pcm)


@pytest.mark.parametrize("pcm", [False, True], ids=["f32", "i16x2"])
def test_pipelined_synthesis_under_the_interpreter(hostsim_lib, pcm):
    import nnnoiseless_amd as nn
    _check(nn, hostsim_lib, False, pcm)
