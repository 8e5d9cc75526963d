"""The file packer (include/nnn_pack.h) on the GPU library: the cases of test_hostsim_pack.py at 70 streams (one
full 64-stream tile and a ragged 6) over about 150 files of 0 to 40 frames, and one run at 4096 streams.  Bit for bit: the yardstick of a
file is the same library's lone run (tests/pack_cases.py)."""
import os

import numpy as np
import pytest

import pack_cases as pc
from conftest import GOLDEN

S = 70
N_FILES = 150


def _files(channels, n_files=N_FILES, seed=0):
    """Files of 0 to 40 whole frames (a few of each edge: 0, 1, 2) from synthetic.make_streams, rounded to integers so that every
    sample format carries them exactly, a few samples of partial frame behind each."""
    from nnnoiseless_amd.synthetic import make_streams
    rng = np.random.default_rng(100 + seed)
    frames = [int(f) for f in rng.integers(0, 41, n_files)]
    frames[:6] = [40, 0, 1, 2, 24, 5]
    x = np.round(make_streams(1000 * seed, n_files * channels, 41)).astype(np.float32).reshape(n_files, channels, 41 * pc.FRAME)
    return [np.ascontiguousarray(x[i, :, :F * pc.FRAME + (7 + 3 * i) % pc.FRAME].T) for i, F in enumerate(frames)]


class _LoneReset:
    """Lone runs on ONE batch of `channels` streams, reset between files (nnn_batch_reset: back to the freshly-created state, frame
    count included) instead of 150 batches made and destroyed; computed once per file and shared by the tests."""

    def __init__(self, lib, files, channels):
        import nnnoiseless_amd as nn
        self.bd, self.files, self.channels, self.memo = nn.BatchDenoiser(channels, lib=lib), files, channels, {}

    def __call__(self, i):
        from nnnoiseless_amd import pcm
        if i not in self.memo:
            x = self.files[i]
            F = x.shape[0] // pc.FRAME
            if F == 0:
                self.memo[i] = (np.zeros((0, self.channels), np.float32), np.zeros((0, self.channels), np.float32))
            else:
                self.bd.reset()
                o, v = self.bd.process_pcm(x[None, :F * pc.FRAME], pcm.PCM_F32, self.channels, discard_first=True)
                self.memo[i] = (o[0].copy(), v.copy())
        return self.memo[i]


@pytest.fixture(scope="module")
def corpus(gpu_lib):
    sets = {}
    for channels in (1, 2):
        files = _files(channels, seed=channels)
        sets[channels] = (files, _LoneReset(gpu_lib, files, channels))
    yield sets
    for _, lone in sets.values():
        lone.bd.close()


@pytest.mark.gpu
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("step", [24, 5])
def test_every_file_is_its_lone_run_gpu(gpu_lib, corpus, channels, step):
    """150 files at odd offsets with gaps, canaries around every output range; f32 in and out."""
    files, lone = corpus[channels]
    outs, vads, s, _ = pc.run_packed(gpu_lib, files, channels, S, step)
    pc.assert_files_equal(outs, vads, files, channels, lone, (channels, step))
    assert s["useful"] == channels * sum(x.shape[0] // pc.FRAME for x in files)
    assert s["useful"] + s["padded"] + s["held_frames"] == s["launched"] and s["max_pad"] <= step - 1


@pytest.mark.gpu
def test_a_lone_batch_agrees_with_the_reset_one_gpu(gpu_lib, corpus):
    """The shared yardstick resets one batch between files; three files on batches of their own give the same bits."""
    for channels in (1, 2):
        files, lone = corpus[channels]
        for i in (0, 4, 7):
            o, v = pc.lone(gpu_lib, files[i], channels)
            assert np.array_equal(pc.bits(o), pc.bits(lone(i)[0])) and np.array_equal(pc.bits(v), pc.bits(lone(i)[1]))


@pytest.mark.gpu
@pytest.mark.parametrize("fmt, out_i16", [("PCM_I16", True), ("PACK_I24", False), ("PACK_I32", True), ("PACK_F32_WAV", False)])
def test_formats_at_odd_offsets_gpu(gpu_lib, corpus, fmt, out_i16):
    """int16 spans on odd elements, 24-bit spans on any byte, reversed order, steps of 5.  The files are integers in the int16 range, so
    the 16-, 24- and 32-bit inputs convert to the very samples of the f32 files and the shared lone runs serve; the WAV-float input is
    compared with lone runs of its own converted samples (a third of the files: a lone run each)."""
    from nnnoiseless_amd import pcm
    files, lone = corpus[1]
    if fmt == "PACK_F32_WAV":
        files = files[:50]
    outs, vads, _, want_in = pc.run_packed(gpu_lib, files, 1, S, 5, in_fmt=getattr(pcm, fmt), out_i16=out_i16, order=range(len(files))[::-1])
    if fmt == "PACK_F32_WAV":
        own = _LoneReset(gpu_lib, want_in, 1)
        pc.assert_files_equal(outs, vads, want_in, 1, own, fmt)
        own.bd.close()
        return
    for i in range(len(files)):
        assert np.array_equal(want_in[i], files[i])
    want = (lambda i: (pc.to_i16(lone(i)[0]), lone(i)[1])) if out_i16 else lone
    pc.assert_files_equal(outs, vads, files, 1, want, fmt)


@pytest.mark.gpu
def test_golden_file_among_neighbours_gpu(gpu_lib, corpus):
    """tests/golden/testing.raw packed as one file among synthetic neighbours, int16 in and out: bit for bit denoise_raw_i16's, and
    reference_output.raw under the metric and bar of test_gpu_parity.py::test_cli_raw_i16_golden."""
    from nnnoiseless_amd import pcm
    raw = np.fromfile(os.path.join(GOLDEN, "testing.raw"), dtype="<i2")
    ref = np.fromfile(os.path.join(GOLDEN, "reference_output.raw"), dtype="<i2")
    files = list(corpus[1][0][:40])
    files.insert(17, raw.astype(np.float32)[:, None])
    outs, _, _, _ = pc.run_packed(gpu_lib, files, 1, S, 24, in_fmt=pcm.PCM_I16, out_i16=True)
    out = outs[17][:, 0]
    assert np.array_equal(out, pcm.denoise_raw_i16(raw, 1, lib=gpu_lib)[:, 0])
    assert out.shape == ref.shape
    d = np.abs(out.astype(np.int32) - ref.astype(np.int32))
    assert d.max() <= 1 and (d != 0).mean() < 1e-3, (d.max(), (d != 0).mean())


@pytest.mark.gpu
def test_4096_streams_three_steps_gpu(gpu_lib):
    """4096 streams, steps of 2 frames, 4300 files of 1 to 6 frames: a multi-block grid, slots refilled, and an idle tail held tile by
    tile once the list runs out.  The yardstick here is one equal-length call of a batch with a stream per file -- a stream's first F
    frames do not depend on what follows them --, and three files are checked against lone batches of their own as well."""
    import nnnoiseless_amd as nn
    from nnnoiseless_amd.synthetic import make_streams_fast
    n_files, T = 4300, 6
    rng = np.random.default_rng(5)
    frames = rng.integers(1, T + 1, n_files)
    frames[:3] = [6, 1, 5]
    x = np.round(make_streams_fast(n_files, T, seed=3)).astype(np.float32).reshape(n_files, T * pc.FRAME)
    files = [x[i, :frames[i] * pc.FRAME + i % 11, None] if frames[i] < T else x[i, :, None] for i in range(n_files)]
    bd = nn.BatchDenoiser(n_files, lib=gpu_lib)
    o, v = bd.process(x.reshape(n_files, T, pc.FRAME))
    bd.close()
    want = lambda i: (o[i, 1:frames[i]].reshape(-1, 1), v[:frames[i], i:i + 1])
    outs, vads, s, _ = pc.run_packed(gpu_lib, files, 1, 4096, 2)
    assert s["steps"] >= 3 and s["held_steps"] > 64
    pc.assert_files_equal(outs, vads, files, 1, want)
    for i in range(3):
        lo, lv = pc.lone(gpu_lib, files[i], 1)
        assert np.array_equal(pc.bits(outs[i]), pc.bits(lo)) and np.array_equal(pc.bits(vads[i]), pc.bits(lv))
