"""The file packer (include/nnn_pack.h) under the test-only SIMT interpreter: files of unequal length through one
batch, every file bit for bit what it gets alone (tests/pack_cases.py), whatever the slots, the step, the order, the formats and the
offsets.  3 mono slots, steps of 2 frames, about 15 file-frames."""
import os
import re
import subprocess
import sys
import wave

import numpy as np
import pytest

import pack_cases as pc
from conftest import ROOT

FRAMES = [3, 0, 1, 2, 5, 2]
S, STEP = 3, 2


@pytest.fixture(scope="module")
def mono(hostsim_lib):
    files = pc.make_files(FRAMES, 1, seed=1, loud=(4,))
    return files, pc.Lone(hostsim_lib, files, 1)


def test_abi_symbols():
    """The functions nnn_pack.h declares are _ffi.PACK_SYMBOLS, and the built library exports each (as test_abi.py reads them)."""
    from nnnoiseless_amd import _ffi
    from nnnoiseless_amd.build import build_library
    src = open(os.path.join(ROOT, "include", "nnn_pack.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b((?:nnn|rnnoise)_[a-z0-9_]+)\s*\(", src))
    assert declared == set(_ffi.PACK_SYMBOLS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", build_library()]).decode()
    for sym in declared:
        assert re.search(rf"\bT {sym}\b", out), sym
    batch = open(os.path.join(ROOT, "include", "nnn_batch.h")).read()
    values = {int(v) for v in re.findall(r"NNN_PCM_\w+ = (\d+)", batch)}
    assert values == {_ffi.PCM_F32, _ffi.PCM_I16, _ffi.PCM_F32_UNIT} and not values & {_ffi.PACK_I24, _ffi.PACK_I32, _ffi.PACK_F32_WAV}
    for name, v in (("NNN_PACK_I24", _ffi.PACK_I24), ("NNN_PACK_I32", _ffi.PACK_I32), ("NNN_PACK_F32_WAV", _ffi.PACK_F32_WAV)):
        assert re.search(rf"\b{name} = {v}\b", src)


def test_composition_bit_for_bit(hostsim_lib, mono):
    """Files of [3, 0, 1, 2, 5, 2] whole frames, a partial frame behind each, at odd offsets with gaps: audio, VAD and counts of every
    file are its lone run's; the canaries around the output ranges survive (run_packed checks them)."""
    files, lone = mono
    outs, vads, s, _ = pc.run_packed(hostsim_lib, files, 1, S, STEP)
    pc.assert_files_equal(outs, vads, files, 1, lone)
    assert s["useful"] == sum(FRAMES) and s["files"] == 5
    assert s["useful"] + s["padded"] + s["held_frames"] == s["launched"]


@pytest.mark.parametrize("order, n_streams, step", [("reversed", 3, 2), ("given", 3, 1), ("given", 2, 2), ("reversed", 2, 3), ("given", 8, 2)])
def test_any_order_any_geometry(hostsim_lib, mono, order, n_streams, step):
    """Reversed, step_frames = 1, 2 slots, a step that is no divisor of anything, more slots than files: the same per-file bits.  With
    8 slots for 5 files the idle slots are held during the run and released after it (run_packed asserts num_held() == 0)."""
    files, lone = mono
    perm = list(range(len(files)))[::-1] if order == "reversed" else None
    outs, vads, s, _ = pc.run_packed(hostsim_lib, files, 1, n_streams, step, order=perm)
    pc.assert_files_equal(outs, vads, files, 1, lone, (order, n_streams, step))
    if n_streams == 8:
        assert s["held_steps"] >= 3 * s["steps"]   # three slots never get a file


def test_file_ending_on_a_step_boundary(hostsim_lib):
    """Files of exactly 2 and 4 frames with steps of 2: the slot is refilled at the boundary, nothing is padded for them."""
    files = pc.make_files([2, 4, 1, 2], 1, seed=2)
    lone = pc.Lone(hostsim_lib, files, 1)
    outs, vads, s, _ = pc.run_packed(hostsim_lib, files, 1, 2, 2)
    pc.assert_files_equal(outs, vads, files, 1, lone)
    assert s["max_pad"] == 1 and s["padded"] == 1   # (only the one-frame file pads)


def test_stereo_equals_denoise_raw_i16(hostsim_lib):
    """4 streams, channels = 2, three files, int16 in and out: each is denoise_raw_i16(file, 2)."""
    from nnnoiseless_amd import pcm
    files = pc.make_files([2, 3, 1], 2, seed=3)
    outs, vads, _, _ = pc.run_packed(hostsim_lib, files, 2, 4, STEP, in_fmt=pcm.PCM_I16, out_i16=True)
    for i, x in enumerate(files):
        want = pcm.denoise_raw_i16(x.astype(np.int16), 2, lib=hostsim_lib)
        assert outs[i].dtype == np.int16 and outs[i].shape == want.shape and np.array_equal(outs[i], want), i
        assert np.array_equal(pc.bits(vads[i]), pc.bits(pc.lone(hostsim_lib, x, 2)[1])), i


@pytest.mark.parametrize("fmt", ["PACK_I24", "PACK_I32", "PACK_F32_WAV", "PCM_I16"])
def test_input_formats(hostsim_lib, fmt):
    """24-bit, 32-bit and WAV-float inputs equal the f32 run of the numpy-converted samples (>> 8, >> 16, * float32(32767))."""
    from nnnoiseless_amd import pcm
    files = pc.make_files([2, 1, 3], 1, seed=4)
    outs, vads, _, want_in = pc.run_packed(hostsim_lib, files, 1, 2, STEP, in_fmt=getattr(pcm, fmt))
    for i in range(len(files)):   # (the bits >> drops are random in the arena and must vanish; the WAV floats round once and differ)
        assert np.array_equal(want_in[i], files[i]) == (fmt != "PACK_F32_WAV")
    pc.assert_files_equal(outs, vads, want_in, 1, lambda i: pc.lone(hostsim_lib, want_in[i], 1), fmt)


def test_int16_out_is_the_f32_out_rounded(hostsim_lib, mono):
    """int16 out = the f32 out through the CLI writers' clamp and round-half-away; the loud file reaches the clamp."""
    files, lone = mono
    outs, vads, _, _ = pc.run_packed(hostsim_lib, files, 1, S, STEP, out_i16=True)
    assert np.abs(lone(4)[0]).max() > 32768.0, "the loud file must reach the clamp"
    pc.assert_files_equal(outs, vads, files, 1, lambda i: (pc.to_i16(lone(i)[0]), lone(i)[1]))


def test_reuse_and_fresh_batch(hostsim_lib, mono):
    """A second run on the same packer gives the first one's bits, and the batch is left fresh: nothing held, and a file processed on it
    directly behaves as on a new batch (but for discard_first, which sees the frames the runs processed)."""
    import nnnoiseless_amd as nn
    from nnnoiseless_amd import pcm
    files, lone = mono
    bd = nn.BatchDenoiser(4, lib=hostsim_lib)
    fp = pcm.FilePacker(bd, 1, STEP)
    for _ in range(2):
        outs, vads, _, _ = pc.run_packed(hostsim_lib, files, 1, 4, STEP, packer=fp)
        pc.assert_files_equal(outs, vads, files, 1, lone)
        assert bd.num_held() == 0
    x = np.stack([files[0][:3 * pc.FRAME, 0]] * 4).reshape(4, 3, pc.FRAME)
    o, v = bd.process(x)
    for s in range(4):
        assert np.array_equal(pc.bits(o[s, 1:].reshape(-1, 1)), pc.bits(lone(0)[0])) and np.array_equal(pc.bits(v[:, s:s + 1]), pc.bits(lone(0)[1]))
    fp.close()
    bd.close()


def test_floors_apply(hostsim_lib):
    """Gain floors set on the batch apply to every file, whatever slot it lands in: equal to the lone run under the same floors."""
    files = pc.make_files([3, 2, 2, 1], 1, seed=5)
    outs, vads, _, _ = pc.run_packed(hostsim_lib, files, 1, 2, STEP, configure=lambda bd: bd.set_gain_floor([0, 1], 0.5))
    pc.assert_files_equal(outs, vads, files, 1, lambda i: pc.lone(hostsim_lib, files[i], 1, floors=0.5))
    plain = pc.lone(hostsim_lib, files[0], 1)[0]
    assert not np.array_equal(pc.bits(outs[0]), pc.bits(plain))   # (the floor is visible at all)


def test_plan_against_the_restated_rule(hostsim_lib):
    """nnn_pack_plan on a few hundred random length lists: slots, first steps and summary are the ten-line restatement's."""
    from nnnoiseless_amd import pcm
    rng = np.random.default_rng(6)
    for _ in range(300):
        n_slots, step = int(rng.integers(1, 9)), int(rng.integers(1, 7))
        frames = [int(f) for f in rng.integers(0, 15, int(rng.integers(0, 30)))]
        slot, first, s = pcm.pack_plan(n_slots, step, frames, hostsim_lib)
        w_slot, w_first, steps, pad = pc.plan_restated(n_slots, step, frames)
        assert list(slot) == w_slot and list(first) == w_first, (n_slots, step, frames)
        assert s["steps"] == len(steps) and s["launched"] == n_slots * sum(steps)
        assert s["useful"] == sum(frames) and s["padded"] == sum(pad) and s["files"] == sum(1 for f in frames if f)
        assert s["useful"] + s["padded"] == s["launched"] - s["held_frames"]
        assert max(pad, default=0) <= step - 1 and s["max_pad"] == max(pad, default=0)
    with pytest.raises(RuntimeError):
        pcm.pack_plan(0, 2, [1], hostsim_lib)
    with pytest.raises(RuntimeError):
        pcm.pack_plan(2, 0, [1], hostsim_lib)


def test_refusals_change_nothing(hostsim_lib, mono):
    """Every refusal of nnn_pack.h, each followed at once by a run that is still bit-exact."""
    import ctypes as C
    import nnnoiseless_amd as nn
    from nnnoiseless_amd import _ffi, pcm
    files, lone = mono
    L = hostsim_lib.L
    two = nn.BatchDenoiser(128, lib=hostsim_lib, groups=[(None, 64), (None, 64)])
    with pytest.raises(RuntimeError, match="model group"):
        pcm.FilePacker(two, 1)
    two.close()
    bd = nn.BatchDenoiser(S, lib=hostsim_lib)
    for ch, step, what in ((2, 2, "channels"), (0, 2, "channels"), (1, -1, "step_frames"), (1, bd.max_group_frames() + 1, "step_frames")):
        with pytest.raises(RuntimeError, match=what):
            pcm.FilePacker(bd, ch, step)
    assert not L.nnn_pack_create(None, 1, 0)
    fp = pcm.FilePacker(bd, 1, STEP)

    def good():
        outs, vads, _, _ = pc.run_packed(hostsim_lib, files, 1, S, STEP, packer=fp)
        pc.assert_files_equal(outs, vads, files, 1, lone)
        assert bd.num_held() == 0

    good()
    x = files[0].astype(np.float32).reshape(-1)
    out, vad = np.full(3 * pc.FRAME, pc.CANARY_F32, np.float32), np.full(8, pc.CANARY_F32, np.float32)
    tab = lambda *f: (_ffi.PackFile * 1)(_ffi.PackFile(*f))
    ok = (0, x.size, 0, 0)

    def raw(h=None, i=x, ni=x.size, fi=_ffi.PCM_F32, o=out, no=out.size, fo=_ffi.PCM_F32, v=vad, nv=vad.size, t=tab(*ok), n=1):
        return L.nnn_pack_run_host(fp._h if h is None else h, _ffi.ptr(i), ni, fi, _ffi.ptr(o), no, fo, _ffi.ptr(v), nv, t, n)

    def refused(match, **kw):
        assert raw(**kw) != 0 and re.search(match, hostsim_lib.error()), (match, hostsim_lib.error())
        assert (out == pc.CANARY_F32).all() and (vad == pc.CANARY_F32).all()
        good()

    assert L.nnn_pack_run_host(None, _ffi.ptr(x), x.size, 0, _ffi.ptr(out), out.size, 0, None, 0, tab(*ok), 1) != 0
    refused("null arena", i=None)
    refused("null arena", o=None)
    refused("null file list", t=None)
    refused("n_files", n=-1)
    refused("input format", fi=_ffi.PCM_F32_UNIT)
    refused("input format", fi=99)
    refused("output format", fo=_ffi.PACK_I24)
    refused("input span", ni=x.size - 1)
    refused("input span", t=tab(1, x.size, 0, 0))
    refused("output span", no=2 * pc.FRAME - 1)
    refused("output span", t=tab(0, x.size, out.size - 2 * pc.FRAME + 1, 0))
    refused("VAD span", nv=2)
    refused("VAD span", t=tab(0, x.size, 0, 6))
    bd.hold_streams([1])
    assert raw() != 0 and "held" in hostsim_lib.error()
    bd.resume_streams([1])
    good()
    bd.analyze(np.zeros((S, 1, 480), np.float32))
    assert raw() != 0 and "pending" in hostsim_lib.error()
    bd.reset()
    good()
    bd.set_inputs_ready(True)
    assert raw() != 0 and "inputs_ready" in hostsim_lib.error()
    bd.set_inputs_ready(False)
    good()
    assert raw() == 0   # (and the raw call itself works: the file's audio and VAD are its lone run's)
    assert np.array_equal(pc.bits(out[:2 * pc.FRAME]), pc.bits(lone(0)[0].reshape(-1))) and np.array_equal(pc.bits(vad[:3]), pc.bits(lone(0)[1].reshape(-1)))
    assert (out[2 * pc.FRAME:] == pc.CANARY_F32).all() and (vad[3:] == pc.CANARY_F32).all()
    fp.close()
    bd.close()


def test_a_faulted_batch_is_refused(hostsim_lib, mono):
    """A set nnn_batch_fault refuses the run (and reset clears it: the next run is bit-exact)."""
    import nnnoiseless_amd as nn
    from nnnoiseless_amd import pcm
    from nnnoiseless_amd.synthetic import make_streams
    files, lone = mono
    bd = nn.BatchDenoiser(5, lib=hostsim_lib)
    fp = pcm.FilePacker(bd, 1, STEP)
    hostsim_lib.check(hostsim_lib.L.nnn_batch_debug_withhold_flag(bd._h, 2))     # (the recipe of test_hostsim_round3)
    with pytest.raises(RuntimeError, match="hand-off"):
        bd.process(make_streams(0, 5, 6))
    assert bd.fault()
    with pytest.raises(RuntimeError, match="hand-off"):
        pc.run_packed(hostsim_lib, files, 1, 5, STEP, packer=fp)
    bd.reset()
    hostsim_lib.check(hostsim_lib.L.nnn_batch_debug_withhold_flag(bd._h, -1))
    assert not bd.fault()
    outs, vads, _, _ = pc.run_packed(hostsim_lib, files, 1, 5, STEP, packer=fp)
    pc.assert_files_equal(outs, vads, files, 1, lone)
    fp.close()
    bd.close()


def test_denoise_files_in_the_callers_order(hostsim_lib):
    """denoise_files sorts longest first, runs, and hands the results back in the caller's order: each is denoise_raw_i16's."""
    from nnnoiseless_amd import pcm
    files = [x.astype(np.int16) for x in pc.make_files([1, 3, 0, 2], 1, seed=7)]
    outs, vads, s = pcm.denoise_files(files, n_streams=2, lib=hostsim_lib)
    assert s["files"] == 3
    for i, x in enumerate(files):
        assert np.array_equal(outs[i], pcm.denoise_raw_i16(x, 1, lib=hostsim_lib)), i
        assert vads[i].shape == (x.shape[0] // pc.FRAME, 1)


def _write_wav(path, x, bits, channels, rate=48000):
    """x: int values in the `bits` range, [n, channels]."""
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(bits // 8)
        w.setframerate(rate)
        if bits == 16:
            w.writeframes(x.astype("<i2").tobytes())
        else:
            s = x.astype(np.int32).reshape(-1)
            w.writeframes(np.stack([s & 255, (s >> 8) & 255, (s >> 16) & 255], axis=1).astype(np.uint8).tobytes())


def test_riff_reader_and_cli(hostsim_lib, tmp_path, monkeypatch, capsys):
    """python -m nnnoiseless_amd.files on two tiny files the test writes, 16- and 24-bit: 48 kHz 16-bit WAVs out whose samples are the
    lone run's; a 44.1 kHz file is refused with a message that names pcm.Resampler."""
    import nnnoiseless_amd
    from nnnoiseless_amd import files as cli
    from nnnoiseless_amd import pcm
    a, b = pc.make_files([3, 2], 1, seed=8)
    b24 = (b.astype(np.int32) << 8) | 0x5A
    _write_wav(tmp_path / "a.wav", a, 16, 1)
    _write_wav(tmp_path / "b.wav", b24, 24, 1)
    _write_wav(tmp_path / "c.wav", a, 16, 1, rate=44100)
    fmt, ch, rate, data = cli.read_wav(str(tmp_path / "b.wav"))
    assert (fmt, ch, rate) == (pcm.PACK_I24, 1, 48000) and data.dtype == np.uint8 and data.size == b.size * 3
    monkeypatch.setattr(nnnoiseless_amd, "library", lambda: hostsim_lib)
    out_dir = tmp_path / "out"
    assert cli.main(["--out-dir", str(out_dir), "--streams", "2", str(tmp_path / "a.wav"), str(tmp_path / "b.wav")]) == 0
    for name, x in (("a.wav", a), ("b.wav", b)):
        with wave.open(str(out_dir / name), "rb") as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 48000)
            got = np.frombuffer(w.readframes(w.getnframes()), "<i2")
        assert np.array_equal(got, pcm.denoise_raw_i16(x.astype(np.int16), 1, lib=hostsim_lib).reshape(-1)), name
    with pytest.raises(SystemExit) as e:
        cli.main(["--out-dir", str(out_dir), str(tmp_path / "c.wav")])
    assert "pcm.Resampler" in str(e.value)
