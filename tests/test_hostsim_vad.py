"""The VAD-only calls (include/nnn_batch.h "VAD-only calls": nnn_batch_vad_*) under the test-only SIMT interpreter:
process_frame's voice-activity value without the denoiser behind it -- k_fft_feat, k_features, k_vad.

Shapes, inputs and the quiet stream are test_hostsim_split.py's: 70 streams (two tiles, six live lanes in the second) with
max_group_frames = 2 -- an 8-slot ring that wraps within the 12 frames -- in calls of (1, 2, 2, 1, 2, 2, 2) frames, and 3 streams in a
default batch, 27 frames in calls of (1, 2, 24).  Batch A (one-frame processing calls, taps on) and batch B (VAD calls, taps off) run
once per shape and library and are shared by the tests.  Every check is a function of (nn, lib, ...), so that test_gpu_vad.py makes the
same assertions on the device through the product library."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_hostsim_split import SHAPES, _bits, make_input

SENT = np.float32(-12345.0)
HEADER = ("magic", "version", "size", "gru_sizes", "mem_id", "last_period", "last_gain", "mem_hp_x")
ADVANCED = HEADER + ("input_mem", "cepstral_mem", "vad_gru")           # what a VAD call leaves as ordinary calls would
UNTOUCHED = ("synthesis_mem", "lastg", "noise_gru", "denoise_gru")     # ... and what keeps its bytes
MID = {"s70": (5, (1, 2, 2, 2)), "s3": (3, (24,))}                     # name: (frame at which A's records are taken, B's calls for the rest)
FRONT_TAPS = ("silence", "ex", "ep", "exp", "pitch")                   # readable with the taps off: what k_fft_feat (and k_pitch) left


def run_ordinary(nn, lib, x, mgf, mid):
    """Batch A: one-frame processing calls with the taps on.  vad [T, S], out [S, T, 480], the features / silence / front taps of every
    frame as [T, S, len], the records after frame mid - 1 and at the end."""
    S, T = x.shape[:2]
    a = nn.BatchDenoiser(S, lib=lib, max_group_frames=mgf, taps=True)
    names = ("features",) + FRONT_TAPS
    vad, out, taps, r = [], [], {k: [] for k in names}, {}
    for t in range(T):
        if t == mid:
            r["records_mid"] = a.export_streams(range(S))
        o, v = a.process(x[:, t:t + 1])
        vad.append(v[0].copy()), out.append(o)
        for k in names:
            taps[k].append(a.tap(k))
    r.update({k: np.stack(v) for k, v in taps.items()})
    r["vad"], r["out"], r["records"] = np.stack(vad), np.concatenate(out, 1), a.export_streams(range(S))
    return r


def run_vad(nn, lib, x, mgf, calls, taps=False, start=0, records=None, tap_names=()):
    """Batch B: VAD calls of the given lengths over x from frame `start` (after importing `records`).  vad [frames, S], the named taps
    after every call (its last frame) as {name: [(frame, [S, len])]}, the records at the end."""
    S = x.shape[0]
    b = nn.BatchDenoiser(S, lib=lib, max_group_frames=mgf, taps=taps)
    if records is not None:
        b.import_streams(range(S), records)
    v, seen, pos = [], {k: [] for k in tap_names}, start
    for n in calls:
        v.append(b.vad(x[:, pos:pos + n]))
        pos += n
        for k in tap_names:
            seen[k].append((pos - 1, b.tap(k)))
    assert not b.fault()
    return {"vad": np.concatenate(v), "taps": seen, "records": b.export_streams(range(S)), "batch": b}


_CACHE = {}


def shared_runs(nn, lib, name):
    """(x, A, B) of a shape on a library, made on first use."""
    key = (lib.path, name)
    if key not in _CACHE:
        mgf, calls = SHAPES[name][3], SHAPES[name][4]
        x = make_input(name)
        a = run_ordinary(nn, lib, x, mgf, MID[name][0])
        _CACHE[key] = (x, a, run_vad(nn, lib, x, mgf, calls, tap_names=FRONT_TAPS))
    return _CACHE[key]


# ---- the checks ------------------------------------------------------------------------------------------------------------------
def check_same_bits(nn, lib, oracle_mod, weights_bytes, name):
    """1. B's VAD rows are A's bit for bit on every frame; the quiet stream's silent frames occur in the middle of the run and read
    exactly 0; against the oracle |vad - ref| <= 1e-4, the bar of every VAD comparison of the suite on this generator."""
    x, a, b = shared_runs(nn, lib, name)
    assert np.array_equal(_bits(b["vad"]), _bits(a["vad"]))
    sil = a["silence"][:, SHAPES[name][5], 0]
    assert sil.any() and not sil[0] and not sil[-1], sil
    assert not _bits(b["vad"][sil.astype(bool), SHAPES[name][5]]).any()                 # +0.0, not merely == 0
    assert b["vad"][~a["silence"][:, :, 0].astype(bool)].min() > 0
    ref = oracle_mod.run_streams(oracle_mod.Model(weights_bytes), x, want=("vad",))["vad"]
    err = np.abs(b["vad"].T.astype(np.float64) - ref).max()
    print(name, "vad against the oracle: max abs err", err)
    assert err <= 1e-4, err


def check_records(nn, lib, name):
    """2. A's mid-run records imported into a fresh batch, the rest of the frames as VAD calls: the end records are A's end records in
    the header fields, INPUT_MEM, CEPSTRAL_MEM and VAD_GRU, and the IMPORTED bytes in SYNTHESIS_MEM, LASTG, NOISE_GRU, DENOISE_GRU."""
    from nnnoiseless_amd import _ffi
    x, a, _ = shared_runs(nn, lib, name)
    mid, calls = MID[name]
    b = run_vad(nn, lib, x, SHAPES[name][3], calls, start=mid, records=a["records_mid"])
    assert np.array_equal(_bits(b["vad"]), _bits(a["vad"][mid:]))
    f = _ffi.stream_state_field
    fed = np.abs(x[:, :mid]).max(axis=(1, 2)) > 0        # (make_streams keeps every 16th stream at digital silence: nothing to be non-zero there)
    assert fed.sum() >= x.shape[0] - 4
    for k in ADVANCED:
        assert np.array_equal(_bits(f(b["records"], k)), _bits(f(a["records"], k))), k
    for k in UNTOUCHED:
        imported = f(a["records_mid"], k)
        assert imported[fed, :GRU_WIDTH.get(k, imported.shape[1])].any(axis=1).all(), k   # non-zero for every stream that has seen a sample
        assert np.array_equal(_bits(f(b["records"], k)), _bits(imported)), k
        assert not np.array_equal(_bits(imported), _bits(f(a["records"], k))), k   # (A's own moved on: the comparison tells the two apart)


GRU_WIDTH = {"noise_gru": 48, "denoise_gru": 96}   # the built-in model's widths inside the 128-float record blocks


def check_alternation(nn, lib, name="s70"):
    """3. Ordinary one-frame calls (the fused tick), VAD calls, ordinary calls of 1 and of 2 frames, a last VAD call: the VAD of every
    frame of the run is A's bit for bit; the audio after the switch back is finite."""
    x, a, _ = shared_runs(nn, lib, name)
    S, T = x.shape[:2]
    m = nn.BatchDenoiser(S, lib=lib, max_group_frames=SHAPES[name][3])
    vad, audio, pos = [], [], 0
    for kind, n in (("p", 1), ("p", 1), ("p", 1), ("v", 2), ("v", 2), ("v", 1), ("p", 1), ("p", 2), ("v", 1)):
        if kind == "p":
            o, v = m.process(x[:, pos:pos + n])
            if pos >= 3:
                audio.append(o)
        else:
            v = m.vad(x[:, pos:pos + n])
        vad.append(v.copy())
        pos += n
    assert pos == T
    assert np.array_equal(_bits(np.concatenate(vad)), _bits(a["vad"]))
    assert all(np.isfinite(o).all() for o in audio) and len(audio) == 2


def check_held(nn, lib):
    """4. A whole 16-stream run and two scattered streams held: their entries of `vad` keep a sentinel (their input is NaN), their
    exported (parked) records do not change, every live stream's VAD is the nothing-held run's bit for bit, before, while and after.
    Everything held: the call succeeds and launches nothing, the frame count moves, and a resume + ordinary call gives what a batch
    gives that made the same hold / resume with no call in between."""
    from nnnoiseless_amd import _ffi
    x, a, b0 = shared_runs(nn, lib, "s70")
    S = x.shape[0]
    held = list(range(16, 32)) + [5, 66]
    live = [s for s in range(S) if s not in held]
    h = nn.BatchDenoiser(S, lib=lib, max_group_frames=2)
    for lo, hi in ((0, 1), (1, 3)):
        assert np.array_equal(_bits(h.vad(x[:, lo:hi])), _bits(b0["vad"][lo:hi]))
    h.hold_streams(held)
    parked = h.export_streams(held)
    for lo, hi in ((3, 5), (5, 6), (6, 8)):                                        # the ring wraps while they are held
        xa = x[:, lo:hi].copy()
        xa[held] = np.nan
        v = np.full((hi - lo, S), SENT, np.float32)
        h.vad(xa, vad=v)
        assert (_bits(v[:, held]) == _bits(SENT)).all()
        assert np.array_equal(_bits(v[:, live]), _bits(b0["vad"][lo:hi][:, live]))
        assert np.array_equal(h.export_streams(held), parked)
    h.resume_streams(held)
    for lo, hi in ((8, 10), (10, 12)):
        v = h.vad(x[:, lo:hi])
        assert np.array_equal(_bits(v[:, live]), _bits(b0["vad"][lo:hi][:, live]))
        assert np.isfinite(v).all()
    # every stream held
    x3 = make_input("s3")[:, :4]
    d, e = nn.BatchDenoiser(3, lib=lib), nn.BatchDenoiser(3, lib=lib)
    nan = np.full((3, 2, 480), np.nan, np.float32)
    for bd in (d, e):
        bd.process(x3[:, 0:2])
        bd.hold_streams(range(3))
    for n in (2, 1):
        v = np.full((n, 3), SENT, np.float32)
        d.vad(nan[:, :n], vad=v)
        assert (_bits(v) == _bits(SENT)).all()
    outs = []
    for bd in (d, e):
        bd.resume_streams(range(3))
        outs.append(bd.process(x3[:, 2:4]))
    assert np.array_equal(_bits(outs[0][0]), _bits(outs[1][0])) and np.array_equal(_bits(outs[0][1]), _bits(outs[1][1]))
    # ... and the frame count moved: discard_first drops the first frame of a batch that has seen none, and this one has
    f, g = nn.BatchDenoiser(3, lib=lib), nn.BatchDenoiser(3, lib=lib)
    f.hold_streams(range(3))
    f.vad(nan[:, :1], vad=np.full((1, 3), SENT, np.float32))
    f.resume_streams(range(3))
    pcm = np.ascontiguousarray(x3[:, :2].reshape(3, 960, 1))
    of, _ = f.process_pcm(pcm, _ffi.PCM_F32, discard_first=True)
    og, _ = g.process_pcm(pcm, _ffi.PCM_F32, discard_first=False)
    assert of.shape == og.shape == (3, 960, 1) and np.array_equal(_bits(of), _bits(og))


def check_formats(nn, lib):
    """5. Packed int16, two channels interleaved, through `vad`: the planar-float calls' bits (the inputs are integers)."""
    from nnnoiseless_amd import _ffi
    x, _, b0 = shared_runs(nn, lib, "s70")
    S, T = x.shape[:2]
    pcm = x.astype(np.int16).reshape(S // 2, 2, T * 480).transpose(0, 2, 1).copy()   # [G, T * 480, 2]: stream 2 g + c = channel c of group g
    b = nn.BatchDenoiser(S, lib=lib, max_group_frames=2)
    got, pos = [], 0
    for n in SHAPES["s70"][4]:
        got.append(b.vad(pcm[:, pos * 480:(pos + n) * 480], fmt=_ffi.PCM_I16, channels=2))
        pos += n
    assert np.array_equal(_bits(np.concatenate(got)), _bits(b0["vad"]))


def check_models(nn, lib, oracle_mod, weights_bytes):
    """6. Four models resident at once -- 16 / 20 / 40 / 72 on 64 streams, the built-in on 64, the widest the format allows (42 / 43 /
    42 / 127: three neuron blocks in the VAD GRU, 32 rows per k_vad block) on 64, sh.rnn on 5: the VAD of VAD calls is the ordinary
    path's on the same batch bit for bit, and within 1e-4 of the oracle per model."""
    from model_fixtures import make_model
    from nnnoiseless_amd.synthetic import make_streams
    blobs = [make_model(16, 20, 40, 72, seed=1), weights_bytes, make_model(42, 43, 42, 127, seed=3), open(os.path.join(GOLDEN, "sh.rnn"), "rb").read()]
    sizes = [64, 64, 64, 5]
    models = [None if bl is weights_bytes else nn.RnnModel.from_bytes(bl, lib=lib) for bl in blobs]
    x = make_streams(31, sum(sizes), 3)
    make = lambda: nn.BatchDenoiser(sum(sizes), lib=lib, groups=list(zip(models, sizes)))
    _, want = make().process(x)
    b = make()
    got = np.concatenate([b.vad(x[:, 0:1]), b.vad(x[:, 1:3])])
    assert np.array_equal(_bits(got), _bits(want))
    lo = 0
    for n, blob in zip(sizes, blobs):
        ref = oracle_mod.run_streams(oracle_mod.Model(blob), x[lo:lo + n], want=("vad",))["vad"]
        err = np.abs(got.T[lo:lo + n].astype(np.float64) - ref).max()
        print("model on streams", lo, "..", lo + n, "vad against the oracle: max abs err", err)
        assert err <= 1e-4, err
        lo += n


def check_refusals(nn, lib):
    """7. Every refusal returns non-zero with its text and leaves the records as they were; after nnn_batch_reset the same calls succeed."""
    from nnnoiseless_amd import _ffi
    x = make_input("s3")[:, :6]
    S = 3
    b = nn.BatchDenoiser(S, lib=lib, max_group_frames=2)
    b.process(x[:, 0:2])
    before = b.export_streams(range(S))
    L, p = b._lib.L, _ffi.ptr
    lay = _ffi.PcmLayout(_ffi.PCM_F32, 1, 0, 0, 2 * 480, 480)
    buf, v = np.ascontiguousarray(x[:, 2:4]), np.full((2, S), SENT, np.float32)

    def refused(call, text):
        with pytest.raises(RuntimeError, match=text):
            call()
        assert (_bits(v) == _bits(SENT)).all()
    for host in (True, False):
        fn = L.nnn_batch_vad_host if host else L.nnn_batch_vad_device
        tail = () if host else (None,)
        refused(lambda: b._lib.check(fn(b._h, None, p(v), 2, C.byref(lay), *tail)), "null buffer")
        refused(lambda: b._lib.check(fn(b._h, p(buf), None, 2, C.byref(lay), *tail)), "null buffer")
        refused(lambda: b._lib.check(fn(b._h, p(buf), p(v), 2, None, *tail)), "null layout")
        refused(lambda: b._lib.check(fn(b._h, p(buf), p(v), 0, C.byref(lay), *tail)), "n_frames")
        refused(lambda: b._lib.check(fn(b._h, p(buf), p(v), 3, C.byref(lay), *tail)), "n_frames")      # max_group_frames + 1
        disc = _ffi.PcmLayout(_ffi.PCM_F32, 1, 1, 0, 2 * 480, 480)
        refused(lambda: b._lib.check(fn(b._h, p(buf), p(v), 2, C.byref(disc), *tail)), "discard_first")
        bad = _ffi.PcmLayout(7, 1, 0, 0, 2 * 480, 480)
        refused(lambda: b._lib.check(fn(b._h, p(buf), p(v), 2, C.byref(bad), *tail)), "format")
        two = _ffi.PcmLayout(_ffi.PCM_F32, 2, 0, 0, 2 * 960, 960)                                        # 3 streams, 2 channels
        refused(lambda: b._lib.check(fn(b._h, p(buf), p(v), 2, C.byref(two), *tail)), "multiple of channels")
    with pytest.raises(RuntimeError, match="n_frames"):
        b.vad(x[:, 2:5])
    assert np.array_equal(b.export_streams(range(S)), before)
    # frames pending from an analyze
    twin = nn.BatchDenoiser(S, lib=lib, max_group_frames=2)
    twin.process(x[:, 0:2])
    for bd in (b, twin):
        bd.analyze(x[:, 2:4])
    refused(lambda: b.vad(x[:, 2:4], vad=v), "pending")
    refused(lambda: b._lib.check(L.nnn_batch_vad_device(b._h, p(buf), p(v), 2, C.byref(lay), None)), "pending")
    assert b.pending_frames() == 2
    g = np.full((2, S, 22), 0.7, np.float32)
    assert np.array_equal(_bits(b.synthesize(g)), _bits(twin.synthesize(g)))                             # the refused calls changed nothing
    assert np.array_equal(b.export_streams(range(S)), twin.export_streams(range(S)))
    # reset drops the pending frames: the same calls succeed, on a fresh batch
    b.analyze(x[:, 4:5])
    refused(lambda: b.vad(x[:, 0:2], vad=v), "pending")
    b.reset()
    fresh = nn.BatchDenoiser(S, lib=lib, max_group_frames=2)
    assert np.array_equal(_bits(b.vad(x[:, 0:2], vad=v)), _bits(fresh.process(x[:, 0:2])[1]))
    b._lib.check(L.nnn_batch_vad_host(b._h, p(buf), p(v), 2, C.byref(lay)))
    assert np.array_equal(_bits(v), _bits(fresh.process(x[:, 2:4])[1]))


def check_fft_feat(nn, lib, name="s70"):
    """8. k_fft_feat against k_fft_xp.  B ran with the taps off (k_fft_feat): what that launch and k_pitch leave -- SILENCE, EX, EP,
    EXP, PITCH, readable without the taps -- is A's after every call.  The FEATURES tap needs the taps on: a second run of VAD calls on
    a taps-on batch, which takes the k_fft_xp fallback, reads A's FEATURES and SILENCE bit for bit; and the taps-off VAD, the taps-on
    VAD and A's VAD agree on every frame.  (What k_fft_feat writes for the feature stage -- `cn`, the feature head -- has no tap of
    its own and is not compared directly with the taps off: it is held to A through the VAD bits and the CEPSTRAL_MEM records.)"""
    x, a, b = shared_runs(nn, lib, name)
    for k in FRONT_TAPS:
        assert len(b["taps"][k]) == len(SHAPES[name][4])
        for t, v in b["taps"][k]:
            assert np.array_equal(_bits(v), _bits(a[k][t])), (k, t)
    b2 = run_vad(nn, lib, x, SHAPES[name][3], SHAPES[name][4], taps=True, tap_names=("features", "silence", "vad"))
    for k in ("features", "silence"):
        for t, v in b2["taps"][k]:
            assert np.array_equal(_bits(v), _bits(a[k][t])), (k, t)
    for t, v in b2["taps"]["vad"]:
        assert np.array_equal(_bits(v[:, 0]), _bits(a["vad"][t])), t
    assert np.array_equal(_bits(b["vad"]), _bits(b2["vad"])) and np.array_equal(_bits(b["vad"]), _bits(a["vad"]))
    assert np.array_equal(b["records"], b2["records"])


# ---- under the interpreter --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nn():
    import nnnoiseless_amd
    return nnnoiseless_amd


@pytest.mark.parametrize("name", list(SHAPES))
def test_same_bits_as_the_ordinary_path(nn, hostsim_lib, oracle_mod, weights_bytes, name):
    check_same_bits(nn, hostsim_lib, oracle_mod, weights_bytes, name)


@pytest.mark.parametrize("name", list(SHAPES))
def test_records(nn, hostsim_lib, name):
    check_records(nn, hostsim_lib, name)


def test_alternating_modes(nn, hostsim_lib):
    check_alternation(nn, hostsim_lib)


def test_held_streams(nn, hostsim_lib):
    check_held(nn, hostsim_lib)


def test_formats(nn, hostsim_lib):
    check_formats(nn, hostsim_lib)


def test_models(nn, hostsim_lib, oracle_mod, weights_bytes):
    check_models(nn, hostsim_lib, oracle_mod, weights_bytes)


def test_refusals(nn, hostsim_lib):
    check_refusals(nn, hostsim_lib)


def test_fft_feat_against_fft_xp(nn, hostsim_lib):
    check_fft_feat(nn, hostsim_lib)
