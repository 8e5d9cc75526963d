"""The network-only calls (include/nnn_batch.h "Network-only calls": nnn_batch_network_*) under the test-only SIMT
interpreter: RnnState::compute on the caller's feature rows -- k_net -- between analyze and synthesize, and on its own.

Shapes, inputs and the quiet stream are test_hostsim_split.py's: 70 streams (two tiles, six live lanes in the second: rows past the batch,
whole blocks past it) with max_group_frames = 2 over 12 frames, and 3 streams in a default batch over 27 frames (one partial block, a
24-frame stretch).  Batch A (one-frame processing calls, taps on) runs once per shape and library and is shared by the tests; everything
else runs under NNN_RNN_ROWS = 16 and 32 (read at batch creation: k_net's rows per block).  Every check is a function of (nn, lib, ...),
so that test_gpu_network.py makes the same assertions on the device through the product library."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_hostsim_split import GRU, SHAPES, _bits, make_input, run_ordinary

SENT = np.float32(-12345.0)
ROWS = (16, 32)


@contextlib.contextmanager
def rnn_rows(rows):
    """NNN_RNN_ROWS for the batches created inside (None: the library's own choice)."""
    old = os.environ.get("NNN_RNN_ROWS")
    if rows is not None:
        os.environ["NNN_RNN_ROWS"] = str(rows)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("NNN_RNN_ROWS", None)
        else:
            os.environ["NNN_RNN_ROWS"] = old


_CACHE = {}


def shared_runs(nn, lib, name):
    """(x, A) of a shape on a library, made on first use and left unchanged: A's taps features [T, S, 42], silence [T, S], g_raw
    [T, S, 22], vad [T, S], its audio out [S, T, 480] and its end records."""
    key = (lib.path, name)
    if key not in _CACHE:
        x = make_input(name)
        a = run_ordinary(lib, x, SHAPES[name][3])
        a = dict(a, silence=np.ascontiguousarray(a["silence"][:, :, 0]), vad=np.ascontiguousarray(a["vad"][:, :, 0]))
        for v in a.values():
            v.setflags(write=False)
        _CACHE[key] = (x, a)
    return _CACHE[key]


def fields(nn):
    from nnnoiseless_amd import _ffi
    return _ffi.STREAM_STATE_FIELDS, _ffi.stream_state_field


def assert_records(nn, got, want_gru, want_rest, tag=""):
    """`got` has `want_gru`'s three GRU blocks and `want_rest`'s bits in every other field."""
    names, f = fields(nn)
    for k in names:
        w = want_gru if k in GRU else want_rest
        assert np.array_equal(_bits(f(got, k)), _bits(f(w, k))), (tag, k)


def quiet_silent(name, a):
    """(quiet stream, mask of its silent frames): they occur in the middle of the run."""
    q = SHAPES[name][5]
    sil = a["silence"][:, q].astype(bool)
    assert sil.any() and not sil[0] and not sil[-1], sil
    return q, sil


def network_calls(bd, a, calls, silence=True, start=0):
    """`network` calls of the given lengths over A's feature rows from frame `start`: (gains, vad) of all of them."""
    g, v, pos = [], [], start
    for n in calls:
        gi, vi = bd.network(a["features"][pos:pos + n], a["silence"][pos:pos + n] if silence else None)
        g.append(gi), v.append(vi)
        pos += n
    return np.concatenate(g), np.concatenate(v)


# ---- the checks ------------------------------------------------------------------------------------------------------------------
def check_triple(nn, lib, name, rows):
    """1. analyze -> network -> synthesize in the pair lengths of SHAPES is the ordinary path: gains = A's g_raw tap, VAD = A's vad
    tap, bit for bit; +0.0 rows on the quiet stream's silent frames; A's audio; A's end records in every field."""
    x, a = shared_runs(nn, lib, name)
    S = x.shape[0]
    with rnn_rows(rows):
        b = nn.BatchDenoiser(S, lib=lib, max_group_frames=SHAPES[name][3])
    gains, vad, out, pos = [], [], [], 0
    for n in SHAPES[name][4]:
        f, sil = b.analyze(x[:, pos:pos + n])
        assert b.pending_frames() == n
        g, v = b.network(f, sil)
        assert b.pending_frames() == n
        out.append(b.synthesize(g, v))
        gains.append(g), vad.append(v)
        pos += n
    gains, vad, out = np.concatenate(gains), np.concatenate(vad), np.concatenate(out, 1)
    assert not b.fault()
    assert np.array_equal(_bits(gains), _bits(a["g_raw"]))
    assert np.array_equal(_bits(vad), _bits(a["vad"]))
    q, sil = quiet_silent(name, a)
    assert not _bits(gains[sil, q]).any() and not _bits(vad[sil, q]).any()          # +0.0, not merely == 0
    assert vad[~a["silence"].astype(bool)].min() > 0
    assert np.array_equal(_bits(out), _bits(a["out"]))
    rec = b.export_streams(range(S))
    assert_records(nn, rec, a["records"], a["records"], "triple")
    assert np.array_equal(rec, a["records"])


def check_alone(nn, lib, name, rows):
    """2. A's feature / silence taps through `network` calls only, in calls of (1, 2, rest) and as ONE call of all frames (more than
    max_group_frames): A's gains and VAD both ways; the records have A's three GRU blocks and a fresh batch's bytes everywhere else;
    the frame count did not move: process_pcm(discard_first=True) afterwards still drops its first frame."""
    from nnnoiseless_amd import _ffi
    x, a = shared_runs(nn, lib, name)
    S, T = x.shape[:2]
    mgf = SHAPES[name][3]
    with rnn_rows(rows):
        c, one, fresh, twin = (nn.BatchDenoiser(S, lib=lib, max_group_frames=mgf) for _ in range(4))
    assert T > c.max_group_frames()
    blank = fresh.export_streams(range(S))
    for bd, calls in ((c, (1, 2, T - 3)), (one, (T,)), (twin, (T,))):
        g, v = network_calls(bd, a, calls)
        assert np.array_equal(_bits(g), _bits(a["g_raw"])), calls
        assert np.array_equal(_bits(v), _bits(a["vad"])), calls
        assert bd.pending_frames() == 0
        assert_records(nn, bd.export_streams(range(S)), a["records"], blank, calls)
    names, f = fields(nn)
    assert all(f(a["records"], k).any() for k in GRU)
    # a fresh batch's first frame under discard_first produces no audio: the 2 frames come back as 1, and it is the twin's second
    pcm = np.ascontiguousarray(x[:, :2].reshape(S, 960, 1))
    dropped, _ = c.process_pcm(pcm, _ffi.PCM_F32, discard_first=True)
    kept, _ = twin.process_pcm(pcm, _ffi.PCM_F32, discard_first=False)
    assert dropped.shape == (S, 480, 1) and kept.shape == (S, 960, 1)
    assert np.array_equal(_bits(dropped), _bits(kept[:, 480:]))


def check_silence_none(nn, lib, name, rows):
    """3. silence=None is a silence array of zeros, bit for bit (rows and records), and is not check 2's run: on the quiet stream's
    silent frames the network ran -- a VAD above zero -- and the state moved."""
    x, a = shared_runs(nn, lib, name)
    S, T = x.shape[:2]
    with rnn_rows(rows):
        e, z = (nn.BatchDenoiser(S, lib=lib, max_group_frames=SHAPES[name][3]) for _ in range(2))
    ge, ve = e.network(a["features"], None)
    gz, vz = z.network(a["features"], np.zeros((T, S), np.int32))
    assert np.array_equal(_bits(ge), _bits(gz)) and np.array_equal(_bits(ve), _bits(vz))
    rec = e.export_streams(range(S))
    assert np.array_equal(rec, z.export_streams(range(S)))
    q, sil = quiet_silent(name, a)
    assert (ve[sil, q] > 0).all() and _bits(ge[sil, q]).any()
    first = int(np.argmax(sil))
    assert np.array_equal(_bits(ge[:first, q]), _bits(a["g_raw"][:first, q])) and np.array_equal(_bits(ve[:first, q]), _bits(a["vad"][:first, q]))
    names, f = fields(nn)
    assert not np.array_equal(_bits(f(rec[q], "denoise_gru")), _bits(f(a["records"][q], "denoise_gru")))
    others = [s for s in range(S) if not a["silence"][:, s].any()]
    assert np.array_equal(_bits(ge[:, others]), _bits(a["g_raw"][:, others]))


def check_held(nn, lib, rows):
    """4. s70: one whole run of 16, a scattered few and all six lanes of tile 1's live part held, NaN in their feature rows, garbage in
    their silence entries, sentinels in their gains / VAD rows: the sentinels stay, live streams' bits are those of the unheld run, the
    held streams' exported records do not change, and after resume they continue like a twin that never saw the calls.  Everything
    held: the call succeeds and writes no row."""
    x, a = shared_runs(nn, lib, "s70")
    S, T = x.shape[:2]
    held = list(range(16, 32)) + [5, 40, 63] + list(range(64, 70))
    live = [s for s in range(S) if s not in held]
    with rnn_rows(rows):
        h, twin, d = nn.BatchDenoiser(S, lib=lib, max_group_frames=2), nn.BatchDenoiser(S, lib=lib, max_group_frames=2), nn.BatchDenoiser(3, lib=lib)
    for bd in (h, twin):
        g, v = network_calls(bd, a, (1, 2))
        assert np.array_equal(_bits(g), _bits(a["g_raw"][:3])) and np.array_equal(_bits(v), _bits(a["vad"][:3]))
    h.hold_streams(held)
    parked = h.export_streams(held)
    for lo, hi in ((3, 5), (5, 8)):
        fa, sa = a["features"][lo:hi].copy(), a["silence"][lo:hi].copy()
        fa[:, held], sa[:, held] = np.nan, 0x7FFFFFF1
        g, v = np.full((hi - lo, S, 22), SENT, np.float32), np.full((hi - lo, S), SENT, np.float32)
        h.network(fa, sa, gains=g, vad=v)
        assert (_bits(g[:, held]) == _bits(SENT)).all() and (_bits(v[:, held]) == _bits(SENT)).all()
        assert np.array_equal(_bits(g[:, live]), _bits(a["g_raw"][lo:hi][:, live])) and np.array_equal(_bits(v[:, live]), _bits(a["vad"][lo:hi][:, live]))
        assert np.array_equal(h.export_streams(held), parked)
    h.resume_streams(held)
    g, v = network_calls(h, a, (2, 2), start=8)
    gt, vt = network_calls(twin, a, (2, 2), start=8)                  # for the held streams frames 8 .. 11 follow frame 2
    assert np.array_equal(_bits(g[:, live]), _bits(a["g_raw"][8:][:, live])) and np.array_equal(_bits(v[:, live]), _bits(a["vad"][8:][:, live]))
    assert np.array_equal(_bits(g[:, held]), _bits(gt[:, held])) and np.array_equal(_bits(v[:, held]), _bits(vt[:, held]))
    assert np.array_equal(h.export_streams(held), twin.export_streams(held))
    assert np.isfinite(g).all() and np.isfinite(v).all()
    # every stream held
    _, a3 = shared_runs(nn, lib, "s3")
    d.network(a3["features"][:2], a3["silence"][:2])
    d.hold_streams(range(3))
    before = d.export_streams(range(3))
    for n in (2, 30):
        g, v = np.full((n, 3, 22), SENT, np.float32), np.full((n, 3), SENT, np.float32)
        d.network(np.full((n, 3, 42), np.nan, np.float32), np.full((n, 3), 7, np.int32), gains=g, vad=v)
        assert (_bits(g) == _bits(SENT)).all() and (_bits(v) == _bits(SENT)).all()
    assert np.array_equal(d.export_streams(range(3)), before)
    d.resume_streams(range(3))
    g, v = d.network(a3["features"][2:4], a3["silence"][2:4])
    assert np.array_equal(_bits(g), _bits(a3["g_raw"][2:4])) and np.array_equal(_bits(v), _bits(a3["vad"][2:4]))


def check_alternation(nn, lib, rows, name="s70"):
    """5. Ordinary one-frame calls and triples of 1 and 2 frames in turn over the run: audio, VAD and end records are the all-ordinary
    run's bit for bit."""
    x, a = shared_runs(nn, lib, name)
    S, T = x.shape[:2]
    with rnn_rows(rows):
        m = nn.BatchDenoiser(S, lib=lib, max_group_frames=SHAPES[name][3])
    out, vad, pos = [], [], 0
    for kind, n in (("p", 1), ("t", 2), ("p", 1), ("t", 1), ("p", 1), ("t", 2), ("p", 1), ("t", 2), ("p", 1)):
        if kind == "p":
            o, v = m.process(x[:, pos:pos + n])
        else:
            f, sil = m.analyze(x[:, pos:pos + n])
            g, v = m.network(f, sil)
            o = m.synthesize(g, v)
        out.append(o), vad.append(v.copy())
        pos += n
    assert pos == T
    assert np.array_equal(_bits(np.concatenate(out, 1)), _bits(a["out"]))
    assert np.array_equal(_bits(np.concatenate(vad)), _bits(a["vad"]))
    assert np.array_equal(m.export_streams(range(S)), a["records"])


def check_models(nn, lib, oracle_mod, weights_bytes, rows):
    """6. A grouped batch, the built-in model on 64 streams and tests/golden/sh.rnn on 6: each group's gains / VAD are the bits of
    that model's own ordinary run (the g_raw / vad taps of one-frame processing calls on the same grouping), and within the bar
    test_hostsim_parity.py holds the g_raw and vad taps to against the oracle: 2e-5 of the row's peak (at least of 1)."""
    from nnnoiseless_amd.synthetic import make_streams
    blobs, sizes = [weights_bytes, open(os.path.join(GOLDEN, "sh.rnn"), "rb").read()], [64, 6]
    models = [None, nn.RnnModel.from_bytes(blobs[1], lib=lib)]
    S, T = sum(sizes), 3
    x = make_streams(31, S, T)
    key = (lib.path, "models")
    if key not in _CACHE:
        o = nn.BatchDenoiser(S, lib=lib, groups=list(zip(models, sizes)), taps=True)
        taps = {k: [] for k in ("features", "silence", "g_raw", "vad")}
        for t in range(T):
            o.process(x[:, t:t + 1])
            for k in taps:
                taps[k].append(o.tap(k))
        ref = [oracle_mod.run_streams(oracle_mod.Model(bl), x[lo:lo + n], want=("g_raw", "vad"))
               for bl, lo, n in zip(blobs, (0, sizes[0]), sizes)]
        _CACHE[key] = ({k: np.stack(v) for k, v in taps.items()}, ref)
    want, ref = _CACHE[key]
    with rnn_rows(rows):
        b = nn.BatchDenoiser(S, lib=lib, groups=list(zip(models, sizes)))
    g, v = b.network(want["features"], np.ascontiguousarray(want["silence"][:, :, 0]))
    assert np.array_equal(_bits(g), _bits(want["g_raw"])) and np.array_equal(_bits(v), _bits(want["vad"][:, :, 0]))
    assert not np.array_equal(_bits(g[:, :6]), _bits(g[:, 64:]))
    lo = 0
    for n, r in zip(sizes, ref):
        rg, rv = r["g_raw"].astype(np.float64), r["vad"].astype(np.float64)          # [n, T, 22], [n, T]
        eg = np.abs(g[:, lo:lo + n].transpose(1, 0, 2) - rg).max(axis=2)
        ev = np.abs(v[:, lo:lo + n].T - rv)
        print("model on streams", lo, "..", lo + n, "against the oracle: g_raw max abs err", eg.max(), "vad", ev.max())
        assert (eg <= 2e-5 * np.maximum(np.abs(rg).max(axis=2), 1.0)).all(), eg.max()
        assert (ev <= 2e-5 * np.maximum(np.abs(rv), 1.0)).all(), ev.max()
        lo += n


def check_refusals(nn, lib, rows):
    """7. Every refusal returns non-zero with its text and changes nothing (an untouched twin has the same records); the call is
    accepted with frames pending and leaves pending_frames as it was, while a second analyze still refuses; the host and device
    variants agree bit for bit (the device variant on page-locked rows, which the device reads and writes in place)."""
    from nnnoiseless_amd import _ffi
    x, a = shared_runs(nn, lib, "s3")
    S = 3
    with rnn_rows(rows):
        b, twin, dv = (nn.BatchDenoiser(S, lib=lib, max_group_frames=2) for _ in range(3))
    for bd in (b, twin, dv):
        bd.process(x[:, 0:2])
    L, p = lib.L, _ffi.ptr
    f, sil = np.ascontiguousarray(a["features"][2:4]), np.ascontiguousarray(a["silence"][2:4])
    g, v = np.full((2, S, 22), SENT, np.float32), np.full((2, S), SENT, np.float32)
    odd = lambda arr: C.c_void_p(arr.ctypes.data + 2)

    def refused(call, text):
        with pytest.raises(RuntimeError, match=text):
            call()
        assert (_bits(g) == _bits(SENT)).all() and (_bits(v) == _bits(SENT)).all()
    for host in (True, False):
        fn = L.nnn_batch_network_host if host else L.nnn_batch_network_device
        tail = () if host else (None,)
        refused(lambda: lib.check(fn(None, p(f), p(sil), p(g), p(v), 2, *tail)), "null batch")
        refused(lambda: lib.check(fn(b._h, None, p(sil), p(g), p(v), 2, *tail)), "null buffer")
        refused(lambda: lib.check(fn(b._h, p(f), p(sil), None, p(v), 2, *tail)), "null buffer")
        refused(lambda: lib.check(fn(b._h, p(f), p(sil), p(g), p(v), 0, *tail)), "n_frames")
        refused(lambda: lib.check(fn(b._h, p(f), p(sil), p(g), p(v), -3, *tail)), "n_frames")
        refused(lambda: lib.check(fn(b._h, odd(f), p(sil), p(g), p(v), 1, *tail)), "aligned")
        refused(lambda: lib.check(fn(b._h, p(f), odd(sil), p(g), p(v), 1, *tail)), "aligned")
        refused(lambda: lib.check(fn(b._h, p(f), p(sil), odd(g), p(v), 1, *tail)), "aligned")
        refused(lambda: lib.check(fn(b._h, p(f), p(sil), p(g), odd(v), 1, *tail)), "aligned")
    with pytest.raises(ValueError):
        b.network(a["features"][2:2])
    assert np.array_equal(b.export_streams(range(S)), twin.export_streams(range(S)))
    # frames pending: accepted, pending_frames as it was, a second analyze still refuses; host and device variants agree
    fb, sb = b.analyze(x[:, 2:4])
    fd, sd = dv.analyze(x[:, 2:4])
    twin.analyze(x[:, 2:4])
    assert np.array_equal(_bits(fb), _bits(f)) and np.array_equal(sb, sil)
    b.network(fb, sb, gains=g, vad=v)
    assert b.pending_frames() == 2
    refused_plain = pytest.raises(RuntimeError, match="pending")
    with refused_plain:
        b.analyze(x[:, 2:4])
    df, ds = nn.pinned_empty((2, S, 42), np.float32, lib=lib), nn.pinned_empty((2, S), np.int32, lib=lib)
    dg, dvad, dg2 = nn.pinned_empty((2, S, 22), np.float32, lib=lib), nn.pinned_empty((2, S), np.float32, lib=lib), nn.pinned_empty((2, S, 22), np.float32, lib=lib)
    df[...], ds[...], dg[...], dvad[...], dg2[...] = fd, sd, SENT, SENT, SENT
    dv.network_device(df.ctypes.data, ds.ctypes.data, dg.ctypes.data, dvad.ctypes.data, 2)
    dv.synchronize()
    assert dv.pending_frames() == 2
    assert np.array_equal(_bits(dg), _bits(g)) and np.array_equal(_bits(dvad), _bits(v))
    assert np.array_equal(_bits(g), _bits(a["g_raw"][2:4])) and np.array_equal(_bits(v), _bits(a["vad"][2:4]))
    o_b, o_dv, o_t = b.synthesize(g, v), dv.synthesize(dg, dvad), twin.synthesize(a["g_raw"][2:4], a["vad"][2:4])
    assert np.array_equal(_bits(o_b), _bits(a["out"][:, 2:4])) and np.array_equal(_bits(o_dv), _bits(o_b)) and np.array_equal(_bits(o_t), _bits(o_b))
    rb = b.export_streams(range(S))
    assert np.array_equal(rb, dv.export_streams(range(S)))
    assert_records(nn, twin.export_streams(range(S)), twin.export_streams(range(S)), rb, "twin")   # (the twin's GRUs never ran frames 2, 3)
    # a set fault refuses
    lib.check(L.nnn_batch_debug_withhold_flag(b._h, 0))                # (the next frame's hand-off flag: the second frame of the call waits for it)
    with pytest.raises(RuntimeError, match="hand-off"):
        b.process(x[:, 4:6])
    assert b.fault()
    g[...], v[...] = SENT, SENT
    refused(lambda: b.network(f, sil, gains=g, vad=v), "hand-off")
    refused(lambda: lib.check(L.nnn_batch_network_device(b._h, p(f), p(sil), p(g), p(v), 2, None)), "hand-off")
    lib.check(L.nnn_batch_debug_withhold_flag(b._h, -1))
    b.reset()
    assert not b.fault()


# ---- under the interpreter --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nn():
    import nnnoiseless_amd
    return nnnoiseless_amd


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_triple_is_the_ordinary_path(nn, hostsim_lib, name, rows):
    check_triple(nn, hostsim_lib, name, rows)


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_network_alone(nn, hostsim_lib, name, rows):
    check_alone(nn, hostsim_lib, name, rows)


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_silence_none(nn, hostsim_lib, name, rows):
    check_silence_none(nn, hostsim_lib, name, rows)


@pytest.mark.parametrize("rows", ROWS)
def test_held_streams(nn, hostsim_lib, rows):
    check_held(nn, hostsim_lib, rows)


@pytest.mark.parametrize("rows", ROWS)
def test_alternation(nn, hostsim_lib, rows):
    check_alternation(nn, hostsim_lib, rows)


@pytest.mark.parametrize("rows", ROWS)
def test_models(nn, hostsim_lib, oracle_mod, weights_bytes, rows):
    check_models(nn, hostsim_lib, oracle_mod, weights_bytes, rows)


@pytest.mark.parametrize("rows", ROWS)
def test_refusals_and_protocol(nn, hostsim_lib, rows):
    check_refusals(nn, hostsim_lib, rows)

