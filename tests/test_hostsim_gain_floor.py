"""Per-stream gain floors (include/nnn_batch.h "Gain floors": nnn_batch_set_gain_floor / get / num_floored) under the
test-only SIMT interpreter: an ordinary call under floors F is, bit for bit, analyze -> network -> max(gains, F) -> synthesize.

Shapes, inputs, the quiet stream and the shared unfloored run A are test_hostsim_split.py's and test_hostsim_network.py's.  Floor pattern P
puts every case into each 16-row block: stream 4k off, 4k+1 one scalar 10^(-18/20) set with bands = 1, 4k+2 a 22-band ramp 0.05 .. 0.95,
4k+3 1.0.  Every comparison is of bits; what is expected comes from the triple (batch D, made once per shape and library) and from numpy,
never from the floored path.  Every check is a function of (nn, lib, ...), so that test_gpu_gain_floor.py makes the same assertions on the
device through the product library."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_hostsim_network import ROWS, assert_records, quiet_silent, rnn_rows, shared_runs
from test_hostsim_split import GRU, SHAPES, _bits, run_split

# the gains sinks: (nnn_batch_set_back_end mode, NNN_RNN_WF_MIN_G at creation).  fused / rnn16: k_back<true> / k_back<false> for every group;
# wf / plain: three launches with k_rnn_wf / k_rnn forced as test_hostsim_parity.py forces them (a value above the longest group: k_rnn)
SINKS = {"fused": (2, None), "rnn16": (4, None), "wf": (0, "1"), "plain": (0, "99")}
DB18 = np.float32(10.0 ** (-18.0 / 20.0))
RAMP = np.linspace(0.05, 0.95, 22).astype(np.float32)


@contextlib.contextmanager
def env(name, value):
    old = os.environ.get(name)
    if value is not None:
        os.environ[name] = value
    try:
        yield
    finally:
        if value is not None:
            if old is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = old


def pattern(S):
    """P as [S, 22]."""
    p = np.zeros((S, 22), np.float32)
    p[1::4], p[2::4], p[3::4] = DB18, RAMP, 1.0
    return p


def set_pattern(b, S, only=None):
    """P through the three ways of giving floors: a scalar per stream (bands = 1), rows of 22, one scalar for the list; 4k is never named."""
    keep = (lambda idx: [s for s in idx if s in only]) if only is not None else (lambda idx: list(idx))
    i1, i2, i3 = keep(range(1, S, 4)), keep(range(2, S, 4)), keep(range(3, S, 4))
    b.set_gain_floor(i1, np.full(len(i1), DB18, np.float32))
    b.set_gain_floor(i2, np.tile(RAMP, (len(i2), 1)))
    b.set_gain_floor(i3, 1.0)


def make_batch(nn, lib, S, mgf, rows=None, sink=None, **kw):
    mode, wf = SINKS[sink] if sink else (None, None)
    with rnn_rows(rows), env("NNN_RNN_WF_MIN_G", wf):
        b = nn.BatchDenoiser(S, lib=lib, max_group_frames=mgf, **kw)
    if mode is not None:
        b.set_back_end(mode)
    return b


def run_calls(b, x, calls, start=0):
    """Processing calls of the given lengths from frame `start`: audio [S, sum, 480], VAD [sum, S]."""
    out, vad, pos = [], [], start
    for n in calls:
        o, v = b.process(x[:, pos:pos + n])
        out.append(o), vad.append(v.copy())
        pos += n
    return np.concatenate(out, 1), np.concatenate(vad)


def run_triple(b, x, calls, floors, start=0, taps=None):
    """analyze -> network -> np.maximum(gains, floors of the frame) -> synthesize in the given lengths; floors [S, 22] or per frame
    [T, S, 22] (indexed by frame of x).  taps: a list that receives (g_raw, g) of each triple's last frame."""
    out, vad, pos = [], [], start
    for n in calls:
        f, sil = b.analyze(x[:, pos:pos + n])
        g, v = b.network(f, sil)
        fl = floors if floors.ndim == 2 else floors[pos:pos + n]
        out.append(b.synthesize(np.maximum(g, fl), v))
        vad.append(v)
        if taps is not None:
            taps.append((b.tap("g_raw"), b.tap("g")))
        pos += n
    return np.concatenate(out, 1), np.concatenate(vad)


_D = {}


def triple_runs(nn, lib, name):
    """Batch D of a shape on a library, made on first use and left unchanged: the triple under P in the lengths of SHAPES -- out
    [S, T, 480], vad [T, S], the records at the end, the g_raw / g taps after each triple and the frame log [T, S, 24]."""
    key = (lib.path, name)
    if key not in _D:
        x, a = shared_runs(nn, lib, name)
        S, T = x.shape[:2]
        d = nn.BatchDenoiser(S, lib=lib, max_group_frames=SHAPES[name][3], taps=True)
        log = nn.pinned_empty((T, S, 24), np.uint32, lib=lib)
        log[...] = 0
        d.set_frame_log(log.ctypes.data, T)
        taps = []
        out, vad = run_triple(d, x, SHAPES[name][4], pattern(S), taps=taps)
        r = {"out": out, "vad": vad, "records": d.export_streams(range(S)), "log": np.array(log),
             "g_raw": np.stack([t[0] for t in taps]), "g": np.stack([t[1] for t in taps])}
        assert d.num_floored() == 0
        for v in r.values():
            v.setflags(write=False)
        _D[key] = r
    return _D[key]


def smoothed(a, floors):
    """The smoothed gains of every frame in numpy f32 from A's raw gains and silence flags: g = max(max(g_raw, F), 0.6 lastg), lastg = g on
    non-silent frames (one rounding per operation, as the kernels).  [T, S, 22], and the mask of non-silent (frame, stream)."""
    T, S = a["silence"].shape
    lastg, g_all = np.zeros((S, 22), np.float32), []
    for t in range(T):
        fl = floors if floors.ndim == 2 else floors[t]
        live = a["silence"][t] == 0
        g = np.maximum(np.maximum(a["g_raw"][t], fl), np.float32(0.6) * lastg)
        lastg = np.where(live[:, None], g, lastg)
        g_all.append(g)
    return np.stack(g_all), a["silence"] == 0


# ---- the checks ------------------------------------------------------------------------------------------------------------------
def check_equals_triple(nn, lib, name, rows, sink, calls=None):
    """1. Batch C under P through one gains sink, the frames in the call lengths of SHAPES (or `calls`), taps on: after every call the
    g_raw tap is max(A's g_raw, P) on non-silent streams and +0.0 on silent ones, and the g tap is D's; the frame log's smoothed gains are D's
    on every frame and numpy's chain on every non-silent one; VAD is A's; audio and every record are D's; the streams 4k (floor off) have A's
    audio and records; the three GRU blocks of every record are A's."""
    x, a = shared_runs(nn, lib, name)
    d = triple_runs(nn, lib, name)
    S, T = x.shape[:2]
    P = pattern(S)
    calls = calls or SHAPES[name][4]
    c = make_batch(nn, lib, S, SHAPES[name][3], rows, sink, taps=True)
    log = nn.pinned_empty((T, S, 24), np.uint32, lib=lib)
    log[...] = 0
    c.set_frame_log(log.ctypes.data, T)
    set_pattern(c, S)
    assert c.num_floored() == S - len(range(0, S, 4))
    out, vad, pos = [], [], 0
    for i, n in enumerate(calls):
        o, v = c.process(x[:, pos:pos + n])
        out.append(o), vad.append(v.copy())
        pos += n
        live = a["silence"][pos - 1] == 0
        want = np.where(live[:, None], np.maximum(a["g_raw"][pos - 1], P), np.float32(0.0))
        assert np.array_equal(_bits(c.tap("g_raw")), _bits(want)), (i, pos)
        if calls == SHAPES[name][4]:
            assert np.array_equal(_bits(c.tap("g")), _bits(d["g"][i])), (i, pos)
            assert np.array_equal(_bits(d["g_raw"][i]), _bits(want)), (i, pos)        # (the triple's tap holds the caller's clamped gains)
    out, vad = np.concatenate(out, 1), np.concatenate(vad)
    assert pos == T and not c.fault()
    q, sil = quiet_silent(name, a)
    assert P[q].any()                                                                  # the quiet stream is a floored one
    g_np, live = smoothed(a, P)
    assert np.array_equal(np.array(log), d["log"])
    assert np.array_equal(_bits(np.array(log)[:, :, 2:].view(np.float32)[live]), _bits(g_np[live]))
    assert np.array_equal(_bits(vad), _bits(a["vad"]))
    assert np.array_equal(_bits(out), _bits(d["out"]))
    rec = c.export_streams(range(S))
    assert np.array_equal(rec, d["records"])
    assert np.array_equal(_bits(out[0::4]), _bits(a["out"][0::4])) and np.array_equal(rec[0::4], a["records"][0::4])
    assert not np.array_equal(_bits(out[1::4]), _bits(a["out"][1::4]))                 # ... and a floor is not a no-op
    assert_records(nn, rec, a["records"], rec, "GRU blocks")
    spoke = live.any(axis=0)                                                            # (a stream that was never non-silent never took a gain)
    assert (nn.stream_state_field(rec, "lastg")[spoke] >= P[spoke]).all() and spoke.sum() > S // 2


def check_one_call(nn, lib, rows, sink):
    """1b. s3 as ONE call of all 27 frames: more than one group (24 + 3).  Not pipelined: a pipelined call needs 32 frames, which the
    shapes do not have; the schedule places launches and no kernel looks at it (test_hostsim_schedule.py)."""
    check_equals_triple(nn, lib, "s3", rows, sink, calls=(SHAPES["s3"][2],))


def check_all_ones(nn, lib, name, rows, sink):
    """2. Floor 1.0 on every stream: run_split with gains of all ones, in audio and records (but the GRU blocks, which the split run never
    touches: A's)."""
    x, a = shared_runs(nn, lib, name)
    S, T = x.shape[:2]
    want = run_split(lib, x, SHAPES[name][3], SHAPES[name][4], np.ones((T, S, 22), np.float32))
    c = make_batch(nn, lib, S, SHAPES[name][3], rows, sink)
    c.set_gain_floor(range(S), 1.0)
    assert c.num_floored() == S
    out, _ = run_calls(c, x, SHAPES[name][4])
    assert np.array_equal(_bits(out), _bits(want["out"]))
    assert_records(nn, c.export_streams(range(S)), a["records"], want["records"], "all ones")


def check_off_is_off(nn, lib, name, rows, sink):
    """3. An empty set only, and P followed by all zeros before the first frame: A bit for bit, num_floored() 0 for both."""
    x, a = shared_runs(nn, lib, name)
    S = x.shape[0]
    e, z = (make_batch(nn, lib, S, SHAPES[name][3], rows, sink) for _ in range(2))
    lib.check(lib.L.nnn_batch_set_gain_floor(e._h, None, 0, None, 1))
    set_pattern(z, S)
    assert z.num_floored() > 0
    z.set_gain_floor(range(S), np.zeros((S, 22), np.float32))
    for b in (e, z):
        assert b.num_floored() == 0 and not b.gain_floor().any()
        out, vad = run_calls(b, x, SHAPES[name][4])
        assert np.array_equal(_bits(out), _bits(a["out"])) and np.array_equal(_bits(vad), _bits(a["vad"]))
        assert np.array_equal(b.export_streams(range(S)), a["records"])


def check_change_between_calls(nn, lib, name, rows, sink):
    """4. Three frames under P, then Q (P rotated by one stream), then the rest: the triple with the per-frame floors; get returns what
    was set, bands = 1 as 22 equal values."""
    x, a = shared_runs(nn, lib, name)
    S, T = x.shape[:2]
    mgf, calls = SHAPES[name][3], SHAPES[name][4]
    assert calls[:2] == (1, 2)
    P = pattern(S)
    Q = np.roll(P, 1, axis=0)
    per_frame = np.stack([P] * 3 + [Q] * (T - 3))
    c, d = make_batch(nn, lib, S, mgf, rows, sink), nn.BatchDenoiser(S, lib=lib, max_group_frames=mgf)
    set_pattern(c, S)
    assert np.array_equal(_bits(c.gain_floor()), _bits(P))
    assert np.array_equal(_bits(c.gain_floor([S - 1, 1, 1])), _bits(P[[S - 1, 1, 1]]))   # (a get's list may repeat)
    o1, v1 = run_calls(c, x, calls[:2])
    c.set_gain_floor(range(S), Q)
    assert np.array_equal(_bits(c.gain_floor()), _bits(Q)) and c.num_floored() == int(Q.any(axis=1).sum())
    o2, v2 = run_calls(c, x, calls[2:], start=3)
    want, want_vad = run_triple(d, x, calls, per_frame)
    assert np.array_equal(_bits(np.concatenate([o1, o2], 1)), _bits(want))
    assert np.array_equal(_bits(np.concatenate([v1, v2])), _bits(want_vad)) and np.array_equal(_bits(want_vad), _bits(a["vad"]))
    assert np.array_equal(c.export_streams(range(S)), d.export_streams(range(S)))
    assert not np.array_equal(_bits(want), _bits(triple_runs(nn, lib, name)["out"]))


def check_lifecycle(nn, lib, rows, sink, name="s70"):
    """5. Floors are configuration: they read back unchanged after reset_streams, import_streams, hold + resume, reset and save_state /
    load_state; the state image has the size of an unfloored batch's; clone carries them and the clone continues bit-identically;
    device_bytes grows by the floor rows (88 bytes per padded stream) at the first set and never again.  A floor set while a stream is
    held (input NaN) applies from its first live frame; the live streams' bits are the nothing-held run's."""
    x, a = shared_runs(nn, lib, name)
    d = triple_runs(nn, lib, name)
    S, T = x.shape[:2]
    mgf, calls = SHAPES[name][3], SHAPES[name][4]
    assert calls[:5] == (1, 2, 2, 1, 2) and name == "s70"
    P = pattern(S)
    b = make_batch(nn, lib, S, mgf, rows, sink)
    plain_bytes, plain_state = b.device_bytes(), len(b.save_state())
    assert not b.gain_floor().any() and b.device_bytes() == plain_bytes                # (a get allocates nothing)
    b.set_gain_floor([1], DB18)
    rows_bytes = (S + 63) // 64 * 64 * 88
    assert b.device_bytes() == plain_bytes + rows_bytes
    set_pattern(b, S)
    assert b.device_bytes() == plain_bytes + rows_bytes and len(b.save_state()) == plain_state
    o, _ = run_calls(b, x, calls[:2])
    assert np.array_equal(_bits(o), _bits(d["out"][:, :3]))

    def same():
        assert np.array_equal(_bits(b.gain_floor()), _bits(P)) and b.num_floored() == int(P.any(axis=1).sum())
    rec = b.export_streams([2])
    b.reset_streams([1, 6, 69]), same()
    b.import_streams([3], rec), same()
    assert b.device_bytes() == plain_bytes + rows_bytes
    b.hold_streams([1, 2, 66]), b.resume_streams([1, 2, 66]), same()
    with_park = b.device_bytes()                                                       # (the first hold made the parked records)
    snap = b.save_state()
    b.reset(), same()
    fresh, _ = run_calls(b, x, calls[:1])
    assert np.array_equal(_bits(fresh), _bits(d["out"][:, :1]))                        # (a reset batch under P starts as D started)
    b.load_state(snap), same()
    b.set_gain_floor([0], 0.0), same()
    assert b.device_bytes() == with_park
    c = b.clone()
    assert np.array_equal(_bits(c.gain_floor()), _bits(P)) and c.num_floored() == b.num_floored()
    ob, vb = run_calls(b, x, calls[2:4], start=3)
    oc, vc = run_calls(c, x, calls[2:4], start=3)
    assert np.array_equal(_bits(ob), _bits(oc)) and np.array_equal(_bits(vb), _bits(vc))
    assert np.array_equal(b.export_streams(range(S)), c.export_streams(range(S)))
    # set while held
    held = [5, 6, 7] + list(range(64, 70))
    live = [s for s in range(S) if s not in held]
    h, twin = make_batch(nn, lib, S, mgf, rows, sink), make_batch(nn, lib, S, mgf, rows, sink)
    for bd in (h, twin):
        set_pattern(bd, S, only=set(live))
        run_calls(bd, x, calls[:2])
    h.hold_streams(held)
    for bd in (h, twin):
        set_pattern(bd, S, only=set(held))                                             # (h: while they are held)
    assert np.array_equal(_bits(h.gain_floor()), _bits(P))
    xa = x.copy()
    xa[held, 3:8] = np.nan
    oh, _ = run_calls(h, xa, calls[2:5], start=3)
    assert np.array_equal(_bits(oh[live]), _bits(d["out"][live, 3:8]))
    h.resume_streams(held)
    oh, _ = run_calls(h, x, (2, 2), start=8)                                           # for the held streams frames 8 .. 11 follow frame 2
    ot, _ = run_calls(twin, x, (2, 2), start=8)
    assert np.array_equal(_bits(oh[live]), _bits(d["out"][live, 8:12]))
    assert np.array_equal(_bits(oh[held]), _bits(ot[held])) and np.isfinite(oh).all()
    rh = h.export_streams(held)
    assert np.array_equal(rh, twin.export_streams(held))
    spoke = (a["silence"][8:, held] == 0).any(axis=0)                                  # (non-silent after the resume: the floor was applied)
    assert (nn.stream_state_field(rh, "lastg")[spoke] >= P[held][spoke]).all() and (P[held][spoke].any(axis=1)).sum() >= 4


def check_other_calls(nn, lib, name, rows, sink):
    """6. On a floored batch network returns A's raw gains and VAD, vad returns A's VAD, and synthesize fed gains below the floor
    produces what an unfloored batch produces from them."""
    x, a = shared_runs(nn, lib, name)
    S, T = x.shape[:2]
    mgf = SHAPES[name][3]
    n, v, f, u = (make_batch(nn, lib, S, mgf, rows, sink) for _ in range(4))
    for b in (n, v, f):
        set_pattern(b, S)
    g, vd = n.network(a["features"], a["silence"])
    assert np.array_equal(_bits(g), _bits(a["g_raw"])) and np.array_equal(_bits(vd), _bits(a["vad"]))
    k = v.max_group_frames()
    assert np.array_equal(_bits(v.vad(x[:, :k])), _bits(a["vad"][:k]))
    low = np.full((k, S, 22), 0.01, np.float32)
    for b in (f, u):
        b.analyze(x[:, :k])
    of, ou = f.synthesize(low), u.synthesize(low)
    assert np.array_equal(_bits(of), _bits(ou)) and np.array_equal(f.export_streams(range(S)), u.export_streams(range(S)))
    assert np.array_equal(_bits(f.gain_floor()), _bits(pattern(S)))


def check_pcm(nn, lib, rows, sink):
    """7a. s70 as 2-channel int16 through one process_pcm call with discard_first, under P: the same layout through the triple's PCM
    variants (the inputs are integers: both boundaries see A's samples)."""
    from nnnoiseless_amd import _ffi
    x, a = shared_runs(nn, lib, "s70")
    S, T = x.shape[:2]
    P = pattern(S)
    pcm = x.astype(np.int16).reshape(S // 2, 2, T * 480).transpose(0, 2, 1).copy()     # [G, T * 480, 2]
    c, d = make_batch(nn, lib, S, 2, rows, sink), nn.BatchDenoiser(S, lib=lib, max_group_frames=2)
    set_pattern(c, S)
    got, vad = c.process_pcm(pcm, _ffi.PCM_I16, channels=2, discard_first=True)
    want, pos = [], 0
    for n in SHAPES["s70"][4]:
        f, sil = d.analyze(pcm[:, pos * 480:(pos + n) * 480], fmt=_ffi.PCM_I16, channels=2)
        g, v = d.network(f, sil)
        want.append(d.synthesize(np.maximum(g, P), v, fmt=_ffi.PCM_I16, channels=2, discard_first=True))
        pos += n
    want = np.concatenate(want, 1)
    assert got.shape == (S // 2, (T - 1) * 480, 2) and np.array_equal(got, want)
    assert np.array_equal(_bits(vad), _bits(a["vad"]))
    assert np.array_equal(c.export_streams(range(S)), d.export_streams(range(S)))
    assert np.array_equal(c.export_streams(range(S)), triple_runs(nn, lib, "s70")["records"])


def check_host_chunks(nn, lib, rows, sink, name="s70"):
    """7b. One host-buffer call of all frames under NNN_HOST_CHUNK=1 (a chunk per frame) and in one piece (NNN_HOST_CHUNK=0): D's audio,
    A's VAD, D's records both ways."""
    x, a = shared_runs(nn, lib, name)
    d = triple_runs(nn, lib, name)
    S = x.shape[0]
    for chunk in ("1", "0"):
        with env("NNN_HOST_CHUNK", chunk):
            b = make_batch(nn, lib, S, SHAPES[name][3], rows, sink)
        set_pattern(b, S)
        out, vad = b.process(x)
        assert np.array_equal(_bits(out), _bits(d["out"])), chunk
        assert np.array_equal(_bits(vad), _bits(a["vad"])) and np.array_equal(b.export_streams(range(S)), d["records"]), chunk


def check_models(nn, lib, weights_bytes, rows, sink):
    """7c. A grouped batch, the built-in model on 64 streams and tests/golden/sh.rnn on 6, under P: its own triple, in audio, VAD and
    records; each model group's launch reads its own streams' floor rows."""
    from nnnoiseless_amd.synthetic import make_streams
    sizes = [64, 6]
    models = [None, nn.RnnModel.from_bytes(open(os.path.join(GOLDEN, "sh.rnn"), "rb").read(), lib=lib)]
    S, T = sum(sizes), 3
    x = make_streams(31, S, T)
    P = pattern(S)
    mode, wf = SINKS[sink]
    with rnn_rows(rows), env("NNN_RNN_WF_MIN_G", wf):
        c, d, u = (nn.BatchDenoiser(S, lib=lib, groups=list(zip(models, sizes))) for _ in range(3))
    c.set_back_end(mode)
    set_pattern(c, S)
    out, vad = c.process(x)
    want, want_vad = run_triple(d, x, (T,), P)
    plain, _ = u.process(x)
    assert np.array_equal(_bits(out), _bits(want)) and np.array_equal(_bits(vad), _bits(want_vad))
    assert np.array_equal(c.export_streams(range(S)), d.export_streams(range(S)))
    assert np.array_equal(_bits(out[0::4]), _bits(plain[0::4]))
    for lo, hi in ((0, 64), (64, 70)):
        fl = np.arange(lo, hi)[np.arange(lo, hi) % 4 != 0]
        assert not np.array_equal(_bits(out[fl]), _bits(plain[fl])), (lo, hi)


def check_refusals(nn, lib, rows, sink):
    """8. Every refusal returns non-zero with its text and changes nothing: the floors read back as before, and the run continued after
    the refused calls is bit-identical to a twin's without them."""
    x, a = shared_runs(nn, lib, "s3")
    S = 3
    P = pattern(S)
    b, twin = (make_batch(nn, lib, S, None, rows, sink) for _ in range(2))
    for bd in (b, twin):
        set_pattern(bd, S)
        run_calls(bd, x, (2,))
    L = lib.L
    ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
    ints = lambda *v: np.array(v, np.int32).ctypes.data_as(ip)
    flts = lambda *v: np.array(v, np.float32).ctypes.data_as(fp)
    buf = np.zeros((3, 22), np.float32)

    def refused(rc_of, text):
        with pytest.raises(RuntimeError, match=text):
            lib.check(rc_of())
    refused(lambda: L.nnn_batch_set_gain_floor(None, ints(0), 1, flts(0.5), 1), "null batch")
    refused(lambda: L.nnn_batch_set_gain_floor(b._h, None, 1, flts(0.5), 1), "null stream list")
    refused(lambda: L.nnn_batch_set_gain_floor(b._h, ints(0), 1, None, 1), "null floor")
    refused(lambda: L.nnn_batch_set_gain_floor(b._h, ints(0), -1, flts(0.5), 1), "negative")
    refused(lambda: L.nnn_batch_set_gain_floor(b._h, ints(0, S), 2, flts(0.5, 0.5), 1), "outside")
    refused(lambda: L.nnn_batch_set_gain_floor(b._h, ints(-1), 1, flts(0.5), 1), "outside")
    refused(lambda: L.nnn_batch_set_gain_floor(b._h, ints(0, 2, 0), 3, flts(0.5, 0.5, 0.5), 1), "twice")
    for bands in (0, 2, 21, 23):
        refused(lambda: L.nnn_batch_set_gain_floor(b._h, ints(0), 1, flts(*([0.5] * 23)), bands), "bands")
    for bad in (np.nan, -0.1, 1.5, np.inf, -np.inf):
        refused(lambda: L.nnn_batch_set_gain_floor(b._h, ints(0, 2), 2, flts(0.5, bad), 1), "outside \\[0, 1\\]")
        refused(lambda: L.nnn_batch_set_gain_floor(b._h, ints(0), 1, flts(*([0.5] * 21 + [bad])), 22), "outside \\[0, 1\\]")
    refused(lambda: L.nnn_batch_get_gain_floor(None, ints(0), 1, buf.ctypes.data_as(fp)), "null batch")
    refused(lambda: L.nnn_batch_get_gain_floor(b._h, None, 1, buf.ctypes.data_as(fp)), "null stream list")
    refused(lambda: L.nnn_batch_get_gain_floor(b._h, ints(0), 1, None), "null floor")
    refused(lambda: L.nnn_batch_get_gain_floor(b._h, ints(0), -2, buf.ctypes.data_as(fp)), "negative")
    refused(lambda: L.nnn_batch_get_gain_floor(b._h, ints(S), 1, buf.ctypes.data_as(fp)), "outside")
    assert not buf.any() and L.nnn_batch_num_floored(None) == 0
    for bad in ([[0.5] * 21], np.zeros((2, 22)), np.zeros((1, 22, 1))):
        with pytest.raises(ValueError):
            b.set_gain_floor([0], bad)
    assert np.array_equal(_bits(b.gain_floor()), _bits(P)) and b.num_floored() == twin.num_floored() == 2
    ob, vb = run_calls(b, x, (1, 2), start=2)
    ot, vt = run_calls(twin, x, (1, 2), start=2)
    assert np.array_equal(_bits(ob), _bits(ot)) and np.array_equal(_bits(vb), _bits(vt))
    assert np.array_equal(b.export_streams(range(S)), twin.export_streams(range(S)))
    assert np.array_equal(_bits(ob), _bits(triple_runs(nn, lib, "s3")["out"][:, 2:5]))
    assert nn.attenuation_limit_db(18) == pytest.approx(10 ** -0.9) and nn.attenuation_limit_db(0) == 1.0


def check_node(nn, lib, devices=(0, 0, 0)):
    """9. P over a node of three shards of s70 (24 + 23 + 23 streams), set with lists that straddle the shard edges, one of them out of
    order: the single batch's triple (D) in audio and VAD; get and num_floored agree with the single batch; a list with a bad entry on
    the last shard changes no shard."""
    x, a = shared_runs(nn, lib, "s70")
    d = triple_runs(nn, lib, "s70")
    S, T = x.shape[:2]
    P = pattern(S)
    node = nn.NodeDenoiser(S, devices, lib=lib, max_group_frames=2)
    edges = [lo for _, lo, _ in node.shards()][1:]
    assert len(edges) == 2 and all(0 < e < S for e in edges)
    i1, i2, i3 = list(range(1, S, 4)), list(range(2, S, 4))[::-1], list(range(3, S, 4))
    for idx in (i1, i2, i3):
        assert all(min(idx) < e <= max(idx) for e in edges)
    with pytest.raises(RuntimeError, match="outside \\[0, 1\\]"):
        node.set_gain_floor([0, S - 1], [0.5, 1.5])
    with pytest.raises(RuntimeError, match="twice"):
        node.set_gain_floor([0, S - 1, S - 1], 0.5)
    assert node.num_floored() == 0 and not node.gain_floor().any()
    node.set_gain_floor(i1, np.full(len(i1), DB18, np.float32))
    node.set_gain_floor(i2, np.tile(RAMP, (len(i2), 1)))
    node.set_gain_floor(i3, 1.0)
    assert np.array_equal(_bits(node.gain_floor()), _bits(P)) and node.num_floored() == int(P.any(axis=1).sum())
    pick = [edges[0], 2, edges[1] - 1, S - 1]
    assert np.array_equal(_bits(node.gain_floor(pick)), _bits(P[pick]))
    out, vad, pos = [], [], 0
    for n in SHAPES["s70"][4]:
        o, v = node.process(x[:, pos:pos + n])
        out.append(o), vad.append(v.copy())
        pos += n
    assert np.array_equal(_bits(np.concatenate(out, 1)), _bits(d["out"])) and np.array_equal(_bits(np.concatenate(vad)), _bits(a["vad"]))
    assert np.array_equal(node.export_streams(range(S)), d["records"])
    node.close()


# ---- under the interpreter --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nn():
    import nnnoiseless_amd
    return nnnoiseless_amd


@pytest.mark.parametrize("sink", list(SINKS))
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_floored_call_is_the_clamped_triple(nn, hostsim_lib, name, rows, sink):
    check_equals_triple(nn, hostsim_lib, name, rows, sink)


@pytest.mark.parametrize("sink", list(SINKS))
def test_one_call_of_all_frames(nn, hostsim_lib, sink):
    check_one_call(nn, hostsim_lib, 32, sink)


@pytest.mark.parametrize("name,sink", [("s70", "fused"), ("s70", "plain"), ("s3", "rnn16"), ("s3", "wf")])
def test_floor_one_is_unit_gains(nn, hostsim_lib, name, sink):
    check_all_ones(nn, hostsim_lib, name, 16 if sink == "plain" else 32, sink)


@pytest.mark.parametrize("sink", list(SINKS))
def test_off_is_off(nn, hostsim_lib, sink):
    check_off_is_off(nn, hostsim_lib, "s70" if sink in ("fused", "plain") else "s3", 32, sink)


@pytest.mark.parametrize("name,sink", [("s70", "wf"), ("s70", "rnn16"), ("s3", "fused"), ("s3", "plain")])
def test_changing_floors_between_calls(nn, hostsim_lib, name, sink):
    check_change_between_calls(nn, hostsim_lib, name, 32 if sink == "plain" else 16, sink)


@pytest.mark.parametrize("sink", ["fused", "wf"])
def test_lifecycle(nn, hostsim_lib, sink):
    check_lifecycle(nn, hostsim_lib, 32, sink)


@pytest.mark.parametrize("name", list(SHAPES))
def test_other_calls_ignore_floors(nn, hostsim_lib, name):
    check_other_calls(nn, hostsim_lib, name, 16, "fused")


@pytest.mark.parametrize("sink", ["fused", "wf"])
def test_pcm_boundary(nn, hostsim_lib, sink):
    check_pcm(nn, hostsim_lib, 32, sink)


@pytest.mark.parametrize("sink", ["rnn16", "wf"])
def test_host_chunks(nn, hostsim_lib, sink):
    check_host_chunks(nn, hostsim_lib, 16, sink)


@pytest.mark.parametrize("sink", ["wf", "plain"])      # (a model outside k_back's shape class sends every group of the batch through three launches)
def test_grouped_models(nn, hostsim_lib, weights_bytes, sink):
    check_models(nn, hostsim_lib, weights_bytes, 16 if sink == "plain" else 32, sink)


def test_refusals(nn, hostsim_lib):
    check_refusals(nn, hostsim_lib, 32, "fused")


def test_node(nn, hostsim_lib, monkeypatch):
    monkeypatch.setenv("NNN_NODE_THREADS", "0")          # (the interpreter runs kernels on the calling thread and is not re-entrant)
    check_node(nn, hostsim_lib)
