"""Channel-linked gains (include/nnn_batch.h "Channel link": nnn_batch_set_channel_link / get) under the test-only SIMT
interpreter: an ordinary call under link (channels, mode) and floors F is, bit for bit, analyze -> network -> the link formula in numpy on
the returned gains with the returned silence flags -> synthesize.

Shapes: 72 streams (one full tile plus half a 16-row run of tail: padding rows beside live ones; a multiple of 2 and of 4) x 12 frames with
max_group_frames = 2, and 4 streams x 27 frames with a 24-frame group.  Inputs are make_streams rounded to integers -- the channels of a
group are independent signals, so their network gains differ -- with test_hostsim_split.py's QUIET stream, whose stretch of exact zeros
gives its group silent and non-silent members in the same frame.  Batch A (the unlinked run: one-frame calls, taps on) and batch D (the
triple under a link) run once per shape, link and library and are shared.  Every comparison is of bits; what is expected comes from the
triple and from numpy's max / min, never from the linked path.  NNN_RNN_ROWS is read by k_rnn's launch (the `plain` sink) alone: the other
three sinks run 16 rows per block whatever it says, so the interpreter file runs them under one value and `plain` under both;
test_gpu_channel_link.py runs every pair.  Every check is a function of (nn, lib, ...), so that the GPU file makes the same assertions on
the device through the product library."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_hostsim_gain_floor import SINKS, env, make_batch, pattern, run_calls, set_pattern, smoothed
from test_hostsim_network import ROWS, assert_records, rnn_rows
from test_hostsim_split import GRU, _bits, quiet_stream, run_ordinary

SHAPES = {   # name: (make_streams seed, streams, frames, max_group_frames, frames of each call, quiet stream, its zero stretch)
    "s72": (41, 72, 12, 2, (1, 2, 2, 1, 2, 2, 2), 7, (4, 8)),
    "s4": (11, 4, 27, None, (1, 2, 24), 1, (5, 9)),
}
LINKS = [(2, "max"), (2, "min"), (4, "max"), (4, "min")]
SENT = np.float32(-12345.0)


def make_input(name):
    from nnnoiseless_amd.synthetic import make_streams
    seed, S, T, _, _, quiet, zeros = SHAPES[name]
    x = np.clip(np.round(make_streams(seed, S, T)), -32768, 32767).astype(np.float32)
    x[quiet] = quiet_stream(T, zeros)
    return x


def link_np(g, sil, channels, mode, live=None, floors=None):
    """The contract's formula on gains [n, S, 22] with silence flags [n, S]: over the members of a group that are live and not silent, the
    max / min per band; then each stream's floor.  Rows that are no members come back as they went in."""
    n, S = sil.shape
    m = sil == 0
    if live is not None:
        m = m & np.asarray(live, bool)[None, :]
    out = g.copy()
    if channels > 1 and mode != "off":
        gg, mm = g.reshape(n, S // channels, channels, 22), m.reshape(n, S // channels, channels, 1)
        if mode == "max":
            r = np.where(mm, gg, np.float32(-np.inf)).max(axis=2, keepdims=True)
        else:
            r = np.where(mm, gg, np.float32(np.inf)).min(axis=2, keepdims=True)
        out = np.where(mm, r, gg).reshape(n, S, 22).astype(np.float32)
    if floors is not None:
        out = np.where(m[:, :, None], np.maximum(out, floors), out)
    return out


def run_triple(b, x, calls, link, floors=None, live=None, start=0):
    """analyze -> network -> link_np -> synthesize in the given lengths from frame `start`; link: (channels, mode) or one per call."""
    out, vad, pos = [], [], start
    for i, n in enumerate(calls):
        ch, mode = link[i] if isinstance(link, list) else link
        f, sil = b.analyze(x[:, pos:pos + n])
        g, v = b.network(f, sil)
        out.append(b.synthesize(link_np(g, sil, ch, mode, live, floors), v))
        vad.append(v)
        pos += n
    return np.concatenate(out, 1), np.concatenate(vad)


_A, _D = {}, {}


def shared_runs(nn, lib, name):
    """(x, A) of a shape on a library, made on first use and left unchanged: the unlinked run's taps features [T, S, 42], silence [T, S],
    g_raw [T, S, 22], vad [T, S], its audio out [S, T, 480] and its end records."""
    key = (lib.path, name)
    if key not in _A:
        x = make_input(name)
        a = run_ordinary(lib, x, SHAPES[name][3])
        a = dict(a, silence=np.ascontiguousarray(a["silence"][:, :, 0]), vad=np.ascontiguousarray(a["vad"][:, :, 0]))
        for v in a.values():
            v.setflags(write=False)
        q = a["silence"][:, SHAPES[name][5]].astype(bool)
        assert q.any() and not q[0] and not q[-1], q                                   # the quiet stream goes silent in the middle of the run
        _A[key] = (x, a)
    return _A[key]


def triple_runs(nn, lib, name, link):
    """Batch D of a shape under a link on a library, made on first use and left unchanged: the triple in the call lengths of SHAPES -- out
    [S, T, 480], vad [T, S], the records at the end and the frame log [T, S, 24]."""
    key = (lib.path, name, link)
    if key not in _D:
        x, a = shared_runs(nn, lib, name)
        S, T = x.shape[:2]
        d = nn.BatchDenoiser(S, lib=lib, max_group_frames=SHAPES[name][3])
        log = nn.pinned_empty((T, S, 24), np.uint32, lib=lib)
        log[...] = 0
        d.set_frame_log(log.ctypes.data, T)
        out, vad = run_triple(d, x, SHAPES[name][4], link)
        assert d.channel_link() == (1, "off")
        r = {"out": out, "vad": vad, "records": d.export_streams(range(S)), "log": np.array(log)}
        for v in r.values():
            v.setflags(write=False)
        _D[key] = r
    return _D[key]


def linked_batch(nn, lib, S, mgf, rows, sink, link, **kw):
    b = make_batch(nn, lib, S, mgf, rows, sink, **kw)
    b.set_channel_link(*link)
    assert b.channel_link() == link
    return b


# ---- the checks ------------------------------------------------------------------------------------------------------------------
def check_equals_triple(nn, lib, name, rows, sink, link):
    """1, 2. Batch C under a link through one gains sink, the frames in the call lengths of SHAPES, taps on: after every call the g_raw tap
    is numpy's link of A's raw gains (+0.0 on silent streams); the frame log is D's on every frame and numpy's smoothing chain over the
    linked gains on every non-silent one; audio and every record are D's; VAD and the three GRU blocks of every record are A's, the
    unlinked run's; the audio is not A's."""
    x, a = shared_runs(nn, lib, name)
    d = triple_runs(nn, lib, name, link)
    S, T = x.shape[:2]
    want_raw = link_np(a["g_raw"], a["silence"], *link)
    assert not np.array_equal(_bits(want_raw), _bits(a["g_raw"]))
    c = linked_batch(nn, lib, S, SHAPES[name][3], rows, sink, link, taps=True)
    log = nn.pinned_empty((T, S, 24), np.uint32, lib=lib)
    log[...] = 0
    c.set_frame_log(log.ctypes.data, T)
    out, vad, pos = [], [], 0
    for i, n in enumerate(SHAPES[name][4]):
        o, v = c.process(x[:, pos:pos + n])
        out.append(o), vad.append(v.copy())
        pos += n
        assert np.array_equal(_bits(c.tap("g_raw")), _bits(want_raw[pos - 1])), (i, pos)
    out, vad = np.concatenate(out, 1), np.concatenate(vad)
    assert pos == T and not c.fault()
    g_np, live = smoothed({"g_raw": want_raw, "silence": a["silence"]}, np.zeros((S, 22), np.float32))
    assert np.array_equal(np.array(log), d["log"])
    assert np.array_equal(_bits(np.array(log)[:, :, 2:].view(np.float32)[live]), _bits(g_np[live]))
    assert np.array_equal(_bits(out), _bits(d["out"]))
    rec = c.export_streams(range(S))
    assert np.array_equal(rec, d["records"])
    assert np.array_equal(_bits(vad), _bits(a["vad"])) and np.array_equal(_bits(vad), _bits(d["vad"]))
    assert_records(nn, rec, a["records"], rec, "GRU blocks")
    assert not np.array_equal(_bits(out), _bits(a["out"]))                             # ... and a link is not a no-op
    assert c.channel_link() == link


def check_silent_member(nn, lib, rows, sink, link, name="s4"):
    """3. One-frame calls, taps on, so that every frame's raw gains show.  While the quiet stream's frames are silent its g_raw row is
    +0.0, its VAD 0 and its lastg what it was at its last non-silent frame, and the other members of its group are linked among
    themselves: a lone partner (2 channels) has A's own raw gains, three partners (4 channels) the max / min of the three.  Beside it a
    batch whose stream 2 is digital silence from the first sample: that stream's audio, lastg and VAD are the unlinked batch's over the
    whole run, and with 2 channels so are its lone partner's."""
    x, a = shared_runs(nn, lib, name)
    S, T = x.shape[:2]
    ch, mode = link
    q = SHAPES[name][5]
    sil = a["silence"][:, q].astype(bool)
    mates = [s for s in range(q // ch * ch, q // ch * ch + ch) if s != q]
    op = np.maximum if mode == "max" else np.minimum
    c = linked_batch(nn, lib, S, SHAPES[name][3], rows, sink, link, taps=True)
    lastg = None
    for t in range(T):
        _, v = c.process(x[:, t:t + 1])
        raw = c.tap("g_raw")
        among = a["g_raw"][t][mates[0]]
        for s in mates[1:]:
            among = op(among, a["g_raw"][t][s])
        lg = nn.stream_state_field(c.export_streams([q]), "lastg")
        if sil[t]:
            assert not raw[q].any() and not np.signbit(raw[q]).any() and v[0, q] == 0 and a["vad"][t, q] == 0, t
            assert np.array_equal(_bits(lg), _bits(lastg)), t
            for s in mates:
                assert np.array_equal(_bits(raw[s]), _bits(among)), (t, s)
        else:
            assert np.array_equal(_bits(raw[q]), _bits(op(among, a["g_raw"][t][q]))), t
        lastg = lg
    z = x[:, :6].copy()
    z[2] = 0
    u, w = make_batch(nn, lib, S, SHAPES[name][3], rows, sink), linked_batch(nn, lib, S, SHAPES[name][3], rows, sink, link)
    (ou, vu), (ow, vw) = u.process(z), w.process(z)
    same = [2, 3] if ch == 2 else [2]
    ru, rw = u.export_streams(same), w.export_streams(same)
    assert np.array_equal(_bits(ow[same]), _bits(ou[same])) and np.array_equal(_bits(vw), _bits(vu)) and not vw[:, 2].any()
    assert np.array_equal(ru, rw) and not nn.stream_state_field(rw[:1], "lastg").any()
    assert not np.array_equal(_bits(ow[:2]), _bits(ou[:2]))                            # (the streams that do have partners are linked)


def check_held(nn, lib, rows, sink, link, name="s72"):
    """4. Three frames with everybody, then five with a few streams held -- one of a pair, two of a four, a whole group, a tail stream;
    NaN in their input, sentinels in their rows of out and vad -- then four with everybody again: the live members are linked among
    themselves (the triple's bits, with the held streams out of the formula), the held streams' rows and records do not change, and
    after resume they join the link from their first frame (all rows are the triple's)."""
    x, a = shared_runs(nn, lib, name)
    S, T = x.shape[:2]
    mgf, calls = SHAPES[name][3], SHAPES[name][4]
    assert calls[:5] == (1, 2, 2, 1, 2) and name == "s72"
    held = [2, 9, 10, 12, 13, 14, 15, 70]
    live = np.ones(S, bool)
    live[held] = False
    c, d = linked_batch(nn, lib, S, mgf, rows, sink, link), nn.BatchDenoiser(S, lib=lib, max_group_frames=mgf)
    o1, _ = run_calls(c, x, calls[:2])
    w1, _ = run_triple(d, x, calls[:2], link)
    assert np.array_equal(_bits(o1), _bits(w1))
    c.hold_streams(held), d.hold_streams(held)
    parked = c.export_streams(held)
    xa = x.copy()
    xa[held, 3:8] = np.nan
    pos = 3
    for n in calls[2:5]:
        o, v = np.full((S, n, 480), SENT, np.float32), np.full((n, S), SENT, np.float32)
        c.process(xa[:, pos:pos + n], out=o, vad=v)
        w, wv = run_triple(d, xa, (n,), link, live=live, start=pos)
        assert (_bits(o[held]) == _bits(SENT)).all() and (_bits(v[:, held]) == _bits(SENT)).all(), pos
        assert np.array_equal(_bits(o[live]), _bits(w[live])) and np.array_equal(_bits(v[:, live]), _bits(wv[:, live])), pos
        assert np.array_equal(_bits(v[:, live]), _bits(a["vad"][pos:pos + n][:, live])), pos
        assert np.array_equal(c.export_streams(held), parked), pos
        pos += n
    assert c.channel_link() == link and c.num_held() == len(held)
    c.resume_streams(held), d.resume_streams(held)
    o2, v2 = run_calls(c, x, (2, 2), start=8)                                          # for the held streams frames 8 .. 11 follow frame 2
    w2, wv2 = run_triple(d, x, (2, 2), link, start=8)
    assert np.array_equal(_bits(o2), _bits(w2)) and np.array_equal(_bits(v2), _bits(wv2)) and np.isfinite(o2).all()
    assert np.array_equal(c.export_streams(range(S)), d.export_streams(range(S)))


def check_floors(nn, lib, name, rows, sink, link):
    """5. Link plus test_hostsim_gain_floor.py's floor pattern P: link first, then each stream's floor -- the triple with both."""
    x, a = shared_runs(nn, lib, name)
    S = x.shape[0]
    mgf, calls = SHAPES[name][3], SHAPES[name][4]
    P = pattern(S)
    c, d = linked_batch(nn, lib, S, mgf, rows, sink, link), nn.BatchDenoiser(S, lib=lib, max_group_frames=mgf)
    set_pattern(c, S)
    out, vad = run_calls(c, x, calls)
    want, want_vad = run_triple(d, x, calls, link, floors=P)
    assert np.array_equal(_bits(out), _bits(want)) and np.array_equal(_bits(vad), _bits(want_vad)) and np.array_equal(_bits(vad), _bits(a["vad"]))
    rec = c.export_streams(range(S))
    assert np.array_equal(rec, d.export_streams(range(S)))
    assert not np.array_equal(_bits(want), _bits(triple_runs(nn, lib, name, link)["out"]))   # (the floors are no no-op beside the link)
    spoke = (a["silence"] == 0).any(axis=0)
    assert (nn.stream_state_field(rec, "lastg")[spoke] >= P[spoke]).all()


def check_off_is_off(nn, lib, name, rows, sink):
    """6. channels = 1, NNN_LINK_OFF with 2 channels, and a batch that linked and switched it off before its first frame: A bit for bit;
    get says (1, "off") for all three."""
    x, a = shared_runs(nn, lib, name)
    S = x.shape[0]
    one, off, back = (make_batch(nn, lib, S, SHAPES[name][3], rows, sink) for _ in range(3))
    one.set_channel_link(1, "max")
    off.set_channel_link(2, "off")
    back.set_channel_link(4, "min")
    assert back.channel_link() == (4, "min")
    back.set_channel_link(1, "off")
    for b in (one, off, back):
        assert b.channel_link() == (1, "off")
        out, vad = run_calls(b, x, SHAPES[name][4])
        assert np.array_equal(_bits(out), _bits(a["out"])) and np.array_equal(_bits(vad), _bits(a["vad"]))
        assert np.array_equal(b.export_streams(range(S)), a["records"])


def check_change_between_calls(nn, lib, name, rows, sink):
    """7. Two calls under (2, max), two under (4, min), one unlinked, the rest under (4, max): the triple with each call's own link."""
    x, a = shared_runs(nn, lib, name)
    S = x.shape[0]
    mgf, calls = SHAPES[name][3], SHAPES[name][4]
    plan = ([(2, "max")] * 2 + [(4, "min")] * 2 + [(1, "off")] + [(4, "max")] * len(calls))[:len(calls)]
    c, d = make_batch(nn, lib, S, mgf, rows, sink), nn.BatchDenoiser(S, lib=lib, max_group_frames=mgf)
    out, vad, pos = [], [], 0
    for n, link in zip(calls, plan):
        c.set_channel_link(*link)
        o, v = c.process(x[:, pos:pos + n])
        out.append(o), vad.append(v.copy())
        pos += n
    want, want_vad = run_triple(d, x, calls, plan)
    assert np.array_equal(_bits(np.concatenate(out, 1)), _bits(want)) and np.array_equal(_bits(np.concatenate(vad)), _bits(want_vad))
    assert np.array_equal(c.export_streams(range(S)), d.export_streams(range(S)))
    assert not np.array_equal(_bits(want), _bits(triple_runs(nn, lib, name, (2, "max"))["out"]))


def check_lifecycle(nn, lib, rows, sink, link=(2, "max"), name="s72"):
    """8. The link is configuration: get returns it unchanged after reset_streams, import_streams, hold + resume, reset and save_state /
    load_state; the state image, the record and device_bytes are an unlinked batch's; clone carries it and the clone continues
    bit-identically; a reset batch under the link starts as D started; a record from a linked batch imports into an unlinked one."""
    x, a = shared_runs(nn, lib, name)
    d = triple_runs(nn, lib, name, link)
    S = x.shape[0]
    mgf, calls = SHAPES[name][3], SHAPES[name][4]
    b = make_batch(nn, lib, S, mgf, rows, sink)
    plain_bytes, plain_state = b.device_bytes(), len(b.save_state())
    assert b.channel_link() == (1, "off")
    b.set_channel_link(*link)
    assert b.device_bytes() == plain_bytes and len(b.save_state()) == plain_state
    o, _ = run_calls(b, x, calls[:2])
    assert np.array_equal(_bits(o), _bits(d["out"][:, :3]))
    rec = b.export_streams([2])
    assert rec.shape == (1, nn.STREAM_STATE_BYTES) and nn.STREAM_STATE_VERSION == 1
    b.reset_streams([1, 6, 69])
    assert b.channel_link() == link
    b.import_streams([3], rec)
    assert b.channel_link() == link
    b.hold_streams([1, 2, 66]), b.resume_streams([1, 2, 66])
    assert b.channel_link() == link
    snap = b.save_state()
    b.reset()
    assert b.channel_link() == link
    fresh, _ = run_calls(b, x, calls[:1])
    assert np.array_equal(_bits(fresh), _bits(d["out"][:, :1]))
    b.load_state(snap)
    assert b.channel_link() == link
    c = b.clone()
    assert c.channel_link() == link
    ob, vb = run_calls(b, x, calls[2:4], start=3)
    oc, vc = run_calls(c, x, calls[2:4], start=3)
    assert np.array_equal(_bits(ob), _bits(oc)) and np.array_equal(_bits(vb), _bits(vc))
    assert np.array_equal(b.export_streams(range(S)), c.export_streams(range(S)))
    u, w = nn.BatchDenoiser(S, lib=lib, max_group_frames=mgf), nn.BatchDenoiser(S, lib=lib, max_group_frames=mgf)
    w.set_channel_link(*link)
    for bd in (u, w):
        bd.import_streams(range(S), b.export_streams(range(S)))
    assert u.channel_link() == (1, "off") and np.array_equal(u.export_streams(range(S)), w.export_streams(range(S)))
    ou, _ = run_calls(u, x, calls[4:5], start=6)
    ow, _ = run_calls(w, x, calls[4:5], start=6)
    ob, _ = run_calls(b, x, calls[4:5], start=6)
    assert np.array_equal(_bits(ow), _bits(ob)) and not np.array_equal(_bits(ou), _bits(ob))


def check_pcm(nn, lib, rows, sink, link=(2, "max")):
    """9a. s72 as packed 2-channel int16 through one process_pcm call with discard_first under (2, max) -- the stereo file's call -- against
    the same layout through the triple's PCM variants (the inputs are integers: both boundaries see A's samples)."""
    from nnnoiseless_amd import _ffi
    x, a = shared_runs(nn, lib, "s72")
    S, T = x.shape[:2]
    pcm = x.astype(np.int16).reshape(S // 2, 2, T * 480).transpose(0, 2, 1).copy()     # [G, T * 480, 2]
    c, d = linked_batch(nn, lib, S, 2, rows, sink, link), nn.BatchDenoiser(S, lib=lib, max_group_frames=2)
    got, vad = c.process_pcm(pcm, _ffi.PCM_I16, channels=2, discard_first=True)
    want, pos = [], 0
    for n in SHAPES["s72"][4]:
        f, sil = d.analyze(pcm[:, pos * 480:(pos + n) * 480], fmt=_ffi.PCM_I16, channels=2)
        g, v = d.network(f, sil)
        want.append(d.synthesize(link_np(g, sil, *link), v, fmt=_ffi.PCM_I16, channels=2, discard_first=True))
        pos += n
    want = np.concatenate(want, 1)
    assert got.shape == (S // 2, (T - 1) * 480, 2) and np.array_equal(got, want)
    assert np.array_equal(_bits(vad), _bits(a["vad"]))
    assert np.array_equal(c.export_streams(range(S)), triple_runs(nn, lib, "s72", link)["records"])


def check_host_chunks(nn, lib, rows, sink, link=(4, "max"), name="s72"):
    """9b. One host-buffer call of all frames under NNN_HOST_CHUNK=1 (a chunk per frame) and in one piece (NNN_HOST_CHUNK=0): D's audio
    and records, A's VAD, both ways."""
    x, a = shared_runs(nn, lib, name)
    d = triple_runs(nn, lib, name, link)
    S = x.shape[0]
    for chunk in ("1", "0"):
        with env("NNN_HOST_CHUNK", chunk):
            b = linked_batch(nn, lib, S, SHAPES[name][3], rows, sink, link)
        out, vad = b.process(x)
        assert np.array_equal(_bits(out), _bits(d["out"])), chunk
        assert np.array_equal(_bits(vad), _bits(a["vad"])) and np.array_equal(b.export_streams(range(S)), d["records"]), chunk


def check_schedules(nn, lib, sink, link=(2, "max")):
    """9c. 4 streams x 40 frames in ONE call (two groups) under NNN_SCHED=seq, lanes and stages: the in-order call's bits are the triple's
    (24 + 16 frames), and the two pipelined schedules give the in-order call's bits."""
    from nnnoiseless_amd.synthetic import make_streams
    S, T = 4, 40
    x = np.clip(np.round(make_streams(43, S, T)), -32768, 32767).astype(np.float32)
    got = {}
    for sched in ("seq", "lanes", "stages"):
        with env("NNN_SCHED", sched), env("NNN_RNN_WF_MIN_G", SINKS[sink][1]):
            b = nn.BatchDenoiser(S, lib=lib)
        b.set_channel_link(*link)
        out, vad = b.process(x)
        got[sched] = (out, vad.copy(), b.export_streams(range(S)))
    d = nn.BatchDenoiser(S, lib=lib)
    want, want_vad = run_triple(d, x, (24, 16), link)
    assert np.array_equal(_bits(got["seq"][0]), _bits(want)) and np.array_equal(_bits(got["seq"][1]), _bits(want_vad))
    assert np.array_equal(got["seq"][2], d.export_streams(range(S)))
    for sched in ("lanes", "stages"):
        for i in range(3):
            assert np.array_equal(_bits(got[sched][i]), _bits(got["seq"][i])), (sched, i)


def check_models(nn, lib, weights_bytes, rows, sink, link=(4, "max")):
    """10. A grouped batch, the built-in model on 64 streams and tests/golden/sh.rnn on 8: its own triple in audio, VAD and records; each
    model group's launch links its own streams."""
    from nnnoiseless_amd.synthetic import make_streams
    sizes = [64, 8]
    models = [None, nn.RnnModel.from_bytes(open(os.path.join(GOLDEN, "sh.rnn"), "rb").read(), lib=lib)]
    S, T = sum(sizes), 3
    x = make_streams(31, S, T)
    mode, wf = SINKS[sink]
    with rnn_rows(rows), env("NNN_RNN_WF_MIN_G", wf):
        c, d, u = (nn.BatchDenoiser(S, lib=lib, groups=list(zip(models, sizes))) for _ in range(3))
    c.set_back_end(mode)
    c.set_channel_link(*link)
    out, vad = c.process(x)
    want, want_vad = run_triple(d, x, (T,), link)
    plain, _ = u.process(x)
    assert np.array_equal(_bits(out), _bits(want)) and np.array_equal(_bits(vad), _bits(want_vad))
    assert np.array_equal(c.export_streams(range(S)), d.export_streams(range(S)))
    for lo, hi in ((0, 64), (64, 72)):
        assert not np.array_equal(_bits(out[lo:hi]), _bits(plain[lo:hi])), (lo, hi)


def check_other_calls(nn, lib, name, rows, sink, link=(2, "min")):
    """11. On a linked batch network returns A's raw, unlinked gains and A's VAD, vad returns A's VAD, analyze returns A's features, and
    synthesize applies the caller's gains as an unlinked batch does."""
    x, a = shared_runs(nn, lib, name)
    S, T = x.shape[:2]
    mgf = SHAPES[name][3]
    n, v, f = (linked_batch(nn, lib, S, mgf, rows, sink, link) for _ in range(3))
    u = make_batch(nn, lib, S, mgf, rows, sink)
    g, vd = n.network(a["features"], a["silence"])
    assert np.array_equal(_bits(g), _bits(a["g_raw"])) and np.array_equal(_bits(vd), _bits(a["vad"]))
    k = v.max_group_frames()
    assert np.array_equal(_bits(v.vad(x[:, :k])), _bits(a["vad"][:k]))
    gains = np.random.default_rng(5).uniform(0.05, 1.0, (k, S, 22)).astype(np.float32)
    feats = [b.analyze(x[:, :k]) for b in (f, u)]
    assert np.array_equal(_bits(feats[0][0]), _bits(a["features"][:k])) and np.array_equal(feats[0][1], feats[1][1])
    of, ou = f.synthesize(gains), u.synthesize(gains)
    assert np.array_equal(_bits(of), _bits(ou)) and np.array_equal(f.export_streams(range(S)), u.export_streams(range(S)))
    assert f.channel_link() == link


def check_refusals(nn, lib, rows, sink):
    """12. Every refusal returns non-zero with its text and changes nothing: get reads as before, and the run continued after the refused
    calls is bit-identical to a twin's without them."""
    x, a = shared_runs(nn, lib, "s4")
    S, link = 4, (2, "max")
    b, twin = (linked_batch(nn, lib, S, None, rows, sink, link) for _ in range(2))
    for bd in (b, twin):
        run_calls(bd, x, (2,))
    L = lib.L

    def refused(rc_of, text):
        with pytest.raises(RuntimeError, match=text):
            lib.check(rc_of())
        assert b.channel_link() == link
    refused(lambda: L.nnn_batch_set_channel_link(None, 2, 1), "null batch")
    for ch in (0, 3, 5, 8, -2):
        refused(lambda: L.nnn_batch_set_channel_link(b._h, ch, 1), "channels")
    for mode in (-1, 3, 7):
        refused(lambda: L.nnn_batch_set_channel_link(b._h, 2, mode), "mode")
    with pytest.raises(ValueError):
        b.set_channel_link(2, "mean")
    six = nn.BatchDenoiser(6, lib=lib)
    with pytest.raises(RuntimeError, match="link group"):
        six.set_channel_link(4, "max")
    assert six.channel_link() == (1, "off")
    six.set_channel_link(2, "min")
    with pytest.raises(RuntimeError, match="link group"):
        six.set_channel_link(4, "min")
    assert six.channel_link() == (2, "min")
    p = nn.BatchDenoiser(S, lib=lib)
    p.analyze(x[:, :1])
    with pytest.raises(RuntimeError, match="pending"):
        p.set_channel_link(2, "max")
    assert p.channel_link() == (1, "off") and p.pending_frames() == 1
    ch, md = C.c_int32(9), C.c_int32(9)
    assert L.nnn_batch_get_channel_link(None, C.byref(ch), C.byref(md)) != 0 and (ch.value, md.value) == (9, 9)
    assert L.nnn_batch_get_channel_link(b._h, None, None) == 0
    ob, vb = run_calls(b, x, (1, 24), start=2)
    ot, vt = run_calls(twin, x, (1, 24), start=2)
    assert np.array_equal(_bits(ob), _bits(ot)) and np.array_equal(_bits(vb), _bits(vt))
    assert np.array_equal(b.export_streams(range(S)), twin.export_streams(range(S)))
    assert np.array_equal(_bits(ob), _bits(triple_runs(nn, lib, "s4", link)["out"][:, 2:]))
    # a set fault refuses (test_hostsim_network.py's recipe: the second frame of the call never sees the first one's hand-off flag)
    lib.check(L.nnn_batch_debug_withhold_flag(b._h, 0))
    with pytest.raises(RuntimeError, match="hand-off"):
        b.process(x[:, :2])
    assert b.fault()
    refused(lambda: L.nnn_batch_set_channel_link(b._h, 4, 2), "hand-off")
    lib.check(L.nnn_batch_debug_withhold_flag(b._h, -1))
    b.reset()
    assert not b.fault() and b.channel_link() == link
    b.set_channel_link(4, "min")
    assert b.channel_link() == (4, "min")


def check_node(nn, lib, devices=(0, 0), link=(4, "max")):
    """13. s72 over a node of two shards (36 + 36 streams: no link group is cut): the single batch's triple in audio, VAD and records; get
    agrees.  Six streams over two shards (3 + 3) cut a 2-channel group at the shard edge: refused, no shard changed."""
    x, a = shared_runs(nn, lib, "s72")
    d = triple_runs(nn, lib, "s72", link)
    S = x.shape[0]
    node = nn.NodeDenoiser(S, devices, lib=lib, max_group_frames=2)
    assert [lo for _, lo, _ in node.shards()] == [0, 36] and node.channel_link() == (1, "off")
    with pytest.raises(RuntimeError, match="channels"):
        node.set_channel_link(3, "max")
    node.set_channel_link(*link)
    assert node.channel_link() == link
    out, vad, pos = [], [], 0
    for n in SHAPES["s72"][4]:
        o, v = node.process(x[:, pos:pos + n])
        out.append(o), vad.append(v.copy())
        pos += n
    assert np.array_equal(_bits(np.concatenate(out, 1)), _bits(d["out"])) and np.array_equal(_bits(np.concatenate(vad)), _bits(a["vad"]))
    assert np.array_equal(node.export_streams(range(S)), d["records"])
    node.close()
    cut = nn.NodeDenoiser(6, devices, lib=lib)
    assert [lo for _, lo, _ in cut.shards()] == [0, 3]
    with pytest.raises(RuntimeError, match="link group"):
        cut.set_channel_link(2, "max")
    assert cut.channel_link() == (1, "off")
    xs = make_input("s4")[:3, :2]
    six = np.concatenate([xs, xs])
    o, _ = cut.process(six)
    assert np.array_equal(_bits(o[:3]), _bits(o[3:]))                                  # (nobody is linked: the two halves run alike)
    cut.close()


# ---- under the interpreter --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nn():
    import nnnoiseless_amd
    return nnnoiseless_amd


SINK_ROWS = [(s, 16) for s in SINKS] + [("plain", 32)]                # (NNN_RNN_ROWS reaches k_rnn alone: see the module's docstring)
# the interpreter takes half a minute per run of s72: every sink and row count there under two of the four links, chosen so that each link
# meets k_rnn at both row counts or three sinks; s4 and the device (test_gpu_channel_link.py) under all four
S72_LINKS = {("fused", 16): [(2, "max"), (4, "min")], ("rnn16", 16): [(2, "min"), (4, "max")], ("wf", 16): [(2, "max"), (4, "min")],
             ("plain", 16): [(2, "min"), (4, "max")], ("plain", 32): [(2, "max"), (4, "min")]}
CASES = [("s4", s, r, l) for s, r in SINK_ROWS for l in LINKS] + [("s72", s, r, l) for s, r in SINK_ROWS for l in S72_LINKS[(s, r)]]


@pytest.mark.parametrize("name,sink,rows,link", CASES)
def test_linked_call_is_the_linked_triple(nn, hostsim_lib, name, sink, rows, link):
    check_equals_triple(nn, hostsim_lib, name, rows, sink, link)


@pytest.mark.parametrize("sink,rows,link", [("fused", 16, (2, "max")), ("rnn16", 16, (4, "min")), ("wf", 16, (4, "max")), ("plain", 32, (2, "min"))])
def test_silent_member(nn, hostsim_lib, sink, rows, link):
    check_silent_member(nn, hostsim_lib, rows, sink, link)


@pytest.mark.parametrize("sink,rows,link", [("fused", 16, (4, "max")), ("rnn16", 16, (2, "max")), ("wf", 16, (2, "min")), ("plain", 32, (4, "min")),
                                            ("plain", 16, (4, "max"))])
def test_held_member(nn, hostsim_lib, sink, rows, link):
    check_held(nn, hostsim_lib, rows, sink, link)


@pytest.mark.parametrize("name,sink,rows,link", [("s72", "fused", 16, (2, "max")), ("s72", "plain", 32, (4, "min")), ("s4", "rnn16", 16, (4, "max")),
                                                 ("s4", "wf", 16, (2, "min"))])
def test_link_then_floor(nn, hostsim_lib, name, sink, rows, link):
    check_floors(nn, hostsim_lib, name, rows, sink, link)


@pytest.mark.parametrize("sink", list(SINKS))
def test_off_is_off(nn, hostsim_lib, sink):
    check_off_is_off(nn, hostsim_lib, "s72" if sink in ("fused", "plain") else "s4", 32, sink)


@pytest.mark.parametrize("name,sink", [("s72", "wf"), ("s72", "rnn16"), ("s4", "fused"), ("s4", "plain")])
def test_changing_the_link_between_calls(nn, hostsim_lib, name, sink):
    check_change_between_calls(nn, hostsim_lib, name, 32 if sink == "plain" else 16, sink)


@pytest.mark.parametrize("sink", ["fused", "wf"])
def test_lifecycle(nn, hostsim_lib, sink):
    check_lifecycle(nn, hostsim_lib, 32, sink)


@pytest.mark.parametrize("name", list(SHAPES))
def test_other_calls_ignore_the_link(nn, hostsim_lib, name):
    check_other_calls(nn, hostsim_lib, name, 16, "fused")


@pytest.mark.parametrize("sink", ["fused", "wf"])
def test_pcm_boundary(nn, hostsim_lib, sink):
    check_pcm(nn, hostsim_lib, 32, sink)


@pytest.mark.parametrize("sink", ["rnn16", "plain"])
def test_host_chunks(nn, hostsim_lib, sink):
    check_host_chunks(nn, hostsim_lib, 16, sink)


@pytest.mark.parametrize("sink", ["wf", "plain"])
def test_schedules(nn, hostsim_lib, sink):
    check_schedules(nn, hostsim_lib, sink)


@pytest.mark.parametrize("sink", ["wf", "plain"])      # (a model outside k_back's shape class sends every group of the batch through three launches)
def test_grouped_models(nn, hostsim_lib, weights_bytes, sink):
    check_models(nn, hostsim_lib, weights_bytes, 16 if sink == "plain" else 32, sink)


def test_refusals(nn, hostsim_lib):
    check_refusals(nn, hostsim_lib, 32, "fused")


def test_node(nn, hostsim_lib, monkeypatch):
    monkeypatch.setenv("NNN_NODE_THREADS", "0")          # (the interpreter runs kernels on the calling thread and is not re-entrant)
    check_node(nn, hostsim_lib)
