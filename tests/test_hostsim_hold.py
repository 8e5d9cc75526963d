"""Hold and resume (include/nnn_batch.h nnn_batch_hold_streams / nnn_batch_resume_streams) under the test-only SIMT interpreter: held
streams sit out calls, keep their state, leave the caller's buffers alone and continue bit for bit; the live streams never notice.
Same base as test_hostsim_stream_state.py: 70 streams (a full tile and a partial one), max_group_frames=2 -- an 8-slot ring that wraps
while streams are held."""
import numpy as np
import pytest

from conftest import assert_flips_in_line, flip_stats

S70, DONE = 70, 11
IDX = [0, 33, 64, 69]
HELD_CALLS = ((0, 1), (1, 4), (4, 5))    # the five frames the streams are held for: calls of 1, 3 and 1 frames
SENT = np.float32(-12345.0)               # what the caller's buffers hold where a held stream would write
SENT_BITS = np.float32(SENT).view(np.uint32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _run_into(bd, x, calls):
    """x [S, T, 480] through bd in calls of the given (lo, hi) ranges, into buffers pre-filled with the sentinel: (out, vad [T, S])."""
    S, T = x.shape[0], x.shape[1]
    out, vad = np.full((S, T, 480), SENT, np.float32), np.full((T, S), SENT, np.float32)
    for lo, hi in calls:
        o, v = np.full((S, hi - lo, 480), SENT, np.float32), np.full((hi - lo, S), SENT, np.float32)
        bd.process(x[:, lo:hi], out=o, vad=v)
        out[:, lo:hi], vad[lo:hi] = o, v
    return out, vad


@pytest.fixture(scope="module")
def x70():
    from nnnoiseless_amd.synthetic import make_streams
    return make_streams(41, S70, 20)


_SNAP = {}   # max_group_frames -> snapshot of a batch with DONE frames behind it


def _batch(lib, x, mgf=2, back_end=None):
    """A batch with DONE frames behind it (calls of 4, 1 and 6 frames; later ones load the first one's snapshot)."""
    import nnnoiseless_amd as nn
    bd = nn.BatchDenoiser(S70, lib=lib, max_group_frames=mgf)
    if mgf in _SNAP:
        bd.load_state(_SNAP[mgf])
    else:
        for lo, hi in ((0, 4), (4, 5), (5, DONE)):
            bd.process(x[:, lo:hi])
        _SNAP[mgf] = bd.save_state()
    if back_end is not None:
        bd.set_back_end(back_end)
    return bd


def _hold_resume_against_twins(make, x, idx, after=((0, 4),), w_cache=None):
    """Batch A holds `idx` for five frames (NaN in their input, sentinels in the buffers), resumes and runs four more.  Twin B held nothing
    and is fed, for `idx`, only the frames they were live for; twin W held nothing and saw every frame.  Returns A's outputs of the
    last four frames for the oracle test."""
    a, b = make(), make()
    rest = [s for s in range(x.shape[0]) if s not in idx]
    a.hold_streams(idx)
    assert a.num_held() == len(idx) and a.held().nonzero()[0].tolist() == sorted(idx)
    xa = x[:, DONE:DONE + 5].copy()
    xa[idx] = np.nan
    o1, v1 = _run_into(a, xa, HELD_CALLS)
    assert (_bits(o1[idx]) == SENT_BITS).all() and (_bits(v1[:, idx]) == SENT_BITS).all()      # nothing of a held stream was written
    a.resume_streams(idx)
    assert a.num_held() == 0
    o2, v2 = _run_into(a, x[:, DONE + 5:DONE + 9], after)
    w_cache = {} if w_cache is None else w_cache
    if "w" not in w_cache:
        w_cache["w"] = make().process(x[:, DONE:DONE + 9])
    wo, wv = w_cache["w"]
    assert np.array_equal(_bits(o1[rest]), _bits(wo[rest, :5])) and np.array_equal(_bits(v1[:, rest]), _bits(wv[:5][:, rest]))
    assert np.array_equal(_bits(o2[rest]), _bits(wo[rest, 5:])) and np.array_equal(_bits(v2[:, rest]), _bits(wv[5:][:, rest]))
    xb = x[:, DONE:DONE + 4].copy()
    xb[idx] = x[idx, DONE + 5:DONE + 9]
    bo, bv = b.process(xb)
    assert np.array_equal(_bits(o2[idx]), _bits(bo[idx])) and np.array_equal(_bits(v2[:, idx]), _bits(bv[:, idx]))
    assert not a.fault()
    return o2, v2


def test_held_streams_continue_bit_for_bit(hostsim_lib, x70):
    _hold_resume_against_twins(lambda: _batch(hostsim_lib, x70), x70, IDX, after=((0, 1), (1, 4)))


@pytest.mark.parametrize("mgf, chain, hp_split, back_end", [(2, "2", "1", None), (2, "0", "0", 2), (1, None, "1", 1), (1, None, "0", 0)])
def test_whole_tiles_and_blocks_held(hostsim_lib, x70, monkeypatch, mgf, chain, hp_split, back_end):
    """A whole tile, a whole 16-stream block, a whole 4-stream block: the early returns of every kernel, in groups (chained and looped
    k_pitch, fused and unfused back end, k_hp and k_hp2) and in one-frame calls (the riders of the tick)."""
    if chain is not None:
        monkeypatch.setenv("NNN_PITCH_CHAIN", chain)
    monkeypatch.setenv("NNN_HP_SPLIT", hp_split)
    make = lambda: _batch(hostsim_lib, x70, mgf=mgf, back_end=back_end)
    w_cache = {}                                                                   # (the twin that holds nothing: once per configuration)
    for idx in (list(range(64)), list(range(16, 32)), list(range(4, 8))):
        _hold_resume_against_twins(make, x70, idx, w_cache=w_cache)


def test_hold_before_the_first_frame(hostsim_lib, x70):
    import nnnoiseless_amd as nn
    a = nn.BatchDenoiser(S70, lib=hostsim_lib, max_group_frames=2)
    a.hold_streams(IDX)
    _run_into(a, x70[:, :7], ((0, 3), (3, 7)))
    a.resume_streams(IDX)
    out, vad = a.process(x70[:, 7:12])
    fresh = nn.BatchDenoiser(len(IDX), lib=hostsim_lib)
    f_out, f_vad = fresh.process(x70[IDX, 7:12])
    assert np.array_equal(_bits(out[IDX]), _bits(f_out)) and np.array_equal(_bits(vad[:, IDX]), _bits(f_vad))


def test_other_calls_on_held_streams(hostsim_lib, x70):
    """The table of include/nnn_batch.h: export, import, reset, clone, save / load, nnn_batch_reset and all-held calls."""
    import nnnoiseless_amd as nn
    make = lambda: _batch(hostsim_lib, x70)
    a = make()
    everything = list(range(S70))
    before = a.export_streams(everything)
    a.hold_streams(IDX)
    _run_into(a, x70[:, DONE:DONE + 3], ((0, 3),))
    assert np.array_equal(a.export_streams(IDX), before[IDX])                      # the parked record: as exported just before the hold
    assert np.array_equal(a.export_streams([1, 64, 2, 0])[[1, 3]], before[[64, 0]])   # ... in a list that mixes held and live streams
    # refusals change nothing
    snapshot = a.export_streams(everything)
    L = a._lib.L
    for call in (lambda: a.hold_streams([0]), lambda: a.hold_streams([1, 33]), lambda: a.resume_streams([1]), lambda: a.resume_streams([0, 1]),
                 lambda: a.hold_streams([S70]), lambda: a.hold_streams([-1]), lambda: a.resume_streams([64, 64]), lambda: a.hold_streams([5, 5]),
                 lambda: a._lib.check(L.nnn_batch_hold_streams(a._h, None, 2)), lambda: a._lib.check(L.nnn_batch_resume_streams(a._h, None, 1)),
                 lambda: a.save_state(), lambda: a.load_state(make().save_state())):
        with pytest.raises(RuntimeError, match="nnnoiseless_amd"):
            call()
    assert np.array_equal(a.export_streams(everything), snapshot) and a.held().nonzero()[0].tolist() == IDX
    with pytest.raises(RuntimeError, match="held"):
        a.save_state()
    # clone carries the holds and the parked records
    c = a.clone()
    assert c.held().nonzero()[0].tolist() == IDX and np.array_equal(c.export_streams(everything), snapshot)
    # import / reset into held streams, then resume == import / reset into live ones
    donor = nn.BatchDenoiser(2, lib=hostsim_lib)
    donor.process(x70[:2, :6])
    rec = donor.export_streams([0, 1])
    a.import_streams([33, 64], rec)
    a.reset_streams([69])
    assert a.num_held() == 4                                                       # (they stay held)
    _run_into(a, x70[:, DONE + 3:DONE + 4], ((0, 1),))
    a.resume_streams(IDX)
    ref = make()
    ref.process(x70[:, DONE:DONE + 4])
    ref.import_streams([33, 64], rec)
    ref.reset_streams([69])
    got, gv = a.process(x70[:, 14:17])
    want, wv = ref.process(x70[:, 14:17])
    live = [s for s in range(S70) if s != 0]
    assert np.array_equal(_bits(got[live]), _bits(want[live])) and np.array_equal(_bits(gv[:, live]), _bits(wv[:, live]))
    # ... and the clone, resumed, carries on like a batch that never ran the held frames for those streams
    c.resume_streams(IDX)
    twin = make()
    xt = x70[:, DONE:DONE + 3].copy()
    twin.process(xt)                                                               # the live streams' three frames
    twin.import_streams(IDX, before[IDX])                                          # the held ones: back to where they were parked
    c_out, _ = c.process(x70[:, 16:18])
    t_out, _ = twin.process(x70[:, 16:18])
    assert np.array_equal(_bits(c_out), _bits(t_out))
    # every stream held: calls succeed, launch nothing, and the frame counter moves (the ring phase of the resume follows it)
    d, b = make(), make()
    d.hold_streams(everything)
    o, v = _run_into(d, np.full((S70, 3, 480), np.nan, np.float32), ((0, 1), (1, 3)))
    assert (_bits(o) == SENT_BITS).all() and (_bits(v) == SENT_BITS).all()
    d.resume_streams(everything)
    d_out, d_vad = d.process(x70[:, DONE:DONE + 3])
    b_out, b_vad = b.process(x70[:, DONE:DONE + 3])
    assert np.array_equal(_bits(d_out), _bits(b_out)) and np.array_equal(_bits(d_vad), _bits(b_vad))
    # nnn_batch_reset releases every hold
    d.hold_streams([1, 2])
    d.reset()
    assert d.num_held() == 0 and not d.held().any()
    r_out, _ = d.process(x70[:, :2])
    f_out, _ = nn.BatchDenoiser(S70, lib=hostsim_lib, max_group_frames=2).process(x70[:, :2])
    assert np.array_equal(_bits(r_out), _bits(f_out))


def test_pcm_one_channel_of_a_group_held(hostsim_lib):
    """Two interleaved int16 channels: the held channel's samples inside frames the other channel writes keep what the caller had there."""
    import nnnoiseless_amd as nn
    from nnnoiseless_amd import _ffi
    from nnnoiseless_amd.synthetic import make_streams
    G, T = 3, 5
    x = make_streams(9, 2 * G, T)                                                  # stream 2 g + c = channel c of group g
    pcm = np.clip(x, -32768, 32767).astype(np.int16).reshape(G, 2, T * 480).transpose(0, 2, 1).copy()   # [G, T * 480, 2]
    a = nn.BatchDenoiser(2 * G, lib=hostsim_lib, max_group_frames=2)
    w = nn.BatchDenoiser(2 * G, lib=hostsim_lib, max_group_frames=2)
    a.process_pcm(pcm[:, :2 * 480], _ffi.PCM_I16, channels=2)
    w.process_pcm(pcm[:, :2 * 480], _ffi.PCM_I16, channels=2)
    a.hold_streams([1, 4])                                                         # channel 1 of group 0, channel 0 of group 2
    out = np.full((G, 3 * 480, 2), -321, np.int16)
    vad = np.full((3, 2 * G), SENT, np.float32)
    a.process_pcm(pcm[:, 2 * 480:], _ffi.PCM_I16, channels=2, out=out, vad=vad)
    w_out, w_vad = w.process_pcm(pcm[:, 2 * 480:], _ffi.PCM_I16, channels=2)
    assert (out[0, :, 1] == -321).all() and (out[2, :, 0] == -321).all() and (_bits(vad[:, [1, 4]]) == SENT_BITS).all()
    for g, c in ((0, 0), (1, 0), (1, 1), (2, 1)):
        assert np.array_equal(out[g, :, c], w_out[g, :, c]) and np.array_equal(_bits(vad[:, 2 * g + c]), _bits(w_vad[:, 2 * g + c]))


def test_node_holds_across_shards(hostsim_lib, monkeypatch):
    import nnnoiseless_amd as nn
    from nnnoiseless_amd.synthetic import make_streams
    monkeypatch.setenv("NNN_NODE_THREADS", "0")
    S = 9
    x = make_streams(30, S, 9)
    node = nn.NodeDenoiser(S, (0, 0, 0), lib=hostsim_lib)                         # shards [0, 3) [3, 6) [6, 9)
    one = nn.BatchDenoiser(S, lib=hostsim_lib)
    node.process(x[:, :3])
    one.process(x[:, :3])
    idx = [2, 3, 5, 6]
    node.hold_streams(idx)
    one.hold_streams(idx)
    assert node.num_held() == 4
    with pytest.raises(RuntimeError):
        node.hold_streams([0, 5])                                                  # (refused as a whole: stream 0 stays live)
    with pytest.raises(RuntimeError):
        node.resume_streams([2, 4])
    assert node.num_held() == 4
    xa = x[:, 3:6].copy()
    xa[idx] = np.nan
    n_out, n_vad = np.full((S, 3, 480), SENT, np.float32), np.full((3, S), SENT, np.float32)
    o_out, o_vad = n_out.copy(), n_vad.copy()
    node.process(xa, out=n_out, vad=n_vad)
    one.process(xa, out=o_out, vad=o_vad)
    assert np.array_equal(_bits(n_out), _bits(o_out)) and np.array_equal(_bits(n_vad), _bits(o_vad))
    assert (_bits(n_out[idx]) == SENT_BITS).all() and (_bits(n_vad[:, idx]) == SENT_BITS).all()
    node.resume_streams(idx)
    one.resume_streams(idx)
    n2, nv2 = node.process(x[:, 6:9])
    o2, ov2 = one.process(x[:, 6:9])
    assert np.array_equal(_bits(n2), _bits(o2)) and np.array_equal(_bits(nv2), _bits(ov2)) and node.num_held() == 0


def test_held_and_resumed_streams_against_the_oracle(hostsim_lib, oracle_mod, weights_bytes, x70):
    """The streams of the first test on the frames they are live for, against the CPU oracle run on those frames alone: the pitch index
    exactly (through the frame log), audio and VAD at the bars of the parity tests.  Inputs make_streams(41, 70, 20), as
    test_hostsim_stream_state.py uses; the oracle's own two builds (f64 and f32 transforms) are checked first for branch flips on these
    streams and frames."""
    import nnnoiseless_amd as nn
    live = list(range(DONE)) + list(range(DONE + 5, DONE + 9))                     # frames 0 .. 10 and 16 .. 19
    xs = x70[IDX][:, live]
    ref = oracle_mod.run_streams(oracle_mod.Model(weights_bytes), xs, want=("out", "pitch", "branch", "vad"))
    ref32 = oracle_mod.run_streams(oracle_mod.Model(weights_bytes, f32_fft=True), xs, want=("out", "branch"))
    assert np.array_equal(ref["branch"], ref32["branch"]), "the oracle's two builds flip a branch on these inputs: pick another seed"
    bd = nn.BatchDenoiser(S70, lib=hostsim_lib, max_group_frames=2)
    T = DONE + 9
    log = np.zeros((T, S70, 24), np.uint32)
    bd.set_frame_log(log.ctypes.data, T)
    outs, vads = [], []
    for lo, hi in ((0, 4), (4, 5), (5, DONE)):
        o, v = bd.process(x70[:, lo:hi])
        outs.append(o[IDX]); vads.append(v[:, IDX])
    bd.hold_streams(IDX)
    xa = x70[:, DONE:DONE + 5].copy()
    xa[IDX] = np.nan
    _run_into(bd, xa, HELD_CALLS)
    bd.resume_streams(IDX)
    for lo, hi in ((16, 17), (17, 20)):
        o, v = bd.process(x70[:, lo:hi])
        outs.append(o[IDX]); vads.append(v[:, IDX])
    out, vad = np.concatenate(outs, 1), np.concatenate(vads, 0)
    lg = log[live][:, IDX].astype(np.int32)                                        # [15, 4, 24]: the held frames' rows are unspecified
    assert np.array_equal(lg[:, :, 0].T, ref["pitch"])
    branch = lg[:, :, 1].T
    st = flip_stats(branch, out, ref, ref32)
    assert_flips_in_line(st, "held and resumed streams")
    flip = branch != ref["branch"]
    excused = flip.copy()
    excused[:, 1:] |= flip[:, :-1]
    ok = ~excused[:, 1:]
    d = (out[:, 1:] - ref["out"][:, 1:]).astype(np.float64)
    rr = ref["out"][:, 1:].astype(np.float64)
    assert np.sqrt((d[ok] ** 2).sum() / (rr[ok] ** 2).sum()) <= 1e-4
    assert np.abs(vad.T - ref["vad"]).max() <= 1e-4


def test_device_record_calls_on_held_streams(hostsim_lib, x70):
    """export_streams_device / import_streams_device meet a held stream as the host variants do: the parked record out, a record in
    (the stream stays held), in lists that mix held and live streams.  (Under the interpreter device memory is host memory.)"""
    import nnnoiseless_amd as nn
    a, ref = _batch(hostsim_lib, x70), _batch(hostsim_lib, x70)
    before = a.export_streams(range(S70))
    a.hold_streams(IDX)
    _run_into(a, x70[:, DONE:DONE + 2], ((0, 2),))
    ref.process(x70[:, DONE:DONE + 2])
    lst = [64, 5, 0, 40]                                                           # held, live, held, live
    d_rec = np.zeros((len(lst), nn.STREAM_STATE_BYTES), np.uint8)
    a.export_streams_device(lst, d_rec.ctypes.data)
    a.synchronize()
    assert np.array_equal(d_rec[[0, 2]], before[[64, 0]]) and np.array_equal(d_rec[[1, 3]], ref.export_streams([5, 40]))
    # records in: stream 64 (held) takes stream 5's, stream 40 (live) takes stream 0's parked one
    swap = np.ascontiguousarray(d_rec[[1, 2]])
    a.import_streams_device([64, 40], swap.ctypes.data)
    a.synchronize()
    ref.import_streams([64, 40], swap)
    assert a.num_held() == len(IDX) and np.array_equal(a.export_streams([64]), swap[:1])
    a.resume_streams([64])
    got, gv = a.process(x70[:, 13:15])
    want, wv = ref.process(x70[:, 13:15])
    for s in (64, 40, 5):
        assert np.array_equal(_bits(got[s]), _bits(want[s])) and np.array_equal(_bits(gv[:, s]), _bits(wv[:, s]))
    # a bad record in a device list that names a held stream: dropped whole, the parked record stays
    bad = swap.copy()
    bad[0, 12] ^= 1                                                                # GRU sizes of another model
    a.import_streams_device([0, 5], bad.ctypes.data)
    with pytest.raises(RuntimeError, match="did not match"):
        a.synchronize()
    assert np.array_equal(a.export_streams([0]), before[[0]])


def test_hold_refused_on_a_faulted_batch_resume_allowed(hostsim_lib):
    import nnnoiseless_amd as nn
    from nnnoiseless_amd.synthetic import make_streams
    a = nn.BatchDenoiser(5, lib=hostsim_lib)
    a.hold_streams([3])
    hostsim_lib.check(hostsim_lib.L.nnn_batch_debug_withhold_flag(a._h, 2))       # (the recipe of test_hostsim_stream_state)
    with pytest.raises(RuntimeError, match="hand-off"):
        a.process(make_streams(0, 5, 6))
    assert a.fault()
    with pytest.raises(RuntimeError, match="faulted"):
        a.hold_streams([1])
    assert a.held().nonzero()[0].tolist() == [3]
    a.resume_streams([3])                                                          # (like import: allowed, the fault stays)
    assert a.num_held() == 0 and a.fault()


def test_empty_hold_allocates_up_front(hostsim_lib):
    import nnnoiseless_amd as nn
    a = nn.BatchDenoiser(5, lib=hostsim_lib, max_group_frames=1)
    L = a._lib.L
    L.nnn_batch_device_bytes.restype = __import__("ctypes").c_size_t
    b0 = L.nnn_batch_device_bytes(a._h)
    a.hold_streams([])
    b1 = L.nnn_batch_device_bytes(a._h)
    assert b1 >= b0 + 5 * nn.STREAM_STATE_BYTES and a.num_held() == 0
    a.hold_streams([2])
    assert L.nnn_batch_device_bytes(a._h) == b1
