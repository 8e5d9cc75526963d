"""Per-stream state records (include/nnn_batch.h NNN_STREAM_STATE_*) under the test-only SIMT interpreter: reset, export and import of
single streams, across batches of other sizes, ring phases and group lengths, and what the record holds against the oracle."""
import numpy as np
import pytest

SPLIT = ((0, 1), (1, 4), (4, 9))   # calls of 1, 3 and 5 frames


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _run(bd, x, split=None):
    """x [S, T, 480] through bd in calls of the given (lo, hi) frame ranges; (out, vad [T, S])."""
    split = split or ((0, x.shape[1]),)
    parts = [bd.process(x[:, lo:hi]) for lo, hi in split]
    return np.concatenate([o for o, _ in parts], 1), np.concatenate([v for _, v in parts], 0)


@pytest.fixture(scope="module")
def base70(hostsim_lib):
    """70 streams (one full tile, one partial), max_group_frames=2 (an 8-slot ring that wraps), 11 frames done: its snapshot."""
    import nnnoiseless_amd as nn
    from nnnoiseless_amd.synthetic import make_streams
    x = make_streams(41, 70, 20)
    bd = nn.BatchDenoiser(70, lib=hostsim_lib, max_group_frames=2)
    _run(bd, x[:, :11], ((0, 4), (4, 5), (5, 11)))
    return x, bd.save_state()


def _batch70(hostsim_lib, snap):
    import nnnoiseless_amd as nn
    bd = nn.BatchDenoiser(70, lib=hostsim_lib, max_group_frames=2)
    bd.load_state(snap)
    return bd


def test_reset_streams(hostsim_lib, base70):
    import nnnoiseless_amd as nn
    x, snap = base70
    idx = [0, 33, 64, 69]
    a = _batch70(hostsim_lib, snap)
    a.reset_streams(idx)
    out, vad = _run(a, x[:, 11:20], SPLIT)
    fresh = nn.BatchDenoiser(4, lib=hostsim_lib)
    f_out, f_vad = fresh.process(x[idx, 11:20])
    assert np.array_equal(_bits(out[idx]), _bits(f_out)) and np.array_equal(_bits(vad[:, idx]), _bits(f_vad))
    b = _batch70(hostsim_lib, snap)
    w_out, w_vad = _run(b, x[:, 11:20], SPLIT)
    rest = [s for s in range(70) if s not in idx]
    assert np.array_equal(_bits(out[rest]), _bits(w_out[rest])) and np.array_equal(_bits(vad[:, rest]), _bits(w_vad[:, rest]))


def test_migration_between_batches_of_other_shape_and_phase(hostsim_lib, base70):
    import nnnoiseless_amd as nn
    from nnnoiseless_amd.synthetic import make_streams
    x, snap = base70
    a = _batch70(hostsim_lib, snap)
    _run(a, x[:, 11:13])                                          # 13 frames done
    src = [5, 64, 2, 40, 69]
    rec = a.export_streams(src)
    assert rec.shape == (5, nn.STREAM_STATE_BYTES) and rec.dtype == np.uint8
    b = nn.BatchDenoiser(130, lib=hostsim_lib, max_group_frames=3)
    b.process(make_streams(7, 130, 4))                            # 4 frames done: another ring phase, another ring length
    dst = [129, 0, 77, 63, 64]
    b.import_streams(dst, rec)
    y = make_streams(8, 130, 10)
    xa = np.zeros((70, 10, 480), np.float32)
    xa[src] = y[dst]
    a_out, a_vad = _run(a, xa, SPLIT + ((9, 10),))
    b_out, b_vad = _run(b, y, ((0, 3), (3, 10)))
    assert np.array_equal(_bits(a_out[src]), _bits(b_out[dst])) and np.array_equal(_bits(a_vad[:, src]), _bits(b_vad[:, dst]))
    # the same record through a lone DenoiseState and back out of it
    st = nn.DenoiseState.from_state(rec[1], lib=hostsim_lib)
    o = np.zeros(480, np.float32)
    for t in range(4):
        v = st.process_frame(o, y[dst[1], t])
        assert np.array_equal(_bits(o), _bits(a_out[src[1], t])) and np.float32(v).view(np.uint32) == _bits(a_vad[t, src[1]])
    c = nn.BatchDenoiser(3, lib=hostsim_lib, max_group_frames=1)
    c.import_streams([2], st.export_state()[None])
    c_out, _ = c.process(np.stack([y[0, 4:10], y[0, 4:10], y[dst[1], 4:10]]))
    assert np.array_equal(_bits(c_out[2]), _bits(a_out[src[1], 4:10]))


def test_round_trips(hostsim_lib):
    import nnnoiseless_amd as nn
    from nnnoiseless_amd.synthetic import make_streams
    x = make_streams(3, 6, 9)
    a = nn.BatchDenoiser(6, lib=hostsim_lib, max_group_frames=2)
    a.process(x[:, :5])
    ref = a.clone()
    idx = [4, 1, 2]
    r1 = a.export_streams(idx)
    a.import_streams(idx, r1)
    assert np.array_equal(a.export_streams(idx), r1)              # export, import, export: the same bytes
    got, gv = a.process(x[:, 5:9])
    want, wv = ref.process(x[:, 5:9])
    assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(_bits(gv), _bits(wv))
    # the zero record (what a fresh state exports) is reset
    zero = nn.BatchDenoiser(1, lib=hostsim_lib).export_streams([0])
    assert not zero[0, 64:].any() and nn.stream_state_field(zero[0], "gru_sizes").tolist() == [24, 48, 96]
    a.import_streams([0, 5], np.concatenate([zero, zero]))
    ref.reset_streams([5, 0])
    assert np.array_equal(a.export_streams(range(6)), ref.export_streams(range(6)))
    got, _ = a.process(x[:, :2])
    want, _ = ref.process(x[:, :2])
    assert np.array_equal(_bits(got), _bits(want))


def test_models_of_other_widths_side_by_side(hostsim_lib):
    """A batch of two resident models (GRU rows of each model's own width in tiles sized for the widest): records carry each stream's
    own sizes and move to batches of that model."""
    import nnnoiseless_amd as nn
    from model_fixtures import make_model
    from nnnoiseless_amd.synthetic import make_streams
    small = nn.RnnModel.from_bytes(make_model(seed=4), lib=hostsim_lib)
    x = make_streams(14, 67, 5)
    g = nn.BatchDenoiser(67, lib=hostsim_lib, groups=[(None, 64), (small, 3)])
    g.process(x[:, :3])
    rec = g.export_streams([65, 10])
    assert nn.stream_state_field(rec, "gru_sizes").tolist() == [[20, 40, 72], [24, 48, 96]]
    with pytest.raises(RuntimeError, match="GRU sizes"):
        g.import_streams([10, 65], rec)
    h_small = nn.BatchDenoiser(2, model=small, lib=hostsim_lib)
    h_small.import_streams([1], rec[:1])
    h_def = nn.BatchDenoiser(1, lib=hostsim_lib)
    h_def.import_streams([0], rec[1:])
    want, _ = g.process(x[:, 3:5])
    got_s, _ = h_small.process(x[[0, 65], 3:5])
    got_d, _ = h_def.process(x[[10], 3:5])
    assert np.array_equal(_bits(got_s[1]), _bits(want[65])) and np.array_equal(_bits(got_d[0]), _bits(want[10]))


def test_record_means_what_the_header_says(hostsim_lib, oracle_mod, weights_bytes):
    import nnnoiseless_amd as nn
    from nnnoiseless_amd.synthetic import make_streams
    S, T = 3, 7
    x = make_streams(12, S, T)
    x[1, :2] = 0.0                                                # silent frames: mem_id and lastg stand still
    om = oracle_mod.Model(weights_bytes)
    bd = nn.BatchDenoiser(S, lib=hostsim_lib, max_group_frames=1)
    bd.process(x)
    rec = bd.export_streams(range(S))
    f = lambda name: nn.stream_state_field(rec, name)
    assert (f("magic") == nn._ffi.STREAM_STATE_MAGIC).all() and (f("version") == 1).all() and (f("size") == nn.STREAM_STATE_BYTES).all()
    for s in range(S):
        st = oracle_mod.State(om)
        filtered, non_silent, lastg = [], 0, np.zeros(22)
        for t in range(T):
            st.process_frame(x[s, t])
            tp = st.taps()
            filtered.append(tp["filtered"].astype(np.float32))
            if not tp["silence"]:
                non_silent += 1
                lastg = tp["g"]
        hist = np.concatenate(filtered)[-1728:]
        assert np.array_equal(_bits(f("input_mem")[s]), _bits(hist))
        assert f("last_period")[s, 0] == tp["pitch_idx"]
        assert f("mem_id")[s, 0] == non_silent % 8
        assert np.abs(f("lastg")[s] - lastg).max() <= 2e-5 * max(np.abs(lastg).max(), 1.0)


def test_refusals_leave_the_batch_untouched(hostsim_lib):
    import nnnoiseless_amd as nn
    from nnnoiseless_amd import _ffi
    from nnnoiseless_amd.synthetic import make_streams
    x = make_streams(5, 5, 4)
    a = nn.BatchDenoiser(5, lib=hostsim_lib, max_group_frames=2)
    a.process(x[:, :2])
    ref = a.clone()
    good = a.export_streams([0, 1])
    from model_fixtures import make_model
    other = nn.BatchDenoiser(1, model=nn.RnnModel.from_bytes(make_model(), lib=hostsim_lib), lib=hostsim_lib).export_streams([0])
    cases = []
    for bad in ([0, 5], [-1], [0, 64]):                           # out of range, padding streams included
        cases += [lambda i=bad: a.reset_streams(i), lambda i=bad: a.export_streams(i), lambda i=bad: a.import_streams(i, np.zeros((len(i), nn.STREAM_STATE_BYTES), np.uint8))]
    cases += [lambda: a.reset_streams([1, 1]), lambda: a.import_streams([2, 2], good)]   # duplicates
    for field, value in (("magic", 0), ("version", 2), ("size", 11200), ("gru_sizes", 25)):
        r = good.copy()
        nn.stream_state_field(r, field)   # (layout check)
        off = _ffi.STREAM_STATE_FIELDS[field][0]
        r[1, off:off + 4] = np.array([value], np.uint32).view(np.uint8)
        cases.append(lambda r=r: a.import_streams([3, 4], r))
    cases.append(lambda: a.import_streams([3, 4], np.concatenate([good[:1], other])))   # another model's GRU sizes
    L = a._lib.L
    idx, p = _ffi.stream_list([0, 1])
    buf = np.zeros((2, nn.STREAM_STATE_BYTES), np.uint8)
    cases += [lambda: a._lib.check(L.nnn_batch_export_streams(a._h, p, 2, _ffi.ptr(buf), buf.nbytes - 1)),     # short buffers
              lambda: a._lib.check(L.nnn_batch_import_streams(a._h, p, 2, _ffi.ptr(good), good.nbytes - 16)),
              lambda: a._lib.check(L.nnn_batch_export_streams(a._h, p, 2, None, buf.nbytes)),                  # null pointers
              lambda: a._lib.check(L.nnn_batch_import_streams(a._h, None, 2, _ffi.ptr(good), good.nbytes)),
              lambda: a._lib.check(L.nnn_batch_export_streams_device(a._h, p, 2, None, None))]
    for call in cases:
        with pytest.raises((RuntimeError, ValueError)):
            call()
    got, _ = a.process(x[:, 2:4])
    want, _ = ref.process(x[:, 2:4])
    assert np.array_equal(_bits(got), _bits(want))


def test_export_refused_from_a_faulted_batch_import_keeps_the_fault(hostsim_lib):
    import nnnoiseless_amd as nn
    from nnnoiseless_amd.synthetic import make_streams
    a = nn.BatchDenoiser(5, lib=hostsim_lib)
    rec = a.export_streams([0])
    hostsim_lib.check(hostsim_lib.L.nnn_batch_debug_withhold_flag(a._h, 2))     # (the recipe of test_hostsim_round3)
    with pytest.raises(RuntimeError, match="hand-off"):
        a.process(make_streams(0, 5, 6))
    assert a.fault()
    with pytest.raises(RuntimeError, match="faulted"):
        a.export_streams([0])
    a.import_streams([1], rec)
    a.reset_streams([0])
    assert a.fault()


def test_node_streams_across_shards(hostsim_lib, monkeypatch):
    import nnnoiseless_amd as nn
    from nnnoiseless_amd.synthetic import make_streams
    monkeypatch.setenv("NNN_NODE_THREADS", "0")
    S = 9
    x = make_streams(30, S, 8)
    n3 = nn.NodeDenoiser(S, (0, 0, 0), lib=hostsim_lib)          # shards [0, 3) [3, 6) [6, 9)
    n3.process(x[:, :3])
    src = [8, 2, 3, 6]
    rec = n3.export_streams(src)
    n2 = nn.NodeDenoiser(6, (0, 0), lib=hostsim_lib)             # shards [0, 3) [3, 6)
    n2.process(make_streams(31, 6, 2))
    dst = [0, 5, 3, 2]
    n2.import_streams(dst, rec)
    y = np.zeros((6, 4, 480), np.float32)
    y[dst] = x[src, 3:7]
    out3, _ = n3.process(x[:, 3:7])
    out2, _ = n2.process(y)
    assert np.array_equal(_bits(out3[src]), _bits(out2[dst]))
    # reset across two shards: those streams start over, the others carry on
    ref = nn.NodeDenoiser(S, (0, 0, 0), lib=hostsim_lib)
    ref.process(x[:, :7])
    n3.reset_streams([2, 4])
    ref_out, _ = ref.process(x[:, 7:8])
    got, _ = n3.process(x[:, 7:8])
    fresh, _ = nn.BatchDenoiser(2, lib=hostsim_lib).process(x[[2, 4], 7:8])
    assert np.array_equal(_bits(got[[2, 4]]), _bits(fresh))
    rest = [s for s in range(S) if s not in (2, 4)]
    assert np.array_equal(_bits(got[rest]), _bits(ref_out[rest]))
    with pytest.raises(RuntimeError):
        n2.import_streams([0, 0], np.concatenate([rec[:1], rec[:1]]))
    with pytest.raises(RuntimeError):
        n3.export_streams([9])
