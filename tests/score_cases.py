"""Shared by the scorer's tests (include/nnn_score.h): a NumPy float64 restatement of the header's sums, written
from the header's stated order -- sequential where the kernel's lanes add sequentially, pairwise where its tree does --, the memory the
calls are made on (the interpreter's "device" memory is the host's; on the GPU it is torch's) and the checks the interpreter tests and the
GPU tests both make.  Every comparison is of the raw 8-byte words; the one thing the header leaves open, WHICH NaN a non-finite sum is,
is taken out by writing every NaN as one (bits)."""
import numpy as np

FRAME = 480
DELAYS = (0, 1, 3, 479, 480, 481, 960)
GARBAGE = 7.25e5          # what the gaps between frames hold: a read outside a frame shows
SHAPES = [(1, 1), (3, 1), (5, 3), (70, 7)]   # a lone wave, a partial block, more than one block


def bits(a):
    """float64 array -> its 8-byte words, every NaN written as the same one."""
    a = np.array(a, dtype=np.float64)
    a[np.isnan(a)] = np.nan
    return a.view(np.uint64)


def assert_same(got, want, tag=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    if got.dtype == np.float64:
        got, want = bits(got), bits(want)
    assert np.array_equal(got, want), (tag, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def reduce480(t):
    """The header's order over the last axis (480 terms): 64 partial sums from +0.0, each over its terms i = L + 64 k in ascending k;
    then p_L <- p_L + p_(L xor m) for m = 32 .. 1; the sum is p_0."""
    p = np.zeros(t.shape[:-1] + (64,), np.float64)
    for k in range(8):
        n = min(64, FRAME - 64 * k)
        p[..., :n] = p[..., :n] + t[..., 64 * k:64 * k + n]
    lanes = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        p = p + p[..., lanes ^ m]
    return p[..., 0]


def frame_sums(rwin, y):
    """float32 [..., 480] reference window and test frame -> float64 [..., 4]: A, B, C, E."""
    with np.errstate(all="ignore"):
        rd, yd = rwin.astype(np.float64), y.astype(np.float64)
        d = rd - yd
        return np.stack([reduce480(rd * rd), reduce480(yd * yd), reduce480(rd * yd), reduce480(d * d)], axis=-1)


class Restated:
    """The object of include/nnn_score.h on the host."""

    def __init__(self, S, max_delay, delays=None):
        self.S, self.H = S, max_delay
        self.delay = np.zeros(S, np.int64) if delays is None else np.asarray(delays, np.int64).copy()
        self.hist = np.zeros((S, max_delay), np.float32)
        self.tot, self.cnt = np.zeros((S, 4), np.float64), np.zeros(S, np.uint64)

    def reset(self, idx=None):
        idx = np.arange(self.S) if idx is None else np.asarray(idx)
        self.hist[idx], self.tot[idx], self.cnt[idx] = 0.0, 0.0, 0

    def set_delay(self, idx, delays):
        idx = np.arange(self.S) if idx is None else np.asarray(idx)
        self.delay[idx] = delays
        self.reset(idx)

    def accumulate(self, ref, test, valid=None):
        """ref / test float32 [S, T, 480]; valid [T, S] or None -> frame sums float64 [T, S, 4]."""
        S, T, _ = ref.shape
        ext = np.concatenate([self.hist, ref.reshape(S, T * FRAME)], axis=1)
        out = np.zeros((T, S, 4), np.float64)
        for f in range(T):
            at = (self.H + f * FRAME - self.delay)[:, None] + np.arange(FRAME)[None, :]
            fs = frame_sums(np.take_along_axis(ext, at, axis=1), test[:, f])
            on = np.ones(S, bool) if valid is None else np.asarray(valid[f]) != 0
            out[f][on] = fs[on]
            with np.errstate(all="ignore"):
                self.tot[on] = self.tot[on] + fs[on]
            self.cnt[on] += np.uint64(1)
        self.hist = ext[:, ext.shape[1] - self.H:].copy()
        return out


# ---- memory the device-style calls are made on ---------------------------------------------------------------------------------------------
class Handle:
    def __init__(self, ptr, get, keep):
        self.ptr, self.get, self.keep = ptr, get, keep


class HostMem:
    """The interpreter's device memory is the host's.  put: a copy of `arr` whose first element lies 4 * skip bytes (for float32) behind
    a 16-byte boundary, garbage in front of it."""
    stream = 0

    def put(self, arr, skip=0):
        arr = np.ascontiguousarray(arr).reshape(-1)
        per = 16 // arr.dtype.itemsize
        raw = np.full(arr.size + skip + per, 99, arr.dtype)
        a0 = ((-raw.ctypes.data) % 16) // arr.dtype.itemsize + skip
        view = raw[a0:a0 + arr.size]
        view[:] = arr
        return Handle(view.ctypes.data, lambda: view.copy(), raw)

    def sync(self):
        pass


class TorchMem:
    """torch tensors on the GPU; put(skip > 0) hands out a view that starts `skip` elements into its tensor.  The calls go on a stream of
    torch's (not its default stream: handle 0 means "the object's own stream" to the library)."""

    def __init__(self):
        import torch
        self.torch = torch
        self._st = torch.cuda.Stream()
        self.stream = self._st.cuda_stream

    def put(self, arr, skip=0):
        arr = np.ascontiguousarray(arr).reshape(-1)
        dt = arr.dtype
        if dt == np.uint64:
            arr = arr.view(np.int64)                 # (the same bits in a type torch has)
        t = self.torch.from_numpy(np.concatenate([np.full(skip, 99, arr.dtype), arr])).to("cuda")
        v = t[skip:]
        self.torch.cuda.synchronize()
        return Handle(v.data_ptr(), lambda: v.cpu().numpy().view(dt), t)

    def sync(self):
        self.torch.cuda.synchronize()


def strides(S, T, layout, frame_pad=0, stream_pad=0):
    """(stream_stride, frame_stride) in floats: "frames" is the batch's [T][S][480], "streams" per-stream-contiguous [S][T][480]; the pads
    widen a frame and a stream (or a row of frames) by that many floats."""
    if layout == "frames":
        ss = FRAME + frame_pad
        return ss, S * ss + stream_pad
    fs = FRAME + frame_pad
    return T * fs + stream_pad, fs


def lay_out(x, ss, fs):
    """x [S, T, 480] as the flat buffer with element (s, f, i) at s * ss + f * fs + i and GARBAGE everywhere else."""
    S, T, _ = x.shape
    buf = np.full((S - 1) * ss + (T - 1) * fs + FRAME, GARBAGE, np.float32)
    at = (np.arange(S) * ss)[:, None, None] + (np.arange(T) * fs)[None, :, None] + np.arange(FRAME)[None, None, :]
    buf[at] = x
    return buf


def device_call(sc, mem, ref, test, valid=None, layout="frames", frame_pad=0, stream_pad=0, skip=(0, 0), sums=True):
    """nnn_score_accumulate_device on copies of ref / test [S, T, 480] in the given layout; returns the frame sums [T, S, 4] (or None)."""
    S, T, _ = ref.shape
    ss, fs = strides(S, T, layout, frame_pad, stream_pad)
    r, y = mem.put(lay_out(ref, ss, fs), skip[0]), mem.put(lay_out(test, ss, fs), skip[1])
    v = None if valid is None else mem.put(np.ascontiguousarray(valid, dtype=np.uint8))
    out = mem.put(np.full((T, S, 4), 123.0, np.float64)) if sums else None
    sc.accumulate_device(r.ptr, y.ptr, T, ss, fs, d_valid=None if v is None else v.ptr, d_frame_sums=None if out is None else out.ptr,
                         hip_stream=mem.stream)
    mem.sync()
    return None if out is None else out.get().reshape(T, S, 4)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def signals(seed, S, T):
    """ref and test float32 [S, T, 480], uniform in the int16 range (not whole numbers: every rounding of the sums matters); a tenth of the
    frames of each all zero."""
    rng = np.random.default_rng(seed)
    r, y = (rng.uniform(-32768.0, 32767.0, (S, T, FRAME)).astype(np.float32) for _ in range(2))
    r[rng.random((S, T)) < 0.1] = 0.0
    y[rng.random((S, T)) < 0.1] = 0.0
    if S * T >= 2:
        r.reshape(-1, FRAME)[0], y.reshape(-1, FRAME)[-1] = 0.0, 0.0
    return r, y


def mixed_delays(S):
    return np.array([DELAYS[(s + S) % len(DELAYS)] for s in range(S)], np.int64)


def scorer(lib, S, delays=None, max_delay=960):
    from nnnoiseless_amd.score import Scorer
    sc = Scorer(S, max_delay, lib=lib)
    if delays is not None:
        sc.set_delay(None, delays)
    return sc


def assert_totals(sc, rs, tag=""):
    tot, cnt = sc.totals()
    assert_same(tot, rs.tot, tag + " totals")
    assert_same(cnt, rs.cnt, tag + " counts")


# ---- the checks ----------------------------------------------------------------------------------------------------------------------------
def check_restatement(lib, mem, S, T):
    """Two calls of T frames (the second reads the history the first left), delays 0 .. 960 mixed across the streams: frame sums and
    totals equal the restatement."""
    d = mixed_delays(S)
    sc, rs = scorer(lib, S, d), Restated(S, 960, d)
    for call in range(2):
        r, y = signals(10 * S + T + call, S, T)
        assert_same(device_call(sc, mem, r, y), rs.accumulate(r, y), f"call {call} frame sums")
        assert_totals(sc, rs, f"call {call}")
    assert (rs.tot[:, 0] != 0).any()
    sc.close()


def check_chunking(lib, mem, S=5, T=7):
    """Seven frames as one call, as 1 + 2 + 4 and as seven calls of one frame, at delay 960 (a one-frame call is shorter than the delay:
    the history shifts); then an eighth frame on each."""
    r, y = signals(77, S, T + 1)
    rs = Restated(S, 960, np.full(S, 960))
    want = np.concatenate([rs.accumulate(r[:, :T], y[:, :T]), rs.accumulate(r[:, T:], y[:, T:])])
    assert (want[T:, :, 2] != 0).any() and (want[2, :, 0] != 0).any()
    for cuts in ([7], [1, 2, 4], [1] * 7):
        sc, got, t = scorer(lib, S, np.full(S, 960)), [], 0
        for n in cuts + [1]:
            got.append(device_call(sc, mem, r[:, t:t + n], y[:, t:t + n], layout="streams"))
            t += n
        assert_same(np.concatenate(got), want, f"cuts {cuts}")
        assert_totals(sc, rs, f"cuts {cuts}")
        sc.close()


def check_layout(lib, mem, S=5, T=3):
    """The batch's [T][S][480] against per-stream-contiguous audio, and 16-byte aligned frames against unaligned ones: a base that is 4-byte
    but not 16-byte aligned, a frame stride that is no multiple of 4, a stream stride that is none."""
    d = np.array([0, 480, 1, 3, 960])[:S]
    r, y = signals(5, S, 2 * T)
    rs = Restated(S, 960, d)
    want = [rs.accumulate(r[:, :T], y[:, :T]), rs.accumulate(r[:, T:], y[:, T:])]
    for kw in ({"layout": "frames"}, {"layout": "streams"}, {"layout": "streams", "stream_pad": 8}, {"layout": "frames", "skip": (1, 0)},
               {"layout": "frames", "skip": (0, 3)}, {"layout": "streams", "skip": (2, 2)}, {"layout": "streams", "frame_pad": 1},
               {"layout": "frames", "frame_pad": 2}, {"layout": "frames", "stream_pad": 1}, {"layout": "streams", "frame_pad": 4, "skip": (4, 8)}):
        sc = scorer(lib, S, d)
        for call in range(2):
            got = device_call(sc, mem, r[:, call * T:(call + 1) * T], y[:, call * T:(call + 1) * T], **kw)
            assert_same(got, want[call], f"{kw} call {call}")
        assert_totals(sc, rs, str(kw))
        sc.close()


def check_valid(lib, mem, S=5, T=8):
    """A quarter of the frames marked 0: their rows are zeros, totals and counts leave them out, and their reference samples still pass
    -- the frame behind a masked one sees them at delay 480."""
    d = np.array([480, 0, 481, 960, 480])[:S]
    r, y = signals(9, S, T)
    r[0, 2], y[0, 3] = r[0, 2] + np.float32(0.5), y[0, 3] + np.float32(0.5)   # (neither is one of the all-zero frames)
    valid = np.ones((T, S), np.uint8)
    valid.reshape(-1)[::4] = 0
    valid[2, 0], valid[3, 0] = 0, 1
    sc, rs = scorer(lib, S, d), Restated(S, 960, d)
    got = device_call(sc, mem, r[:, :5], y[:, :5], valid[:5])
    got = np.concatenate([got, device_call(sc, mem, r[:, 5:], y[:, 5:], valid[5:], layout="streams", skip=(1, 1))])
    want = np.concatenate([rs.accumulate(r[:, :5], y[:, :5], valid[:5]), rs.accumulate(r[:, 5:], y[:, 5:], valid[5:])])
    assert_same(got, want, "frame sums")
    assert (got[valid == 0] == 0).all() and (valid == 0).sum() >= T * S // 4
    assert_same(got[3, 0], frame_sums(r[0, 2], y[0, 3]), "the frame behind a masked one")
    assert r[0, 2].any() and y[0, 3].any()
    assert_totals(sc, rs)
    assert np.array_equal(sc.totals()[1], valid.sum(axis=0).astype(np.uint64))
    sc.close()


def check_identities(lib, mem, S=3, T=3):
    """test == ref at delay 0: E = 0 and A, B, C the same bits.  test == -ref: C = -A and E = 4 A.  An impulse as reference: at delay d
    only the test sample d later enters C."""
    r, _ = signals(3, S, T)
    sc = scorer(lib, S)
    fs = device_call(sc, mem, r, r.copy())
    assert (fs[..., 3] == 0).all() and (fs[..., 0] != 0).any()
    assert_same(fs[..., 1], fs[..., 0]), assert_same(fs[..., 2], fs[..., 0])
    sc.reset()
    fs = device_call(sc, mem, r, -r, layout="streams", skip=(1, 1))
    assert_same(fs[..., 2] + 0.0, -fs[..., 0] + 0.0), assert_same(fs[..., 3], 4.0 * fs[..., 0])   # (+ 0.0: an all-zero frame's C is +0, not -0)
    sc.close()
    delays = np.array([0, 1, 3, 479, 480, 481, 960])
    S = delays.size
    y = np.random.default_rng(4).uniform(1.0, 30000.0, (S, 4, FRAME)).astype(np.float32)
    imp = np.zeros((S, 4, FRAME), np.float32)
    at = 100 + 37 * np.arange(S)                       # the impulse's sample in its stream
    imp.reshape(S, -1)[np.arange(S), at] = 3.0
    sc = scorer(lib, S, delays)
    fs = device_call(sc, mem, imp[:, :1], y[:, :1])
    fs = np.concatenate([fs, device_call(sc, mem, imp[:, 1:], y[:, 1:])])
    hit = y.reshape(S, -1)[np.arange(S), at + delays].astype(np.float64)
    want = np.zeros((4, S))
    want[(at + delays) // FRAME, np.arange(S)] = 3.0 * hit
    assert (hit != 0).all()
    assert_same(fs[..., 2], want, "C")
    assert_same(fs[..., 0].sum(axis=0), np.full(S, 9.0), "A")
    sc.close()


def check_range(lib, mem, S=4, T=3):
    """f32 subnormals (2^-140) and 3e38: the squares fit f64.  One NaN and one inf sample poison their own frame's sums and their
    stream's totals, and nothing else."""
    r, y = signals(6, S, T)
    r[0, 0, :240], y[0, 0, 240:] = np.float32(2.0 ** -140), np.float32(2.0 ** -140)
    r[0, 0, 240:], y[0, 0, :240] = np.float32(2.0 ** -141), np.float32(-2.0 ** -149)
    r[1, 1, ::2], y[1, 1, ::3] = np.float32(3e38), np.float32(-3e38)
    y[2, 1, 17] = np.nan
    r[3, 1, 400] = np.inf                            # (stream 3 has delay 480: frame 2 sees it)
    r[3, 2, 5] = np.inf                              # (and this one is the next call's to see)
    y[3, 2] = 1.0
    d = np.array([0, 1, 0, 480])[:S]
    sc, rs = scorer(lib, S, d), Restated(S, 960, d)
    got, want = device_call(sc, mem, r, y), rs.accumulate(r, y)
    assert_same(got, want)
    assert_totals(sc, rs)
    assert (got[0, 0] > 0).all() and (got[0, 0] < 1e-70).all() and np.isfinite(got[1, 1]).all() and (got[1, 1, [0, 1, 3]] > 1e76).all()
    bad = ~np.isfinite(got).all(axis=-1)
    assert np.array_equal(np.argwhere(bad), [[1, 2], [2, 3]]), np.argwhere(bad)
    assert np.isnan(got[1, 2, 1:]).all() and np.isfinite(got[1, 2, 0]) and got[2, 3, 0] == np.inf
    tot, _ = sc.totals()
    assert np.isfinite(tot[:2]).all() and not np.isfinite(tot[2:]).all(axis=-1).any()
    # an inf sits in the history now: it reaches the next call's first frame at delay 480, and that frame alone
    r2, y2 = signals(8, S, 2)
    y2[3] = 2.0
    got2 = device_call(sc, mem, r2, y2)
    assert_same(got2, rs.accumulate(r2, y2), "behind the inf")
    assert got2[0, 3, 0] == np.inf and np.isfinite(got2[1]).all() and np.isfinite(got2[0, :3]).all()
    sc.close()


def check_reset(lib, mem, S=5, T=2):
    """Per-stream reset: totals, count and history of the named streams to zero, the others go on bit for bit, the delays stay; set_delay
    does the same with a new delay."""
    d = np.array([960, 480, 481, 3, 960])[:S]
    r, y = signals(12, S, 3 * T)
    sc, rs = scorer(lib, S, d), Restated(S, 960, d)
    assert_same(device_call(sc, mem, r[:, :T], y[:, :T]), rs.accumulate(r[:, :T], y[:, :T]))
    sc.reset([4, 1]), rs.reset([4, 1])
    assert np.array_equal(sc.delay(), d) and np.array_equal(sc.delay([4, 0]), d[[4, 0]])
    assert_totals(sc, rs, "after the reset")
    assert (rs.tot[[1, 4]] == 0).all() and (rs.cnt[[0, 2, 3]] == T).all()
    assert_same(device_call(sc, mem, r[:, T:2 * T], y[:, T:2 * T]), rs.accumulate(r[:, T:2 * T], y[:, T:2 * T]), "behind the reset")
    fresh = Restated(S, 960, d)                                   # streams 1 and 4 are where a new object would be, the others are not
    fresh.accumulate(r[:, T:2 * T], y[:, T:2 * T])
    assert_same(sc.totals()[0][[1, 4]], fresh.tot[[1, 4]], "the reset streams")
    assert not np.array_equal(bits(sc.totals()[0][[0, 2, 3]]), bits(fresh.tot[[0, 2, 3]]))
    sc.set_delay([2, 0], [7, 0]), rs.set_delay([2, 0], [7, 0])
    assert np.array_equal(sc.delay(), rs.delay)
    assert_totals(sc, rs, "after set_delay")
    assert_same(device_call(sc, mem, r[:, 2 * T:], y[:, 2 * T:]), rs.accumulate(r[:, 2 * T:], y[:, 2 * T:]), "behind set_delay")
    assert_totals(sc, rs, "at the end")
    sc.reset(), rs.reset()
    assert_totals(sc, rs, "after the whole reset")
    assert np.array_equal(sc.delay(), rs.delay)
    sc.close()


def check_twice(lib, mem, S=70, T=3):
    """The same calls on two fresh objects: the same bits."""
    d = mixed_delays(S)
    r, y = signals(21, S, T)
    res = []
    for _ in range(2):
        sc = scorer(lib, S, d)
        fs = device_call(sc, mem, r, y)
        device_call(sc, mem, y, r, layout="streams", sums=False)
        res.append((fs,) + sc.totals())
        sc.close()
    for a, b in zip(*res):
        assert_same(a, b)


def check_host_call(lib, mem, S=5, T=3):
    """The host call (dense [S][T][480]) gives the device-style call's bits, with and without a mask and a table."""
    d = mixed_delays(S)
    r, y = signals(31, S, 2 * T)
    valid = (np.arange(T * S).reshape(T, S) % 3 != 1).astype(np.uint8)
    a, b = scorer(lib, S, d), scorer(lib, S, d)
    assert_same(a.accumulate(r[:, :T], y[:, :T], frame_sums=True), device_call(b, mem, r[:, :T], y[:, :T]))
    assert_same(a.accumulate(r[:, T:], y[:, T:], valid, frame_sums=True), device_call(b, mem, r[:, T:], y[:, T:], valid))
    assert a.accumulate(r[:, :T], y[:, :T]) is None
    device_call(b, mem, r[:, :T], y[:, :T], sums=False)
    for x, z in zip(a.totals(), b.totals()):
        assert_same(x, z)
    # totals_device: the same numbers in the caller's memory
    t, c = mem.put(np.zeros((S, 4), np.float64)), mem.put(np.zeros(S, np.uint64))
    b.totals_device(t.ptr, c.ptr, mem.stream)
    mem.sync()
    assert_same(t.get().reshape(S, 4), a.totals()[0]), assert_same(c.get(), a.totals()[1])
    a.close(), b.close()
