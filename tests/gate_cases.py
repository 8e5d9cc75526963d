"""Shared by the VAD gate's tests (include/nnn_gate.h): a NumPy restatement of the header's rule, written from the
header -- a Python loop over frames for the counter, float32 NumPy operations for the at most three roundings per sample --, the calls
on every layout the header allows, and the checks the interpreter tests and the GPU tests both make.  Every comparison is of raw bits:
float32 as uint32, int16, the open bytes, the exported records byte for byte."""
import numpy as np

from score_cases import HostMem, TorchMem  # noqa: F401  (the memory the device-style calls are made on; the test files make one)

FRAME = 480
NEVER = 0x7fffffff
RS, GS, LV, TH = (0, 1, 3, 8), (0, 2, 7), (0.0, 0.1, 1.0), (0.5, 0.25, 0.0)
RAMP = np.arange(1, FRAME + 1, dtype=np.float32) / np.float32(480.0)
GARBAGE = np.float32(7.25e5)      # what the gaps between frames hold
SENT = np.float32(-7.5e5)         # what an output buffer holds before an out-of-place call
SENT16 = np.int16(-12345)
SENT_OPEN = np.uint8(0xEE)
SHAPES = [(1, 1), (3, 2), (5, 5), (70, 11)]
F32, I16, F32_UNIT = 0, 1, 2


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


def assert_same(got, want, tag=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    g, w = bits(got), bits(want)
    assert np.array_equal(g, w), (tag, int((g != w).sum()), np.argwhere(g != w)[:4].tolist())


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def round_i16(y):
    """The batch's int16 writer: clamp, then round half away from zero (in float64, where y +- 0.5 is exact)."""
    y = np.clip(y.astype(np.float64), -32768.0, 32767.0)
    return np.where(y >= 0, np.floor(y + 0.5), np.ceil(y - 0.5)).astype(np.int16)


def params(S, rot=0):
    """Mixed per-stream parameters: every R, G, level and threshold of the issue's lists, turned by `rot`."""
    s = np.arange(S)
    return {"threshold": np.array(TH, np.float32)[(s // 2 + rot) % 3], "grace": np.array(GS)[(s + rot // 2) % 3],
            "lookback": np.array(RS)[(s + rot) % 4], "level": np.array(LV, np.float32)[(s // 3 + rot) % 3]}


class Restated:
    """The object of include/nnn_gate.h on the host."""

    def __init__(self, S, max_lookback=8, par=None):
        self.S, self.H = S, max_lookback
        self.thr, self.lvl = np.zeros(S, np.float32), np.zeros(S, np.float32)
        self.G, self.R = np.zeros(S, np.int64), np.zeros(S, np.int64)
        self.since, self.was = np.full(S, NEVER, np.int64), np.zeros(S, np.int64)
        self.hist = np.zeros((S, 8, FRAME), np.float32)
        if par is not None:
            self.set_params(None, par)

    def reset(self, idx=None):
        idx = np.arange(self.S) if idx is None else np.asarray(idx)
        self.since[idx], self.was[idx], self.hist[idx] = NEVER, 0, 0.0

    def set_params(self, idx, par):
        idx = np.arange(self.S) if idx is None else np.asarray(idx)
        self.thr[idx], self.G[idx], self.R[idx], self.lvl[idx] = par["threshold"], par["grace"], par["lookback"], par["level"]
        self.reset(idx)

    def apply(self, x, vad, live=None, base=None, i16=False):
        """x float32 [S, T, 480] (for i16: the int16 samples as floats), vad [T, S] -> (y [S, T, 480] float32 or int16, open uint8 [T, S]).
        What a stream marked 0 owns is `base`'s (default: the sentinels)."""
        S, T, _ = x.shape
        y = np.full(x.shape, SENT16 if i16 else SENT) if base is None else np.array(base)
        opn = np.full((T, S), SENT_OPEN)
        one = np.float32(1.0)
        for s in range(S):
            if live is not None and not live[s]:
                continue
            R, lim, thr, lvl = int(self.R[s]), int(self.G[s] + self.R[s]), self.thr[s], self.lvl[s]
            ext = np.concatenate([self.hist[s, :R], x[s]])           # row t is the source of frame t: in_(t-R)
            since, was = int(self.since[s]), int(self.was[s])
            for t in range(T):
                voiced = bool(vad[t, s] >= thr)                      # step 1 (NaN: False)
                since = 0 if voiced else min(since + 1, NEVER)       # step 2
                o = since <= lim                                     # step 3
                hn, hp = (one if o else lvl), (one if was else lvl)  # step 4
                src = ext[t]                                         # step 5
                g = np.full(FRAME, hn) if hp == hn else hp + (hn - hp) * RAMP   # step 6: float32 operations, one rounding each
                with np.errstate(all="ignore"):
                    prod = src * g
                yb = np.where(g == one, bits(src), np.where(g == 0, np.uint32(0), bits(prod)))   # step 7
                yf = yb.astype(np.uint32).view(np.float32)
                y[s, t] = round_i16(yf) if i16 else yf
                opn[t, s] = o
                was = int(o)
            self.since[s], self.was[s] = since, was
            self.hist[s, :R] = ext[T:T + R]
        return y, opn

    def export(self, idx=None):
        from nnnoiseless_amd import _ffi
        idx = np.arange(self.S) if idx is None else np.asarray(idx)
        rec = np.zeros(len(idx), _ffi.GATE_STATE_DTYPE)
        rec["magic"], rec["version"], rec["size"] = _ffi.GATE_STATE_MAGIC, _ffi.GATE_STATE_VERSION, _ffi.GATE_STATE_BYTES
        rec["threshold"], rec["grace"], rec["lookback"], rec["level"] = self.thr[idx], self.G[idx], self.R[idx], self.lvl[idx]
        rec["since"], rec["was_open"] = self.since[idx], self.was[idx]
        for k, s in enumerate(idx):
            rec["history"][k, :self.R[s]] = self.hist[s, :self.R[s]]
        return rec.view(np.uint8).reshape(len(idx), _ffi.GATE_STATE_BYTES)

    def import_(self, idx, records):
        from nnnoiseless_amd import _ffi
        rec = np.ascontiguousarray(records).view(_ffi.GATE_STATE_DTYPE).reshape(-1)
        for k, s in enumerate(idx):
            self.thr[s], self.G[s], self.R[s], self.lvl[s] = rec["threshold"][k], rec["grace"][k], rec["lookback"][k], rec["level"][k]
            self.since[s], self.was[s] = rec["since"][k], rec["was_open"][k]
            self.hist[s] = rec["history"][k]


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def audio(seed, S, T, whole=False):
    """float32 [S, T, 480] uniform in the int16 range: not whole numbers (the product with a level rounds) unless `whole` (int16 data)."""
    x = np.random.default_rng(seed).uniform(-32768.0, 32767.0, (S, T, FRAME)).astype(np.float32)
    return np.round(x) if whole else x


def vad_rows(seed, T, thr):
    """float32 [T, S]: runs of voiced and unvoiced frames per stream, so a gate opens and closes at every grace period; voiced values
    include the threshold itself, unvoiced ones NaN and the float just below the threshold."""
    rng = np.random.default_rng(seed)
    S = len(thr)
    v = np.zeros((T, S), np.float32)
    for s in range(S):
        on = bool(rng.integers(2))
        for t in range(T):
            if rng.random() < (0.45 if on else 0.2):
                on = not on
            below = np.nextafter(thr[s], np.float32(-1.0))
            v[t, s] = rng.choice([thr[s], 0.7, 0.9, 1.0]) if on else rng.choice([0.0, 0.1, np.nan, below if thr[s] > 0 else np.nan])
            if not on and thr[s] == 0 and not np.isnan(v[t, s]):
                v[t, s] = np.nan                                     # (threshold 0: only NaN is unvoiced)
    return v


def gate(lib, S, H=8, par=None):
    from nnnoiseless_amd.gate import VadGate
    g = VadGate(S, H, lib=lib)
    if par is not None:
        g.set_params(par["threshold"], par["grace"], par["lookback"], par["level"])
    return g


# ---- the calls -----------------------------------------------------------------------------------------------------------------------------
def f32_index(S, T, layout="frames", frame_pad=0, stream_pad=0):
    """(element index [S, T, 480], stream_stride, frame_stride): "frames" is the batch's [T][S][480], "streams" per-stream-contiguous."""
    if layout == "frames":
        ss = FRAME + frame_pad
        fs = S * ss + stream_pad
    else:
        fs = FRAME + frame_pad
        ss = T * fs + stream_pad
    at = (np.arange(S) * ss)[:, None, None] + (np.arange(T) * fs)[None, :, None] + np.arange(FRAME)[None, None, :]
    return at, ss, fs


def pcm_index(S, T, C, frame_pad=0, group_pad=0):
    fs = FRAME * C + frame_pad
    gs = T * fs + group_pad
    s = np.arange(S)
    at = ((s // C) * gs + s % C)[:, None, None] + (np.arange(T) * fs)[None, :, None] + (np.arange(FRAME) * C)[None, None, :]
    return at, gs, fs


def _run(g, mem, call, x, vad, at, dtype, live, inplace, want_open, skip):
    """Lay x out at `at` in a buffer of GARBAGE, make the call, return (y [S, T, 480], open [T, S] or None); everything outside the frames
    and everything a masked stream owns must come back as it was."""
    S, T, _ = x.shape
    n = int(at.max()) + 1
    garbage, sent = (np.int16(9999), SENT16) if dtype == np.int16 else (GARBAGE, SENT)
    buf = np.full(n, garbage, dtype)
    buf[at] = x.astype(dtype)
    hin = mem.put(buf, skip)
    hout = hin if inplace else mem.put(np.full(n, sent, dtype), skip)
    hv = mem.put(np.ascontiguousarray(vad, dtype=np.float32))
    hl = None if live is None else mem.put(np.ascontiguousarray(live, dtype=np.uint8))
    ho = mem.put(np.full((T, S), SENT_OPEN, np.uint8)) if want_open else None
    call(hin.ptr, hout.ptr, hv.ptr, None if hl is None else hl.ptr, None if ho is None else ho.ptr)
    mem.sync()
    res = hout.get()
    outside = np.ones(n, bool)
    outside[at] = False
    assert (res[outside] == (garbage if inplace else sent)).all(), "a write outside the frames"
    if not inplace:
        assert_same(hin.get(), buf, "the input of an out-of-place call")
    return res[at], None if ho is None else ho.get().reshape(T, S)


def device_call(g, mem, x, vad, live=None, inplace=False, want_open=True, skip=0, **layout):
    S, T, _ = x.shape
    at, ss, fs = f32_index(S, T, **layout)
    return _run(g, mem, lambda i, o, v, l, op: g.apply_device(i, o, v, T, ss, fs, d_live=l, d_open=op, hip_stream=mem.stream),
                x, vad, at, np.float32, live, inplace, want_open, skip)


def pcm_call(g, mem, x, vad, fmt, C, live=None, inplace=False, want_open=True, skip=0, **pads):
    S, T, _ = x.shape
    at, gs, fs = pcm_index(S, T, C, **pads)
    return _run(g, mem, lambda i, o, v, l, op: g.apply_pcm_device(i, o, v, T, fmt, C, gs, fs, d_live=l, d_open=op, hip_stream=mem.stream),
                x, vad, at, np.int16 if fmt == I16 else np.float32, live, inplace, want_open, skip)


def assert_records(g, rs, tag=""):
    assert_same(g.export_streams(None), rs.export(), tag + " records")


# ---- the checks ----------------------------------------------------------------------------------------------------------------------------
def check_restatement(lib, mem, S, T, rots=(0, 1, 2, 3)):
    """Two calls of T frames (the second reads the state the first left) under mixed parameters, out of place then in place: audio, open
    flags and records equal the restatement.  Across the rotations every stream position sees every look-back: T < R, T == R and T > R."""
    opened = closed = False
    for rot in rots:
        par = params(S, rot)
        g, rs = gate(lib, S, 8, par), Restated(S, 8, par)
        for call in range(2):
            x, v = audio(100 * S + 10 * T + call, S, T), vad_rows(7 * S + T + call + rot, T, par["threshold"])
            y, o = device_call(g, mem, x, v, inplace=bool(call))
            wy, wo = rs.apply(x, v)
            assert_same(y, wy, f"rot {rot} call {call} audio"), assert_same(o, wo, f"rot {rot} call {call} open")
            assert_records(g, rs, f"rot {rot} call {call}")
            opened, closed = opened or bool((wo == 1).any()), closed or bool((wo == 0).any())
        g.close()
    assert opened and (closed or S * T == 1)


def check_chunking(lib, mem, S=8, T=11):
    """Eleven frames as one call, as 1 + 10, as 3 + 8 and as eleven calls of one frame: the same audio, open flags and records."""
    par = params(S, 1)
    x, v = audio(77, S, T), vad_rows(78, T, par["threshold"])
    rs = Restated(S, 8, par)
    wy, wo = rs.apply(x, v)
    assert (wo == 1).any() and (wo == 0).any() and set(par["lookback"]) == set(RS)
    for cuts in ([11], [1, 10], [3, 8], [1] * 11):
        g, ys, os_, t = gate(lib, S, 8, par), [], [], 0
        for k, n in enumerate(cuts):
            y, o = device_call(g, mem, x[:, t:t + n], v[t:t + n], layout="streams", inplace=bool(k & 1))
            ys.append(y), os_.append(o)
            t += n
        assert_same(np.concatenate(ys, axis=1), wy, f"cuts {cuts} audio"), assert_same(np.concatenate(os_), wo, f"cuts {cuts} open")
        assert_records(g, rs, f"cuts {cuts}")
        g.close()


def check_in_place(lib, mem, T=5):
    """In place equals out of place, for every look-back 0 .. 8, over three calls (one of them shorter than the longest look-back)."""
    S = 9
    par = {"threshold": np.full(S, 0.5, np.float32), "grace": np.arange(S) % 3, "lookback": np.arange(S), "level": np.array(LV, np.float32)[np.arange(S) % 3]}
    a, b, rs = gate(lib, S, 8, par), gate(lib, S, 8, par), Restated(S, 8, par)
    for call, n in enumerate((T, 2, T)):
        x, v = audio(30 + call, S, n), vad_rows(40 + call, n, par["threshold"])
        ya, oa = device_call(a, mem, x, v, inplace=True)
        yb, ob = device_call(b, mem, x, v, inplace=False)
        wy, wo = rs.apply(x, v)
        assert_same(ya, wy, f"call {call} in place"), assert_same(yb, wy, f"call {call} out of place")
        assert_same(oa, wo), assert_same(ob, wo)
    assert_records(a, rs, "in place"), assert_records(b, rs, "out of place")
    a.close(), b.close()


def check_layout(lib, mem, S=6, T=3):
    """Padded strides, both orders of streams and frames, a base at an odd float; the packed boundary at one and two channels in all three
    formats with padding, and an int16 base at an odd element.  Two calls each, in place and out of place."""
    par = params(S, 2)
    xs, vs = [audio(5 + c, S, T, whole=True) for c in range(2)], [vad_rows(15 + c, T, par["threshold"]) for c in range(2)]

    def want(i16):
        rs = Restated(S, 8, par)
        return [rs.apply(xs[c], vs[c], i16=i16) for c in range(2)], rs

    (wf, rf), (wi, ri) = want(False), want(True)
    assert any((o == 1).any() for _, o in wf) and any((o == 0).any() for _, o in wf)
    for kw in ({"layout": "frames"}, {"layout": "streams"}, {"layout": "streams", "stream_pad": 8}, {"layout": "frames", "skip": 1},
               {"layout": "streams", "skip": 3}, {"layout": "streams", "frame_pad": 1}, {"layout": "frames", "frame_pad": 2},
               {"layout": "frames", "stream_pad": 1}, {"layout": "streams", "frame_pad": 4, "skip": 2}):
        for inplace in (False, True):
            g = gate(lib, S, 8, par)
            for c in range(2):
                y, o = device_call(g, mem, xs[c], vs[c], inplace=inplace, **kw)
                assert_same(y, wf[c][0], f"{kw} in place {inplace} call {c}"), assert_same(o, wf[c][1])
            assert_records(g, rf, str(kw))
            g.close()
    for fmt in (F32, I16, F32_UNIT):
        for C in (1, 2):
            for kw in ({}, {"skip": 1}, {"frame_pad": 2 * C + 1, "group_pad": 3}, {"frame_pad": 4, "skip": 3 if fmt == I16 else 2}):
                for inplace in (False, True):
                    g = gate(lib, S, 8, par)
                    w, r = (wi, ri) if fmt == I16 else (wf, rf)
                    for c in range(2):
                        y, o = pcm_call(g, mem, xs[c], vs[c], fmt, C, inplace=inplace, **kw)
                        assert_same(y, w[c][0], f"format {fmt} channels {C} {kw} in place {inplace} call {c}"), assert_same(o, w[c][1])
                    assert_records(g, r, f"format {fmt} channels {C} {kw}")
                    g.close()
    # an open gate returns the int16 unchanged: threshold 0, the stream's own input one look-back late
    g = gate(lib, S, 8, {**par, "threshold": np.float32(0.0), "lookback": 1})
    y, _ = pcm_call(g, mem, xs[0], np.zeros_like(vs[0]), I16, 2, inplace=True, skip=1)
    assert_same(y[:, 1:], xs[0][:, :-1].astype(np.int16), "int16 through an open gate")
    g.close()


def check_transparency(lib, mem):
    """Threshold 0 and R = 0: the output is the input bit for bit, NaN (quiet, signalling, with payloads), inf, -0.0 and subnormals in it.
    R = 3: the input three frames late behind zeros.  A muted stream (level 0, VAD below the threshold) with NaN and inf in its input:
    every output bit pattern is +0.0."""
    S, T = 4, 5
    x = audio(3, S, T)
    odd = np.array([0x7fc00000, 0xffc00001, 0x7f800001, 0x7fa12345, 0x7f800000, 0xff800000, 0x80000000, 0x00000001, 0x807fffff, 0x00400000], np.uint32)
    x.reshape(-1)[::7][:odd.size * 20] = np.tile(odd.view(np.float32), 20)
    x[:, :, 479] = odd.view(np.float32)[3]
    v = np.random.default_rng(1).random((T, S)).astype(np.float32)
    for inplace in (False, True):
        g = gate(lib, S, 8)                                    # as created: threshold 0, R 0
        y, o = device_call(g, mem, x, v, inplace=inplace, layout="streams", skip=1)
        # (the rule's h_(-1) = level makes the first frame after a reset the ramp out of the closed state: at the level 0 an object is
        # created with, frame 0 is the restatement's ramp and every frame behind it the input; at level 1 there is no ramp at all)
        assert_same(y[:, 1:], x[:, 1:], "threshold 0, R 0")
        m = ~np.isnan(x[:, 0])                                 # (which NaN a NaN times a ramp gain is, the header leaves open)
        assert_same(y[:, 0][m], Restated(S, 8).apply(x[:, :1], v[:1])[0][:, 0][m], "threshold 0, R 0: the first frame")
        assert (o == 1).all()
        g.set_params(0.0, 0, 0, 1.0)
        y, o = device_call(g, mem, x, v, inplace=inplace, layout="streams", skip=1)
        assert_same(y, x, "threshold 0, R 0, level 1: every frame")
        g.set_params(0.0, 0, 3, 0.0)
        y, o = device_call(g, mem, x, v, inplace=inplace)
        assert_same(y[:, 3:], x[:, :2], "R 3: the delayed input"), assert_same(y[:, :3], np.zeros((S, 3, FRAME), np.float32), "R 3: the zeros in front")
        y, _ = device_call(g, mem, x, v, inplace=inplace)
        assert_same(y[:, :3], x[:, 2:], "R 3: the next call's first frames"), assert_same(y[:, 3:], x[:, :2])
        g.set_params(0.5, 0, [0, 1, 3, 8], 0.0)
        y, o = device_call(g, mem, x, np.full((T, S), 0.25, np.float32), inplace=inplace)
        assert (bits(y) == 0).all() and (o == 0).all(), "a muted stream emits +0.0"
        g.close()


def check_ramp(lib, mem):
    """Closed -> open -> closed at level 0 and at 0.1, R = 0, G = 0: the first and last sample of each ramp frame match the formula
    (written out here, apart from the restatement), the frames on either side are exact copies, exact x * level, or +0.0."""
    lv = np.array([0.0, 0.1], np.float32)
    x = audio(9, 2, 6)
    v = np.array([0, 0, 1, 1, 0, 0], np.float32)[:, None].repeat(2, axis=1)
    g = gate(lib, 2, 0, {"threshold": 0.5, "grace": 0, "lookback": 0, "level": lv})
    y, o = device_call(g, mem, x, v, layout="streams")
    assert o.T.tolist() == [[0, 0, 1, 1, 0, 0]] * 2
    one = np.float32(1.0)
    for s in range(2):
        L = lv[s]
        for i in (0, 479):
            up = L + (one - L) * RAMP[i]
            dn = one + (L - one) * RAMP[i]
            assert up.dtype == np.float32 and dn.dtype == np.float32
            for t, gi in ((2, up), (4, dn)):
                want = x[s, t, i] if gi == one else np.float32(0.0) if gi == 0 else x[s, t, i] * gi
                assert_same(y[s, t, i], np.float32(want), f"level {L} frame {t} sample {i}")
        assert_same(y[s, 3], x[s, 3], "the open frame")
        for t in (0, 1, 5):
            assert_same(y[s, t], np.zeros(FRAME, np.float32) if L == 0 else x[s, t] * L, f"closed frame {t}")
    assert RAMP[479] == one and (bits(y[0, 4, 479:]) == 0).all() and np.array_equal(bits(y[0, 2, 479:]), bits(x[0, 2, 479:]))
    rs = Restated(2, 0, {"threshold": 0.5, "grace": 0, "lookback": 0, "level": lv})
    assert_same(y, rs.apply(x, v)[0], "the whole ramp against the restatement")
    g.close()


def check_live(lib, mem, S=7, T=4):
    """Masked streams: their output and d_open bytes keep the sentinel (out of place) or the input (in place), their input and VAD may be
    NaN, their state does not move -- continuing them later equals never having made the masked calls --, and the live streams' bits are
    the unmasked call's."""
    par = params(S, 3)
    live = np.array([1, 0, 1, 1, 0, 1, 0], np.uint8)[:S]
    xs, vs = [audio(50 + c, S, T) for c in range(3)], [vad_rows(60 + c, T, par["threshold"]) for c in range(3)]
    for inplace in (False, True):
        g, full, rs = gate(lib, S, 8, par), gate(lib, S, 8, par), Restated(S, 8, par)
        device_call(g, mem, xs[0], vs[0]), device_call(full, mem, xs[0], vs[0]), rs.apply(xs[0], vs[0])
        x1, v1 = xs[1].copy(), vs[1].copy()
        x1[live == 0], v1[:, live == 0] = np.nan, np.nan
        y, o = device_call(g, mem, x1, v1, live=live, inplace=inplace)
        yf, of = device_call(full, mem, xs[1], vs[1], inplace=inplace)
        assert_same(y[live == 1], yf[live == 1], "live streams' audio"), assert_same(o[:, live == 1], of[:, live == 1], "live streams' open flags")
        assert_same(y[live == 0], x1[live == 0] if inplace else np.full_like(x1[live == 0], SENT), "masked streams' audio")
        assert (o[:, live == 0] == SENT_OPEN).all()
        wy, wo = rs.apply(x1, v1, live=live, base=x1 if inplace else None)
        assert_same(y, wy), assert_same(o, wo)
        assert_records(g, rs, "after the masked call")
        # the masked streams go on from where call 0 left them
        y, o = device_call(g, mem, xs[2], vs[2], inplace=inplace)
        ref, rr = gate(lib, S, 8, par), Restated(S, 8, par)
        device_call(ref, mem, xs[0], vs[0]), rr.apply(xs[0], vs[0])
        y2, o2 = device_call(ref, mem, xs[2], vs[2])
        assert_same(y[live == 0], y2[live == 0], "masked streams, continued"), assert_same(o[:, live == 0], o2[:, live == 0])
        assert_same(y, rs.apply(xs[2], vs[2])[0])
        for q in (g, full, ref):
            q.close()


def check_state(lib, mem, S=6, T=4):
    """Per-stream reset and set_params; a stream moved mid-run into a second object with a larger max_lookback continues bit for bit;
    import into a smaller max_lookback is refused and changes nothing."""
    import pytest
    par = params(S, 0)
    par["lookback"] = np.minimum(par["lookback"], 3)
    xs, vs = [audio(80 + c, S, T) for c in range(4)], [vad_rows(90 + c, T, par["threshold"]) for c in range(4)]
    g, rs = gate(lib, S, 3, par), Restated(S, 3, par)
    assert_same(device_call(g, mem, xs[0], vs[0])[0], rs.apply(xs[0], vs[0])[0])
    g.reset([4, 1]), rs.reset([4, 1])
    assert_records(g, rs, "after the reset")
    got = g.params()
    assert np.array_equal(got["lookback"], par["lookback"]) and np.array_equal(bits(got["threshold"]), bits(par["threshold"]))
    y, o = device_call(g, mem, xs[1], vs[1], inplace=True)
    wy, wo = rs.apply(xs[1], vs[1])
    assert_same(y, wy, "behind the reset"), assert_same(o, wo)
    new = {"threshold": np.float32(0.25), "grace": 2, "lookback": np.array([2, 0]), "level": np.float32(0.1)}
    g.set_params(new["threshold"], new["grace"], new["lookback"], new["level"], idx=[2, 0]), rs.set_params([2, 0], new)
    assert_records(g, rs, "after set_params")
    assert g.params([2, 0])["lookback"].tolist() == [2, 0] and g.params([3])["lookback"][0] == par["lookback"][3]
    y, o = device_call(g, mem, xs[2], vs[2])
    wy, wo = rs.apply(xs[2], vs[2])
    assert_same(y, wy, "behind set_params"), assert_same(o, wo)
    # streams 3 and 2 move to streams 0 and 4 of a wider object of eight streams
    src = [3, 2]
    assert rs.R[3] == 3 and rs.R[2] == 2
    rec = g.export_streams(src)
    assert_same(rec, rs.export(src), "exported records")
    big, rb = gate(lib, 8, 8, params(8, 1)), Restated(8, 8, params(8, 1))
    x8, v8 = audio(85, 8, T), vad_rows(95, T, rb.thr)
    device_call(big, mem, x8, v8), rb.apply(x8, v8)
    big.import_streams([0, 4], rec), rb.import_([0, 4], rec)
    assert_records(big, rb, "after the import")
    x8[[0, 4]], v8[:, [0, 4]] = xs[3][src], vs[3][:, src]
    y8, o8 = device_call(big, mem, x8, v8, inplace=True)
    y, o = device_call(g, mem, xs[3], vs[3])
    assert_same(y8[[0, 4]], y[src], "the moved streams continue"), assert_same(o8[:, [0, 4]], o[:, src])
    assert_same(y8, rb.apply(x8, v8)[0])
    small = gate(lib, 2, 2)
    before = small.export_streams(None)
    with pytest.raises(RuntimeError, match="lookback 3, this object's max_lookback is 2"):
        small.import_streams([1, 0], rec)
    assert_same(small.export_streams(None), before, "a refused import")
    g.reset(), rs.reset()
    assert_records(g, rs, "after the whole reset")
    for q in (g, big, small):
        q.close()


def check_host_call(lib, mem, S=5, T=3):
    """The host call (dense [S][T][480]) gives the device-style call's bits, with and without a mask and the open flags, in place too."""
    par = params(S, 1)
    live = np.array([1, 1, 0, 1, 0], np.uint8)[:S]
    a, rs = gate(lib, S, 8, par), Restated(S, 8, par)
    for call, lv in enumerate((None, live, None)):
        x, v = audio(20 + call, S, T), vad_rows(25 + call, T, par["threshold"])
        base = np.full_like(x, SENT)
        out = x.copy() if call == 2 else base.copy()
        y, o = a.apply(out if call == 2 else x, v, live=lv, out=out, want_open=True)
        wy, wo = rs.apply(x, v, live=lv)
        if lv is not None:
            wo[:, lv == 0] = 0                                  # (the Python mirror hands back zeros where nothing was written)
        assert y is out
        assert_same(y, wy, f"host call {call}"), assert_same(o, wo)
    assert a.apply(x, v).shape == x.shape
    a.close()


def check_refusals(lib, mem):
    """Every refusal of the header with its text; each leaves the object as it was: the records before and after are the same bytes and a
    following call equals the restatement's."""
    import ctypes as C
    import pytest
    from nnnoiseless_amd import _ffi
    from nnnoiseless_amd.gate import VadGate
    L = lib.L

    def refused(rc, text):
        assert rc != 0 and text in lib.error(), (rc, text, lib.error())

    for S, H, text in ((0, 0, "n_streams"), (-1, 2, "n_streams"), (4, -1, "max_lookback"), (4, 9, "max_lookback")):
        assert not L.nnn_gate_create(S, H, 0) and text in lib.error()
    with pytest.raises(RuntimeError, match=r"max_lookback = 9 outside \[0, 8\]"):
        VadGate(4, 9, lib=lib)
    L.nnn_gate_destroy(None)
    S, T = 4, 2
    par = params(S, 1)
    g, rs = gate(lib, S, 3, {**par, "lookback": np.minimum(par["lookback"], 3)}), Restated(S, 3, {**par, "lookback": np.minimum(par["lookback"], 3)})
    x, v = audio(1, S, T), vad_rows(2, T, par["threshold"])
    assert_same(device_call(g, mem, x, v)[0], rs.apply(x, v)[0])
    before = g.export_streams(None)
    hx, hv = mem.put(x.transpose(1, 0, 2)), mem.put(v)
    p, pv, h = hx.ptr, hv.ptr, g._h
    lay = _ffi.PcmLayout(F32, 1, 0, 0, FRAME, S * FRAME)
    pp = np.zeros(S, _ffi.GATE_PARAMS_DTYPE)
    rec = np.zeros((S, _ffi.GATE_STATE_BYTES), np.uint8)
    ip = (C.c_int * 2)(0, 1)
    # a NULL object
    refused(L.nnn_gate_apply_device(None, p, p, pv, None, None, T, FRAME, S * FRAME, None), "null gate")
    refused(L.nnn_gate_apply_pcm_device(None, p, p, pv, None, None, T, C.byref(lay), None), "null gate")
    refused(L.nnn_gate_apply_host(None, _ffi.ptr(x), _ffi.ptr(x), _ffi.ptr(v), None, None, T), "null gate")
    refused(L.nnn_gate_set_params(None, None, S, _ffi.ptr(pp)), "null gate")
    refused(L.nnn_gate_get_params(None, None, S, _ffi.ptr(pp)), "null gate")
    refused(L.nnn_gate_reset(None, None, 0), "null gate")
    refused(L.nnn_gate_export_streams(None, None, S, _ffi.ptr(rec), rec.nbytes), "null gate")
    refused(L.nnn_gate_import_streams(None, None, S, _ffi.ptr(rec), rec.nbytes), "null gate")
    assert L.nnn_gate_state_bytes(None) == 0 and "null gate" in lib.error()
    assert L.nnn_gate_state_bytes(h) == _ffi.GATE_STATE_BYTES == g.export_streams([0]).size
    # NULL buffers, the frame count, the strides
    for args, text in (((None, p, pv), "null input"), ((p, None, pv), "null output"), ((p, p, None), "null vad")):
        refused(L.nnn_gate_apply_device(h, *args, None, None, T, FRAME, S * FRAME, None), text)
        refused(L.nnn_gate_apply_pcm_device(h, *args, None, None, T, C.byref(lay), None), text)
    refused(L.nnn_gate_apply_host(h, None, _ffi.ptr(x), _ffi.ptr(v), None, None, T), "null input")
    refused(L.nnn_gate_apply_host(h, _ffi.ptr(x), None, _ffi.ptr(v), None, None, T), "null output")
    refused(L.nnn_gate_apply_host(h, _ffi.ptr(x), _ffi.ptr(x), None, None, None, T), "null vad")
    for n in (0, -3):
        refused(L.nnn_gate_apply_device(h, p, p, pv, None, None, n, FRAME, S * FRAME, None), f"n_frames = {n}")
        refused(L.nnn_gate_apply_pcm_device(h, p, p, pv, None, None, n, C.byref(lay), None), f"n_frames = {n}")
        refused(L.nnn_gate_apply_host(h, _ffi.ptr(x), _ffi.ptr(x), _ffi.ptr(v), None, None, n), f"n_frames = {n}")
    refused(L.nnn_gate_apply_device(h, p, p, pv, None, None, T, FRAME, FRAME - 1, None), "frame_stride = 479 is below a frame's 480")
    refused(L.nnn_gate_apply_device(h, p + 2, p, pv, None, None, T, FRAME, S * FRAME, None), "4-byte samples")
    # the packed boundary: format, channels, discard_first, layout, stride
    refused(L.nnn_gate_apply_pcm_device(h, p, p, pv, None, None, T, None, None), "null layout")
    for bad, text in ((_ffi.PcmLayout(3, 1, 0, 0, FRAME, S * FRAME), "bad format 3"), (_ffi.PcmLayout(-1, 1, 0, 0, FRAME, S * FRAME), "bad format -1"),
                      (_ffi.PcmLayout(F32, 0, 0, 0, FRAME, S * FRAME), "channels = 0"), (_ffi.PcmLayout(I16, 3, 0, 0, FRAME, S * FRAME * 3), "channels = 3"),
                      (_ffi.PcmLayout(F32, 1, 1, 0, FRAME, S * FRAME), "discard_first must be 0"),
                      (_ffi.PcmLayout(F32, 2, 0, 0, 2 * T * FRAME, 2 * FRAME - 1), "frame_stride = 959 is below a frame's 960")):
        refused(L.nnn_gate_apply_pcm_device(h, p, p, pv, None, None, T, C.byref(bad), None), text)
    refused(L.nnn_gate_apply_pcm_device(h, p + 1, p, pv, None, None, T, C.byref(_ffi.PcmLayout(I16, 1, 0, 0, FRAME, S * FRAME)), None), "2-byte samples")
    # index lists
    with pytest.raises(RuntimeError, match=r"stream 4 outside \[0, 4\)"):
        g.set_params(0.5, 0, 0, 0.0, idx=[0, 4])
    with pytest.raises(RuntimeError, match="stream -1 outside"):
        g.reset([-1])
    with pytest.raises(RuntimeError, match="stream 7 outside"):
        g.params([7])
    with pytest.raises(RuntimeError, match="stream 9 outside"):
        g.export_streams([9])
    with pytest.raises(RuntimeError, match="stream 2 is listed twice"):
        g.set_params(0.5, 0, 0, 0.0, idx=[2, 1, 2])
    with pytest.raises(RuntimeError, match="stream 1 is listed twice"):
        g.import_streams([1, 1], before[:2])
    with pytest.raises(RuntimeError, match="5 entries for 4 streams"):
        lib.check(L.nnn_gate_set_params(h, None, 5, _ffi.ptr(np.zeros(5, _ffi.GATE_PARAMS_DTYPE))))
    refused(L.nnn_gate_set_params(h, None, S, None), "null params")
    refused(L.nnn_gate_set_params(h, None, -1, _ffi.ptr(pp)), "n = -1")
    refused(L.nnn_gate_export_streams(h, ip, 2, None, 0), "null records")
    refused(L.nnn_gate_export_streams(h, ip, 2, _ffi.ptr(rec), _ffi.GATE_STATE_BYTES), "bytes for 2 records")
    refused(L.nnn_gate_import_streams(h, ip, 2, _ffi.ptr(before), _ffi.GATE_STATE_BYTES), "bytes for 2 records")
    # parameters out of range, or NaN
    for kw, text in (({"threshold": -0.1}, "threshold -0.1 outside"), ({"threshold": 1.5}, "threshold 1.5 outside"), ({"threshold": np.nan}, "threshold nan outside"),
                     ({"grace": -1}, "grace -1 outside"), ({"grace": 6001}, r"grace 6001 outside \[0, 6000\]"), ({"lookback": -1}, "lookback -1 outside"),
                     ({"lookback": 4}, r"lookback 4 outside \[0, 3\]"), ({"level": -0.5}, "level -0.5 outside"), ({"level": 1.25}, "level 1.25 outside"),
                     ({"level": np.nan}, "level nan outside")):
        a = {"threshold": 0.5, "grace": 1, "lookback": 1, "level": 0.5, **kw}
        with pytest.raises(RuntimeError, match="entry 1: " + text):
            g.set_params([0.5, a["threshold"]], [1, a["grace"]], [1, a["lookback"]], [0.5, a["level"]], idx=[3, 0])
    with pytest.raises(ValueError):
        g.set_params([0.5, 0.5, 0.5], 0, 0, 0.0, idx=[0, 1])
    with pytest.raises(ValueError):
        g.apply(x[:3], v)
    with pytest.raises(ValueError):
        g.apply(x, v[:, :3])
    # records that are none
    for field, value, text in (("magic", 5, "is not a gate record"), ("version", 2, "has version 2"), ("size", 48, "says 48 bytes"),
                               ("lookback", 9, "lookback 9 outside"), ("level", np.nan, "level nan outside"), ("since", -2, "has a state no gate reaches"),
                               ("was_open", 2, "has a state no gate reaches")):
        bad = before.copy()
        bad.view(_ffi.GATE_STATE_DTYPE).reshape(-1)[field][1] = value
        with pytest.raises(RuntimeError, match="record 1 " + text if "outside" not in text else "entry 1: " + text):
            g.import_streams(None, bad)
    # nothing of that changed the object
    assert_same(g.export_streams(None), before, "after the refusals")
    x, v = audio(3, S, T), vad_rows(4, T, par["threshold"])
    y, o = device_call(g, mem, x, v, inplace=True)
    wy, wo = rs.apply(x, v)
    assert_same(y, wy, "after the refusals"), assert_same(o, wo)
    assert L.nnn_gate_set_params(h, None, 0, None) == 0 and L.nnn_gate_reset(h, ip, 0) == 0
    assert_records(g, rs, "at the end")
    g.close()
