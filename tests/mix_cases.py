"""Shared by the conference mixer's tests (include/nnn_mix.h): a NumPy restatement of the header's rule, written
from the header -- Python loops over frames, rooms and members, float32 NumPy operations for the ramp, float64 ones for the terms and
the room's total in ascending stream index --, the calls on every layout the header allows, and the checks the interpreter tests and the
GPU tests both make.  Every comparison is of raw bits: float32 as uint32, int16, the heard counts."""
import numpy as np

from gate_cases import F32, F32_UNIT, FRAME, I16, RAMP, HostMem, TorchMem, assert_same, bits, f32_index, pcm_index, round_i16  # noqa: F401
from nnnoiseless_amd import _ffi

TILE, REG = _ffi.MIX_TILE, _ffi.MIX_REG_TALKERS
GARBAGE = np.float32(7.25e5)      # what the gaps between frames hold
SENT = np.float32(-7.5e5)         # what an output buffer holds before a call
SENT16 = np.int16(-12345)
SENT_HEARD = np.int32(-77)
GAINS = np.array([1.0, 0.5, 2.0, 1.0, 0.25, 16.0, 0.0, 1.0, 0.75], np.float32)   # (0: a talker nobody hears)


def rooms_for(S):
    """The room labels of the shapes: interleaved rooms, labels in non-ascending order, -1 and labelled rooms of one."""
    s = np.arange(S)
    r = np.full(S, -1, np.int32)
    if S == 3:                                        # a pair and a loner
        r[[0, 2]] = 2
    elif S == 12:                                     # rooms of 1, 2 and 9 (REG + 1), interleaved
        r[:] = 3
        r[[1, 7]], r[5] = 1, 0
    elif S == 45:                                     # rooms of 33 (TILE + 1) and 8 (REG), four alone
        r[:] = 40
        r[s[s % 5 == 1][:8]] = 7
        r[[4, 17, 30, 44]] = -1
    elif S == 80:                                     # one room of 70; a room of 3, one of 2, five alone
        r[:] = 9
        rest = s[s % 8 == 3]
        r[rest] = -1
        r[rest[:3]], r[rest[3:5]], r[rest[5]] = 79, 0, 4
    elif S == 38:                                     # rooms of 32 (TILE) and 3, three alone
        r[:] = 5
        r[[2, 20, 37]] = 1
        r[[0, 11, 29]] = -1
    elif S > 80:                                      # many rooms of mixed size: 1, 2, 3, 5, 9, 40 members, interleaved by a stride
        sizes, k, lab = [1, 2, 3, 5, 9, 40], 0, S - 1
        order = (s * 37) % S if np.gcd(37, S) == 1 else s
        at = 0
        while at < S:
            n = sizes[k % len(sizes)]
            r[order[at:at + n]] = lab if n > 1 or k % 2 else -1
            at, k, lab = at + n, k + 1, lab - 1
    return r


SHAPES = [(1, 1), (3, 2), (12, 3), (45, 5), (80, 2), (38, 1)]
assert sorted(set(np.bincount(rooms_for(45)[rooms_for(45) >= 0]))) == [0, REG, TILE + 1] and (rooms_for(80) == 9).sum() == 70
assert (rooms_for(38) == 5).sum() == TILE and (rooms_for(12) == 3).sum() == REG + 1


def groups(room):
    """The rooms as lists of members in ascending stream index."""
    g = {}
    for s, r in enumerate(room):
        g.setdefault(("room", int(r)) if r >= 0 else ("alone", s), []).append(s)
    return list(g.values())


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def load(raw, fmt):
    """The format's loader: what the rule calls x."""
    raw = np.asarray(raw)
    if fmt == I16:
        return raw.astype(np.float32)
    with np.errstate(all="ignore"):
        return raw.astype(np.float32) * np.float32(32768.0) if fmt == F32_UNIT else raw.astype(np.float32)


def write(y, fmt):
    """The format's writer."""
    if fmt == I16:
        return round_i16(y)
    if fmt == F32_UNIT:
        return np.clip(y / np.float32(32768.0), np.float32(-1.0), np.float32(1.0)).astype(np.float32)
    return y


class Restated:
    """The object of include/nnn_mix.h on the host."""

    def __init__(self, S, room=None, gain=None):
        self.S = S
        self.room = np.full(S, -1, np.int64) if room is None else np.array(room, np.int64)
        self.gain = np.ones(S, np.float32) if gain is None else np.array(gain, np.float32)
        self.prev = np.zeros(S, np.float32)
        self.counts = set()                          # the values A took in rooms of more than one member (for the tests' coverage asserts)

    def reset(self, idx=None):
        self.prev[np.arange(self.S) if idx is None else np.asarray(idx)] = 0

    def apply(self, x, talk=None, live=None, ofmt=F32):
        """x float32 [S, T, 480] after the loader -> (y [S, T, 480] in the output format, heard int32 [T, S]); what a stream marked 0 owns
        is the sentinels'."""
        S, T, _ = x.shape
        y = np.full(x.shape, SENT16 if ofmt == I16 else SENT)
        heard = np.full((T, S), SENT_HEARD)
        alive = np.ones(S, bool) if live is None else np.asarray(live) != 0
        zero = np.float32(0.0)
        for t in range(T):
            hn = np.where(np.ones(S, bool) if talk is None else np.asarray(talk[t]) != 0, self.gain, zero).astype(np.float32)   # step 1
            hp = self.prev
            for members in groups(self.room):
                L = [s for s in members if alive[s]]
                aud = [s for s in L if hp[s] != 0 or hn[s] != 0]                                       # step 3
                if len(members) > 1:
                    self.counts.add(len(aud))
                c = {}
                for s in aud:
                    g = np.full(FRAME, hn[s]) if hp[s] == hn[s] else hp[s] + (hn[s] - hp[s]) * RAMP    # step 2: float32, one rounding each
                    assert g.dtype == np.float32
                    with np.errstate(all="ignore"):
                        c[s] = x[s, t].astype(np.float64) * g.astype(np.float64)                      # step 4
                total = np.zeros(FRAME, np.float64)
                with np.errstate(all="ignore"):
                    for s in aud:                                                                      # step 5: ascending stream index
                        total = total + c[s]
                    for p in L:                                                                        # step 6
                        if p in c and len(aud) == 1:
                            yp = np.zeros(FRAME, np.float32)
                        elif p in c and len(aud) == 2:
                            yp = c[aud[1] if p == aud[0] else aud[0]].astype(np.float32)
                        else:
                            yp = (total - c.get(p, np.float64(0.0))).astype(np.float32)
                        y[p, t] = write(yp, ofmt)
                        heard[t, p] = len(aud) - (p in c)                                              # step 7
            self.prev = np.where(alive, hn, hp).astype(np.float32)                                     # step 8
        return y, heard


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def audio(seed, S, T, whole=False):
    """float32 [S, T, 480] uniform in a quarter of the int16 range: not whole numbers (the product with a gain rounds) unless `whole`."""
    x = np.random.default_rng(seed).uniform(-8192.0, 8191.0, (S, T, FRAME)).astype(np.float32)
    return np.round(x) if whole else x


def gains_for(S, rot=0):
    return GAINS[(np.arange(S) + rot) % GAINS.size]


def talk_rows(seed, room, T, call=0):
    """uint8 [T, S]: coin flips, and in the largest room a schedule that, with the ramp frames, walks A through 2, 3, everybody, 0 (call 0)
    and 1, 2, 1 (call 1): toggles in consecutive frames in both directions."""
    S = len(room)
    talk = (np.random.default_rng(seed).random((T, S)) < 0.5).astype(np.uint8)
    big = max(groups(room), key=len)
    if len(big) > 2:
        plan = ([big[:2], big[:3], big, [], []] if call == 0 else [big[3:4], big[3:4], big[3:5], big[4:5], []])
        for t in range(T):
            talk[t, big] = 0
            talk[t, plan[t % 5]] = 1
    return talk


def mixer(lib, S, room=None, gain=None):
    from nnnoiseless_amd.mix import ConferenceMixer
    m = ConferenceMixer(S, lib=lib)
    if room is not None:
        m.set_rooms(room)
    if gain is not None:
        m.set_gains(gain)
    return m


# ---- the calls -----------------------------------------------------------------------------------------------------------------------------
def _run(mem, call, raw, at_in, at_out, odt, talk, live, want_heard, skip):
    """Lay raw [S, T, 480] out at `at_in` in a buffer of garbage, make the call into a buffer of sentinels, return (y [S, T, 480], heard
    [T, S] or None); the input and everything outside the output's frames must come back as they were."""
    S, T, _ = raw.shape
    idt = raw.dtype
    buf = np.full(int(at_in.max()) + 1, np.int16(9999) if idt == np.int16 else GARBAGE, idt)
    buf[at_in] = raw
    sent = SENT16 if odt == np.int16 else SENT
    n = int(at_out.max()) + 1
    hin, hout = mem.put(buf, skip[0]), mem.put(np.full(n, sent, odt), skip[1])
    ht = None if talk is None else mem.put(np.ascontiguousarray(talk, dtype=np.uint8))
    hl = None if live is None else mem.put(np.ascontiguousarray(live, dtype=np.uint8))
    hh = mem.put(np.full((T, S), SENT_HEARD, np.int32)) if want_heard else None
    call(hin.ptr, hout.ptr, None if ht is None else ht.ptr, None if hl is None else hl.ptr, None if hh is None else hh.ptr)
    mem.sync()
    res = hout.get()
    outside = np.ones(n, bool)
    outside[at_out] = False
    assert (res[outside] == sent).all(), "a write outside the frames"
    assert_same(hin.get(), buf, "the input")
    return res[at_out], None if hh is None else hh.get().reshape(T, S)


def device_call(m, mem, x, talk=None, live=None, want_heard=True, skip=(0, 0), lin=None, lout=None):
    S, T, _ = x.shape
    (ai, iss, ifs), (ao, oss, ofs) = f32_index(S, T, **(lin or {})), f32_index(S, T, **(lout or {"layout": "streams"}))
    return _run(mem, lambda i, o, tk, lv, hd: m.apply_device(i, o, T, iss, ifs, oss, ofs, d_talk=tk, d_live=lv, d_heard=hd, hip_stream=mem.stream),
                x.astype(np.float32), ai, ao, np.float32, talk, live, want_heard, skip)


def pcm_call(m, mem, raw, ifmt, iC, ofmt, oC, talk=None, live=None, want_heard=True, skip=(0, 0), ipads=None, opads=None):
    S, T, _ = raw.shape
    (ai, igs, ifs), (ao, ogs, ofs) = pcm_index(S, T, iC, **(ipads or {})), pcm_index(S, T, oC, **(opads or {}))
    return _run(mem, lambda i, o, tk, lv, hd: m.apply_pcm_device(i, o, T, (ifmt, iC, igs, ifs), (ofmt, oC, ogs, ofs), d_talk=tk, d_live=lv, d_heard=hd,
                                                                 hip_stream=mem.stream),
                raw.astype(np.int16 if ifmt == I16 else np.float32), ai, ao, np.int16 if ofmt == I16 else np.float32, talk, live, want_heard, skip)


# ---- the checks ----------------------------------------------------------------------------------------------------------------------------
def check_restatement(lib, mem, S, T):
    """Three calls of T frames under mixed gains and talk masks: the second reads the prev the first left, the third comes behind a
    set_gains of some streams.  Audio and heard equal the restatement; in the 45 x 5 shape A takes 0, 1, 2, 3 and more than REG."""
    room, gain = rooms_for(S), gains_for(S)
    m, rs = mixer(lib, S, room, gain), Restated(S, room, gain)
    counts = set()
    for call in range(3):
        if call == 2:
            idx = np.arange(0, S, 2)[::-1]
            new = gains_for(idx.size, 3)
            m.set_gains(new, idx=idx)
            rs.gain[idx] = new
        x, talk = audio(100 * S + 10 * T + call, S, T), talk_rows(7 * S + T + call, room, T, call % 2)
        talk = None if (S == 3 and call == 1) else talk
        y, h = device_call(m, mem, x, talk, lin={"layout": "frames"} if call else None)
        wy, wh = rs.apply(x, talk)
        assert_same(y, wy, f"call {call} audio"), assert_same(h, wh, f"call {call} heard")
        counts |= rs.counts
    if (S, T) == (45, 5):
        assert {0, 1, 2, 3} <= counts and max(counts) > REG, counts
    m.close()


def check_chunking(lib, mem, S=12, T=11):
    """Eleven frames as one call, as eleven calls of one frame, as 3 + 8 and as 5 + 5 + 1: the same audio and heard counts."""
    room, gain = rooms_for(S), gains_for(S, 1)
    x, talk = audio(77, S, T), talk_rows(78, room, T)
    wy, wh = Restated(S, room, gain).apply(x, talk)
    assert len(set(wh.reshape(-1).tolist())) > 3
    for cuts in ([11], [1] * 11, [3, 8], [5, 5, 1]):
        m, ys, hs, t = mixer(lib, S, room, gain), [], [], 0
        for k, n in enumerate(cuts):
            y, h = device_call(m, mem, x[:, t:t + n], talk[t:t + n], lin={"layout": "streams" if k & 1 else "frames"})
            ys.append(y), hs.append(h)
            t += n
        assert_same(np.concatenate(ys, axis=1), wy, f"cuts {cuts} audio"), assert_same(np.concatenate(hs), wh, f"cuts {cuts} heard")
        m.close()


def check_layout(lib, mem, S=6, T=2):
    """Padded strides, both orders of streams and frames, each side's base at every 4-byte offset of a 16-byte line; the packed boundary:
    all 3 x 3 format pairs at one and two channels with padding and odd int16 bases; a room loud enough to saturate the int16 writer and
    the unit writer's clamp."""
    room = np.array([4, 0, 4, 0, 4, -1], np.int32)
    gain = np.array([1.0, 2.0, 0.5, 1.0, 1.0, 1.0], np.float32)
    xs, talks = [audio(5 + c, S, T, whole=True) for c in range(2)], [talk_rows(15 + c, room, T, c) for c in range(2)]

    def want(ifmt, ofmt, raws):
        rs = Restated(S, room, gain)
        return [rs.apply(load(raws[c], ifmt), talks[c], ofmt=ofmt) for c in range(2)]

    wf = want(F32, F32, xs)
    for lin, lout, skip in (({"layout": "frames"}, {"layout": "frames"}, (0, 0)), ({"layout": "streams", "stream_pad": 8}, {"layout": "frames", "frame_pad": 2}, (0, 0)),
                            ({"layout": "frames", "stream_pad": 1}, {"layout": "streams", "frame_pad": 1}, (0, 0)),
                            ({"layout": "streams", "frame_pad": 4}, {"layout": "streams"}, (1, 0)), ({"layout": "frames"}, {"layout": "frames"}, (2, 1)),
                            ({"layout": "frames"}, {"layout": "streams", "frame_pad": 4}, (3, 2)), ({"layout": "streams"}, {"layout": "frames"}, (0, 3)),
                            ({"layout": "streams", "frame_pad": 3, "stream_pad": 5}, {"layout": "frames", "frame_pad": 1, "stream_pad": 2}, (1, 1))):
        m = mixer(lib, S, room, gain)
        for c in range(2):
            y, h = device_call(m, mem, xs[c], talks[c], lin=lin, lout=lout, skip=skip)
            assert_same(y, wf[c][0], f"{lin} {lout} {skip} call {c}"), assert_same(h, wf[c][1])
        m.close()
    unit = [(x / np.float32(32768.0)).astype(np.float32) for x in xs]
    for ifmt in (F32, I16, F32_UNIT):
        raws = unit if ifmt == F32_UNIT else xs
        for ofmt in (F32, I16, F32_UNIT):
            w = want(ifmt, ofmt, raws)
            for iC, oC, ipads, opads, skip in ((1, 1, {}, {}, (0, 0)), (2, 1, {"frame_pad": 5, "group_pad": 3}, {"frame_pad": 4}, (1, 3 if ofmt == I16 else 2)),
                                               (1, 2, {"frame_pad": 4}, {"frame_pad": 3, "group_pad": 1}, (3 if ifmt == I16 else 1, 0)), (2, 2, {}, {}, (2, 1))):
                m = mixer(lib, S, room, gain)
                for c in range(2):
                    y, h = pcm_call(m, mem, raws[c], ifmt, iC, ofmt, oC, talks[c], skip=skip, ipads=ipads, opads=opads)
                    assert_same(y, w[c][0], f"formats {ifmt} -> {ofmt} channels {iC} -> {oC} call {c}"), assert_same(h, w[c][1])
                m.close()
    # a loud room: four talkers near full scale at gain 16 saturate both clamping writers
    loud = np.clip(audio(9, S, T, whole=True) * 4, -32768, 32767).astype(np.float32)
    m = mixer(lib, S, np.zeros(S, np.int32), np.full(S, 16.0, np.float32))
    for ofmt, lo, hi in ((I16, -32768, 32767), (F32_UNIT, -1.0, 1.0)):
        m.reset()
        y, _ = pcm_call(m, mem, loud, I16, 1, ofmt, 1)
        wy, _ = Restated(S, np.zeros(S), np.full(S, 16.0)).apply(load(loud, I16), ofmt=ofmt)
        assert_same(y, wy, f"clamp of format {ofmt}")
        assert (y[:, 1] == lo).any() and (y[:, 1] == hi).any() and y.min() == lo and y.max() == hi
    m.close()


def check_live(lib, mem, S=12, T=3):
    """Masked streams are no members for the call: their output rows and heard entries keep the sentinel, their inputs and talk entries
    may be anything, their prev is frozen -- continuing them later equals never having made the masked call --, and the others' bits
    are those of a room without them."""
    room, gain = rooms_for(S), gains_for(S, 2)
    live = (np.arange(S) % 3 != 1).astype(np.uint8)
    xs, talks = [audio(50 + c, S, T) for c in range(3)], [talk_rows(60 + c, room, T, c % 2) for c in range(3)]
    m, rs = mixer(lib, S, room, gain), Restated(S, room, gain)
    y, h = device_call(m, mem, xs[0], talks[0])
    assert_same(y, rs.apply(xs[0], talks[0])[0])
    x1, t1 = xs[1].copy(), talks[1].copy()
    x1[live == 0], t1[:, live == 0] = np.nan, 1
    y, h = device_call(m, mem, x1, t1, live=live)
    wy, wh = rs.apply(x1, t1, live=live)
    assert_same(y, wy, "the masked call"), assert_same(h, wh)
    assert (y[live == 0] == SENT).all() and (h[:, live == 0] == SENT_HEARD).all() and np.isfinite(y[live == 1]).all()
    # the same bits as a mixer in which the masked streams sit alone and silent
    other = mixer(lib, S, np.where(live == 0, -1, room).astype(np.int32), gain)
    device_call(other, mem, xs[0], talks[0])
    x2 = np.where((live == 0)[:, None, None], np.float32(0), xs[1])
    y2, h2 = device_call(other, mem, x2, talks[1])
    assert_same(y[live == 1], y2[live == 1], "live streams against a room without the others"), assert_same(h[:, live == 1], h2[:, live == 1])
    # prev was frozen: the third call continues the masked streams from call 0
    y, h = device_call(m, mem, xs[2], talks[2])
    wy, wh = rs.apply(xs[2], talks[2])
    assert_same(y, wy, "behind the masked call"), assert_same(h, wh)
    assert (rs.prev[live == 0] != 0).any()
    m.close(), other.close()


def check_inaudible_nan(lib, mem, S=12, T=3):
    """NaN in every inaudible stream-frame's input (talk 0 after a silent frame, or gain 0) does not reach any output."""
    room, gain = rooms_for(S), gains_for(S)
    x, talk = audio(33, S, T), talk_rows(34, room, T)
    rs = Restated(S, room, gain)
    wy, wh = rs.apply(x, talk)
    h = np.where(talk != 0, gain, 0).astype(np.float32)
    aud = (h != 0) | (np.concatenate([np.zeros((1, S), np.float32), h[:-1]]) != 0)         # [T, S]
    assert (~aud).sum() > 3 and aud.sum() > 3
    xn = x.copy()
    xn[~aud.T] = np.nan
    m = mixer(lib, S, room, gain)
    y, hd = device_call(m, mem, xn, talk)
    assert_same(y, wy, "NaN in the inaudible inputs"), assert_same(hd, wh)
    m.close()


def check_consequences(lib, mem):
    """What the header says follows from the rule, each checked against numbers made here and not by the restatement."""
    S, T = 10, 3
    room = np.array([6, 6, 6, 6, 2, 2, -1, 6, 6, 0], np.int32)           # a room of six, a pair, a loner, a labelled room of one
    six, pair = [0, 1, 2, 3, 7, 8], [4, 5]
    x = audio(3, S, T, whole=True)
    odd = np.array([0x80000000, 0x00000001, 0x807fffff, 0x7f7fffff, 0x3f800001], np.uint32).view(np.float32)
    x.reshape(-1)[::97][:odd.size * 20] = np.tile(odd, 20)
    m = mixer(lib, S, room)
    # a lone talker and a lone audible talker receive +0.0; one steady talker at gain 1: everybody else gets its bits (-0.0 -> +0.0)
    talk = np.zeros((T, S), np.uint8)
    talk[:, [2, 6, 9]] = 1
    device_call(m, mem, x, talk)                                        # (the fade-in)
    y, h = device_call(m, mem, x, talk)
    assert (bits(y[[2, 6, 9]]) == 0).all() and (bits(y[pair]) == 0).all()
    thru = np.where(bits(x[2]) == 0x80000000, np.uint32(0), bits(x[2]))
    for p in (0, 1, 3, 7, 8):
        assert np.array_equal(bits(y[p]), thru), p
    assert h[:, 2].tolist() == [0] * T and h[:, 0].tolist() == [1] * T and h[:, 4].tolist() == [0] * T
    # A == 2, steady, gain 1: each side gets the other's bits; a listener gets the correctly rounded sum
    talk[:, [7, 4, 5]] = 1
    device_call(m, mem, x, talk)
    y, h = device_call(m, mem, x, talk)
    assert_same(y[2], x[7], "A == 2"), assert_same(y[7], x[2], "A == 2")     # (no sum is formed: -0.0 stays -0.0 here)
    assert_same(y[4], x[5], "a pair"), assert_same(y[5], x[4], "a pair")
    assert (bits(x[[2, 7, 4, 5]]) == 0x80000000).any()
    assert_same(y[0], (x[2].astype(np.float64) + x[7].astype(np.float64)).astype(np.float32))
    assert h[0].tolist() == [2, 2, 1, 2, 1, 1, 0, 1, 2, 0]
    m.close()
    # int16 samples, steady gain 1, a room of 40: the output is the exact integer sum of the others (int64), correctly rounded to int16's range
    S = 40
    xi = np.random.default_rng(8).integers(-32768, 32768, (S, T, FRAME)).astype(np.int16)
    m = mixer(lib, S, np.full(S, 11, np.int32))
    pcm_call(m, mem, xi, I16, 1, F32, 1)
    y, _ = pcm_call(m, mem, xi, I16, 1, F32, 1)                           # steady frames only
    others = xi.astype(np.int64).sum(axis=0)[None] - xi.astype(np.int64)
    assert np.abs(others).max() < 2 ** 24
    assert_same(y, others.astype(np.float32), "the exact integer sum of the others")
    # relabelling the rooms leaves the bits unchanged
    S, T = 12, 3
    room, gain = rooms_for(S), gains_for(S)
    x, talk = audio(21, S, T), talk_rows(22, room, T)
    a = mixer(lib, S, room, gain)
    relabel = {3: 0, 1: 11, 0: 5, -1: -1}
    b = mixer(lib, S, np.array([relabel[int(r)] for r in room], np.int32), gain)
    ya, ha = device_call(a, mem, x, talk)
    yb, hb = device_call(b, mem, x, talk)
    assert_same(ya, yb, "relabelled rooms"), assert_same(ha, hb)
    m.close(), a.close(), b.close()


def check_nonfinite(lib, mem):
    """A non-finite audible sample is non-finite for the other members of its room at that sample and touches nothing else: in a room
    with three talkers and a listener, in a two-party room (the other side gets the very bits), and beside a lone talker, who itself
    gets +0.0 whatever it says -- the header's `A == 1` case, which only such a sample tells from T - c_p."""
    S, T = 10, 2
    room = np.array([3, 3, 3, 3, 1, 1, 0, 0, 0, -1], np.int32)            # 0 1 2 talk to 3; 4 and 5 to each other; 6 to 7 and 8; 9 alone
    talk = np.tile(np.array([1, 1, 1, 0, 1, 1, 1, 0, 0, 1], np.uint8), (T, 1))
    clean = audio(91, S, T)
    x = clean.copy()
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    x[0, :, 5], x[1, :, 7], x[4, :, 9], x[6, :, 11], x[6, :, 13], x[9, :, 15] = inf, nan, -inf, nan, inf, nan
    hit = np.zeros((S, FRAME), bool)                                      # (listener or fellow talker, sample) that must turn non-finite
    hit[np.ix_([0, 1, 2, 3], [5, 7])] = True
    hit[5, 9] = hit[np.ix_([7, 8], [11, 13])] = True
    m, ref = mixer(lib, S, room), mixer(lib, S, room)
    device_call(m, mem, x, talk), device_call(ref, mem, clean, talk)      # (the fade-in; the frames below are steady)
    y, h = device_call(m, mem, x, talk)
    yc, hc = device_call(ref, mem, clean, talk)
    for t in range(T):
        assert not np.isfinite(y[:, t][hit]).any(), "a non-finite audible sample reaches its room"
        assert_same(y[:, t][~hit], yc[:, t][~hit], "everything else is untouched")
    assert_same(y[5, :, 9], np.full(T, -inf), "a two-party call hands over the very sample")
    assert np.isposinf(y[[7, 8]][:, :, 13]).all() and np.isnan(y[[7, 8]][:, :, 11]).all() and np.isposinf(y[[2, 3]][:, :, 5]).all()
    assert (bits(y[[6, 9]]) == 0).all(), "a lone talker gets +0.0 whatever it says"
    assert_same(h, hc), assert_same(y[4], clean[5])
    wy, wh = Restated(S, room).apply(x, talk)                             # (prev 0: its frame 0 is a fade-in, its frame 1 steady)
    fin = np.isfinite(wy[:, 1])
    assert np.array_equal(fin, np.isfinite(y[:, 1])) and np.array_equal(fin, ~hit)
    assert_same(y[:, 1][fin], wy[:, 1][fin], "the restatement where it is finite")
    # the one live member of a larger room, saying nothing but NaN: +0.0, nobody heard, the masked rows and the other rooms as before
    live = np.ones(S, np.uint8)
    live[[1, 2, 3]] = 0
    x[0] = nan
    y, h = device_call(m, mem, x, talk, live=live)
    assert (bits(y[0]) == 0).all() and (h[:, 0] == 0).all() and (y[[1, 2, 3]] == SENT).all() and (h[:, [1, 2, 3]] == SENT_HEARD).all()
    for t in range(T):
        assert_same(y[4:, t][~hit[4:]], yc[4:, t][~hit[4:]], "the other rooms beside a room of one live member")
    m.close(), ref.close()


def check_n_streams(lib, mem, T=3):
    """The bits do not depend on n_streams: a room of four alone in an object of four against the same room spread over an object of
    twelve whose other streams talk in rooms of their own."""
    at = [2, 5, 6, 11]
    gain, x, talk = gains_for(4, 1), audio(55, 4, T), talk_rows(56, np.zeros(4, np.int32), T)
    small = mixer(lib, 4, np.zeros(4, np.int32), gain)
    room = np.array([4, 4, 7, 4, -1, 7, 7, 0, 0, 4, 0, 7], np.int32)
    g12, x12, t12 = gains_for(12, 2), audio(57, 12, T), talk_rows(58, room, T)
    g12[at], x12[at], t12[:, at] = gain, x, talk
    big = mixer(lib, 12, room, g12)
    for call in range(2):
        ys, hs = device_call(small, mem, x, talk)
        yb, hb = device_call(big, mem, x12, t12, lin={"layout": "frames"})
        assert_same(yb[at], ys, f"call {call}: the room inside a larger object"), assert_same(hb[:, at], hs)
    assert (hs > 0).any() and (ys != 0).any()
    small.close(), big.close()


def check_state(lib, mem, S=12, T=2):
    """reset zeroes prev of the listed streams only; set_rooms and set_gains take effect at the next call's first frame and read back."""
    room, gain = rooms_for(S), gains_for(S)
    m, rs = mixer(lib, S, room, gain), Restated(S, room, gain)
    xs = [audio(80 + c, S, T) for c in range(4)]
    assert_same(device_call(m, mem, xs[0])[0], rs.apply(xs[0])[0])
    m.reset([4, 1]), rs.reset([4, 1])
    y, h = device_call(m, mem, xs[1])
    wy, wh = rs.apply(xs[1])
    assert_same(y, wy, "behind the reset"), assert_same(h, wh)
    assert not np.array_equal(wy[:, 0], Restated(S, room, gain).apply(xs[1])[0][:, 0])
    m.set_rooms([1, -1, 3], idx=[0, 7, 5])
    m.set_gains(np.float32(0.125), idx=[2])
    rs.room[[0, 7, 5]], rs.gain[2] = [1, -1, 3], 0.125
    assert m.rooms().tolist() == rs.room.tolist() and m.rooms([7, 0]).tolist() == [-1, 1]
    assert_same(m.gains(), rs.gain) and m.gains([2])[0] == 0.125
    y, h = device_call(m, mem, xs[2])
    wy, wh = rs.apply(xs[2])
    assert_same(y, wy, "behind the setters"), assert_same(h, wh)
    m.reset(), rs.reset()
    y, h = device_call(m, mem, xs[3])
    assert_same(y, rs.apply(xs[3])[0], "behind the whole reset")
    assert_same(y, Restated(S, rs.room, rs.gain).apply(xs[3])[0], "a reset object is a new one")
    m.close()


def check_host_call(lib, mem, S=12, T=3):
    """The host call (dense [S][T][480]) gives the device-style call's bits, with and without masks; masked rows are left as they were."""
    room, gain = rooms_for(S), gains_for(S, 1)
    live = (np.arange(S) % 4 != 2).astype(np.uint8)
    m, rs = mixer(lib, S, room, gain), Restated(S, room, gain)
    for call, (lv, tk) in enumerate(((None, True), (live, True), (None, False))):
        x = audio(20 + call, S, T)
        talk = talk_rows(25 + call, room, T, call % 2) if tk else None
        out = np.full_like(x, SENT)
        y, h = m.apply(x, talk=talk, live=lv, out=out, want_heard=True)
        wy, wh = rs.apply(x, talk, live=lv)
        if lv is not None:
            wh[:, lv == 0] = 0                                  # (the Python mirror hands back zeros where nothing was written)
        assert y is out
        assert_same(y, wy, f"host call {call}"), assert_same(h, wh)
    assert m.apply(x).shape == x.shape
    m.close()


def check_refusals(lib, mem):
    """Every refusal of the header with its text; each leaves the object as it was: rooms and gains read back unchanged and a following
    call equals the restatement's (so prev did not move either)."""
    import ctypes as C
    import pytest
    from nnnoiseless_amd.mix import ConferenceMixer
    L = lib.L

    def refused(rc, text):
        assert rc != 0 and text in lib.error(), (rc, text, lib.error())

    for S in (0, -1):
        assert not L.nnn_mix_create(S, 0) and "n_streams" in lib.error()
    with pytest.raises(RuntimeError, match="n_streams = 0"):
        ConferenceMixer(0, lib=lib)
    L.nnn_mix_destroy(None)
    S, T = 4, 2
    room, gain = np.array([1, 1, -1, 1], np.int32), np.array([1.0, 0.5, 1.0, 2.0], np.float32)
    m, rs = mixer(lib, S, room, gain), Restated(S, room, gain)
    x = audio(1, S, T)
    assert_same(device_call(m, mem, x)[0], rs.apply(x)[0])
    hx, ho = mem.put(x.transpose(1, 0, 2)), mem.put(np.zeros(x.size, np.float32))
    p, q, h = hx.ptr, ho.ptr, m._h
    lay = _ffi.PcmLayout(F32, 1, 0, 0, FRAME, S * FRAME)
    bl = C.byref(lay)
    ri, gf = np.zeros(S, np.int32), np.ones(S, np.float32)
    # a NULL object
    refused(L.nnn_mix_apply_device(None, p, q, None, None, None, T, FRAME, S * FRAME, FRAME, S * FRAME, None), "null mixer")
    refused(L.nnn_mix_apply_pcm_device(None, p, q, None, None, None, T, bl, bl, None), "null mixer")
    refused(L.nnn_mix_apply_host(None, _ffi.ptr(x), _ffi.ptr(x), None, None, None, T), "null mixer")
    refused(L.nnn_mix_set_rooms(None, None, S, _ffi.ptr(ri)), "null mixer"), refused(L.nnn_mix_get_rooms(None, None, S, _ffi.ptr(ri)), "null mixer")
    refused(L.nnn_mix_set_gains(None, None, S, _ffi.ptr(gf)), "null mixer"), refused(L.nnn_mix_get_gains(None, None, S, _ffi.ptr(gf)), "null mixer")
    refused(L.nnn_mix_reset(None, None, 0), "null mixer")
    # NULL buffers, the frame count, overlap, strides, alignment
    for args, text in (((None, q), "null input"), ((p, None), "null output")):
        refused(L.nnn_mix_apply_device(h, *args, None, None, None, T, FRAME, S * FRAME, FRAME, S * FRAME, None), text)
        refused(L.nnn_mix_apply_pcm_device(h, *args, None, None, None, T, bl, bl, None), text)
    for n in (0, -3):
        refused(L.nnn_mix_apply_device(h, p, q, None, None, None, n, FRAME, S * FRAME, FRAME, S * FRAME, None), f"n_frames = {n}")
        refused(L.nnn_mix_apply_pcm_device(h, p, q, None, None, None, n, bl, bl, None), f"n_frames = {n}")
        refused(L.nnn_mix_apply_host(h, _ffi.ptr(x), _ffi.ptr(np.zeros_like(x)), None, None, None, n), f"n_frames = {n}")
    refused(L.nnn_mix_apply_device(h, p, p, None, None, None, T, FRAME, S * FRAME, FRAME, S * FRAME, None), "the output overlaps the input")
    refused(L.nnn_mix_apply_pcm_device(h, p, p, None, None, None, T, bl, bl, None), "the output overlaps the input")
    refused(L.nnn_mix_apply_host(h, _ffi.ptr(x), _ffi.ptr(x), None, None, None, T), "the output overlaps the input")
    refused(L.nnn_mix_apply_device(h, p, q, None, None, None, T, FRAME, FRAME - 1, FRAME, S * FRAME, None), "input frame_stride = 479 is below a frame's 480")
    refused(L.nnn_mix_apply_device(h, p, q, None, None, None, T, FRAME, S * FRAME, FRAME, FRAME - 1, None), "output frame_stride = 479 is below a frame's 480")
    refused(L.nnn_mix_apply_device(h, p + 2, q, None, None, None, T, FRAME, S * FRAME, FRAME, S * FRAME, None), "4-byte samples")
    # the packed boundary: format, channels, discard_first, layout, stride -- on either side
    refused(L.nnn_mix_apply_pcm_device(h, p, q, None, None, None, T, None, bl, None), "null input layout")
    refused(L.nnn_mix_apply_pcm_device(h, p, q, None, None, None, T, bl, None, None), "null output layout")
    for bad, text in ((_ffi.PcmLayout(3, 1, 0, 0, FRAME, S * FRAME), "format 3"), (_ffi.PcmLayout(-1, 1, 0, 0, FRAME, S * FRAME), "format -1"),
                      (_ffi.PcmLayout(F32, 0, 0, 0, FRAME, S * FRAME), "channels = 0"), (_ffi.PcmLayout(I16, 3, 0, 0, FRAME, S * FRAME * 3), "channels = 3"),
                      (_ffi.PcmLayout(F32, 1, 1, 0, FRAME, S * FRAME), "discard_first must be 0"),
                      (_ffi.PcmLayout(F32, 2, 0, 0, 2 * T * FRAME, 2 * FRAME - 1), "frame_stride = 959 is below a frame's 960")):
        refused(L.nnn_mix_apply_pcm_device(h, p, q, None, None, None, T, C.byref(bad), bl, None), text)
        refused(L.nnn_mix_apply_pcm_device(h, p, q, None, None, None, T, bl, C.byref(bad), None), text)
    i16 = _ffi.PcmLayout(I16, 1, 0, 0, FRAME, S * FRAME)
    refused(L.nnn_mix_apply_pcm_device(h, p + 1, q, None, None, None, T, C.byref(i16), bl, None), "2-byte samples")
    refused(L.nnn_mix_apply_pcm_device(h, p, q + 1, None, None, None, T, bl, C.byref(i16), None), "2-byte samples")
    # index lists, rooms and gains
    with pytest.raises(RuntimeError, match=r"stream 4 outside \[0, 4\)"):
        m.set_rooms(0, idx=[0, 4])
    with pytest.raises(RuntimeError, match="stream -1 outside"):
        m.reset([-1])
    with pytest.raises(RuntimeError, match="stream 7 outside"):
        m.gains([7])
    with pytest.raises(RuntimeError, match="stream 2 is listed twice"):
        m.set_rooms(0, idx=[2, 1, 2])
    with pytest.raises(RuntimeError, match="stream 1 is listed twice"):
        m.set_gains(0.5, idx=[1, 1])
    with pytest.raises(RuntimeError, match="5 entries for 4 streams"):
        lib.check(L.nnn_mix_set_gains(h, None, 5, _ffi.ptr(np.ones(5, np.float32))))
    refused(L.nnn_mix_set_rooms(h, None, S, None), "null rooms"), refused(L.nnn_mix_set_gains(h, None, S, None), "null gains")
    refused(L.nnn_mix_set_rooms(h, None, -1, _ffi.ptr(ri)), "n = -1")
    for bad, text in ((-2, r"room -2 outside \[-1, 4\)"), (4, "room 4 outside")):
        with pytest.raises(RuntimeError, match="entry 1: " + text):
            m.set_rooms([0, bad], idx=[3, 0])
    for bad, text in ((-0.5, "gain -0.5 outside"), (16.5, r"gain 16.5 outside \[0, 16\]"), (np.nan, "gain nan outside"), (np.inf, "gain inf outside")):
        with pytest.raises(RuntimeError, match="entry 1: " + text):
            m.set_gains([0.5, bad], idx=[3, 0])
    with pytest.raises(ValueError):
        m.set_gains([0.5, 0.5, 0.5], idx=[0, 1])
    with pytest.raises(ValueError):
        m.apply(x[:3])
    with pytest.raises(ValueError):
        m.apply(x, talk=np.ones((T, 3)))
    # nothing of that changed the object
    assert m.rooms().tolist() == room.tolist() and np.array_equal(bits(m.gains()), bits(gain))
    x = audio(3, S, T)
    talk = np.array([[1, 0, 1, 1], [0, 0, 1, 1]], np.uint8)
    y, hd = device_call(m, mem, x, talk)
    wy, wh = rs.apply(x, talk)
    assert_same(y, wy, "after the refusals"), assert_same(hd, wh)
    assert L.nnn_mix_set_rooms(h, None, 0, None) == 0 and L.nnn_mix_reset(h, (C.c_int * 1)(0), 0) == 0
    m.close()
