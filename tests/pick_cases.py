"""Shared by the talker picker's tests (include/nnn_pick.h): a NumPy restatement of the header's rule, written from
the header -- Python loops over frames, rooms and members, float64 scalars for the level, the scorer's summation order for a frame's
energy, a Python tuple sort for the ranking --, the calls on every layout the header allows, and the checks the interpreter tests and the
GPU tests both make.  Every comparison is of raw bits: the talk bytes, the dominant indices, float64 levels as uint64."""
import itertools

import numpy as np

from gate_cases import F32, F32_UNIT, FRAME, I16, HostMem, TorchMem, f32_index, pcm_index  # noqa: F401
from nnnoiseless_amd import _ffi
from score_cases import reduce480

SEG, WAVE = _ffi.PICK_SEG_ROOM, _ffi.PICK_WAVE_ROOM
GARBAGE = np.float32(7.25e5)      # what the gaps between frames hold
SENT_TALK = np.uint8(0xEE)        # what the output rows hold before a call
SENT_DOM = np.int32(-77)
SENT_LEVEL = np.float64(-7.5e5)
PAD = 24                          # sentinels in front of and behind every output's [T][S]
DBL_MAX = np.finfo(np.float64).max
SHAPES = [(1, 1), (3, 2), (12, 3), (80, 5), (300, 4)]
POLICIES = list(itertools.product((1, 3, 8), (0.0, 0.875, 1.0), (1.0, 4.0)))
EVENTS = {"takeover", "held_off", "tie", "none", "exactly_k", "more_than_k", "pin_over_louder"}


def same(got, want, tag=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    u = {8: np.uint64, 4: np.uint32, 2: np.uint16, 1: np.uint8}[got.dtype.itemsize]
    g, w = got.view(u), want.view(u)
    assert np.array_equal(g, w), (tag, int((g != w).sum()), np.argwhere(g != w)[:4].tolist())


def next_policy(k, decay, stick):
    """What the third call of a restatement case switches to: every value another one of the issue's lists."""
    return {1: 3, 3: 8, 8: 1}[k], {0.0: 0.875, 0.875: 1.0, 1.0: 0.0}[decay], {1.0: 4.0, 4.0: 1.0}[stick]


def rooms_for(S, k=3):
    """(labels, the room of identical twins, the room the open schedule walks through 'all, exactly k, none', the pinned streams).
    Interleaved rooms, labels in non-ascending order, -1 and labelled rooms of one; the sizes cross every class bound of the header
    (1 | 2 .. SEG | SEG + 1 .. WAVE | beyond) and k | k + 1."""
    s = np.arange(S)
    r = np.full(S, -1, np.int32)
    twins, sched, pins = [], [], []
    if S == 3:                                        # a pair and a loner
        r[[0, 2]] = 2
        twins = [0, 2]
    elif S == 12:                                     # rooms of 9, 2 and 1, interleaved
        r[:] = 3
        r[[1, 7]], r[5] = 1, 0
        twins, pins = [1, 7], [4]
        sched = s[r == 3].tolist()
    elif S == 80:                                     # a room of 63, one of k + 1 (the twins), one of 2, a labelled room of one, the rest alone
        order = (s * 37) % S
        r[order[:63]] = 70
        r[order[63:64 + k]] = 9
        r[order[64 + k:66 + k]] = 0
        r[order[66 + k]] = 4
        twins, sched = np.sort(order[63:64 + k]).tolist(), np.sort(order[63:64 + k]).tolist()
        pins = np.sort(order[:63])[[5, 40]].tolist()
    elif S == 300:                                    # rooms of 130, 65, 64, 9 (the twins), k, k + 1, 2, a labelled room of one, the duel's
        order = (s * 37) % S                          # (duel_for), the rest alone
        at, lab = 0, S - 1
        for n in (130, 65, 64, 9, k, k + 1, 2, 1, len(duel_for(S, k))):
            r[order[at:at + n]] = lab
            if n == 9 and not twins:
                twins = np.sort(order[at:at + n]).tolist()
            elif n == k and not sched:
                sched = np.sort(order[at:at + n]).tolist()
            at, lab = at + n, lab - 3
        pins = np.sort(order[:130])[[3, 77]].tolist() + np.sort(order[130:195])[[10]].tolist()
    return r, twins, sched, pins


def duel_for(S, k):
    """The members of the 300 shape's last room, two more than the larger k of a restatement case's policies, whose amplitudes audio()
    scripts: in every call the first `loud` (the k in force) loud enough to take the room whatever went before; then one challenger 2.25
    times an incumbent's energy -- inside a stick of 4, beyond one of 1 --; then another one 25 times it."""
    if S != 300:
        return []
    at = 130 + 65 + 64 + 9 + k + k + 1 + 2 + 1
    return np.sort(((np.arange(S) * 37) % S)[at:at + max(k, next_policy(k, 0.0, 1.0)[0]) + 2]).tolist()


def groups(room):
    """The rooms as lists of members in ascending stream index."""
    g = {}
    for s, r in enumerate(room):
        g.setdefault(("room", int(r)) if r >= 0 else ("alone", s), []).append(s)
    return list(g.values())


assert {len(g) for g in groups(rooms_for(300, 3)[0])} >= {1, 2, 3, 4, 9, 64, 65, 130} and {len(g) for g in groups(rooms_for(80, 8)[0])} >= {1, 2, 9, 63}
assert SEG == 8 and WAVE == 64, "the shapes above were placed for these class bounds: 2, 8 | 9, 63, 64 | 65, 130"


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def load(raw, fmt):
    """The format's loader: what the rule calls x."""
    raw = np.asarray(raw)
    with np.errstate(all="ignore"):
        return raw.astype(np.float32) * np.float32(32768.0) if fmt == F32_UNIT else raw.astype(np.float32)


def energy(x):
    """Step 1 for open stream-frames: float32 [..., 480] -> float64 [...]."""
    with np.errstate(all="ignore"):
        xd = x.astype(np.float64)
        e = reduce480(xd * xd)
        return np.where(e <= DBL_MAX, e, np.float64(0.0))


def u64(v):
    return int(np.float64(v).view(np.uint64))


class Restated:
    """The object of include/nnn_pick.h on the host."""

    def __init__(self, S, room=None, pinned=None, k=3, decay=0.875, stick=4.0):
        self.S = S
        self.room = np.full(S, -1, np.int64) if room is None else np.array(room, np.int64)
        self.pinned = np.zeros(S, np.int64) if pinned is None else np.array(pinned, np.int64)
        self.set_policy(k, decay, stick)
        self.level, self.sel = np.zeros(S, np.float64), np.zeros(S, np.int64)
        self.events = set()                          # what the room-frames so far showed (for the tests' coverage asserts)

    def set_policy(self, k, decay, stick):
        self.k, self.decay, self.stick = int(k), np.float64(np.float32(decay)), np.float64(np.float32(stick))

    def reset(self, idx=None):
        idx = np.arange(self.S) if idx is None else np.asarray(idx)
        self.level[idx], self.sel[idx] = 0.0, 0

    def select(self, x, opn=None, live=None):
        """x float32 [S, T, 480] after the loader -> (talk uint8 [T, S], dominant int32 [T, S], level float64 [T, S]); what a stream marked
        0 owns is the sentinels'."""
        S, T, _ = x.shape
        talk, dom, lvl = np.full((T, S), SENT_TALK), np.full((T, S), SENT_DOM), np.full((T, S), SENT_LEVEL)
        alive = np.ones(S, bool) if live is None else np.asarray(live) != 0
        gate = np.ones((T, S), bool) if opn is None else np.asarray(opn) != 0
        en = np.zeros((T, S), np.float64)
        on = gate & alive[None, :]
        en[on] = energy(x.transpose(1, 0, 2)[on])                                      # step 1: closed and absent frames are not read
        for t in range(T):
            for members in groups(self.room):
                L = [s for s in members if alive[s]]
                for s in L:                                                            # step 2
                    e = en[t, s] if gate[t, s] else np.float64(0.0)
                    d = self.level[s] * self.decay
                    self.level[s] = e if e > d else d
                cand = [s for s in L if gate[t, s]]                                    # step 3
                score = {s: self.level[s] * self.stick if self.sel[s] else self.level[s] for s in cand}
                rank = sorted(cand, key=lambda s: (-self.pinned[s], -u64(score[s]), s))
                top = rank[:self.k]                                                    # step 4
                self._note(rank, top, score)
                for s in L:
                    talk[t, s], dom[t, s], lvl[t, s] = s in top, rank[0] if rank else -1, self.level[s]
                    self.sel[s] = s in top
        return talk, dom, lvl

    def _note(self, rank, top, score):
        ev, k = self.events, self.k
        ev.add("none" if not rank else "exactly_k" if len(rank) == k else "more_than_k" if len(rank) > k else "fewer")
        out = rank[len(top):]
        if not out:
            return
        free = lambda L: [s for s in L if not self.pinned[s]]   # noqa: E731
        if any(not self.sel[s] for s in free(top)) and any(self.sel[s] for s in free(out)):
            ev.add("takeover")
        if any(self.sel[i] and not self.sel[c] and self.level[c] > self.level[i] for i in free(top) for c in free(out)):
            ev.add("held_off")
        a, b = top[-1], out[0]
        if self.pinned[a] == self.pinned[b] and u64(score[a]) == u64(score[b]):
            ev.add("tie")
        if any(self.pinned[p] and not self.pinned[c] and u64(score[c]) > u64(score[p]) for p in top for c in out):
            ev.add("pin_over_louder")


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
AMPS = np.array([1.0, 1.5, 3.0, 10.0, 30.0], np.float32)


def audio(seed, S, T, twins=(), pins=(), whole=False, duel=(), call=0, loud=0):
    """float32 [S, T, 480]: noise of a few hundred units times a per-stream-frame amplitude of AMPS -- energy ratios of 2.25 (inside a
    stick of 4) up to 900 --; the `twins` all carry the first twin's samples, the `pins` stay quiet, the `duel` follows duel_for's script,
    fifty times louder with every call (a decay of 1 never lets a level fall).  `whole`: whole numbers inside the int16 range, so that
    the three formats hold the same samples."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-270.0, 270.0, (S, T, FRAME)).astype(np.float32)
    amp = AMPS[rng.integers(0, AMPS.size, (S, T))]
    if len(pins):
        amp[list(pins)] = np.float32(0.25)
    if len(duel):
        amp[duel] = 1.0
        amp[duel[:loud], :2] = 8.0
        amp[duel[loud], 1], amp[duel[loud + 1], 2] = 12.0, 40.0
        amp[duel] *= np.float32(50.0) ** call
    x = x * amp[:, :, None]
    if len(twins):
        x[list(twins)] = x[twins[0]]
    return np.round(x) if whole else x


def open_rows(seed, S, T, call=0, twins=(), sched=(), pins=(), duel=()):
    """uint8 [T, S]: coin flips; the twins and the duel always open, the pins in every other frame; the scheduled room all open, then
    exactly its first k, then nobody."""
    o = (np.random.default_rng(seed).random((T, S)) < 0.6).astype(np.uint8)
    o[:, list(twins) + list(duel)] = 1
    o[:, list(pins)] = ((np.arange(T) + call) % 2)[:, None]
    if len(sched):
        plan = [sched, sched[:-1] if call else sched, [], sched[:1]]
        for t in range(T):
            o[t, sched] = 0
            o[t, plan[(t + call) % 4]] = 1
    return o


def picker(lib, S, room=None, pinned=None, policy=None):
    from nnnoiseless_amd.pick import TalkerPicker
    p = TalkerPicker(S, lib=lib)
    if room is not None:
        p.set_rooms(room)
    if pinned is not None:
        p.set_pinned(pinned)
    if policy is not None:
        p.set_policy(*policy)
    return p


def pin_mask(S, pins):
    m = np.zeros(S, np.uint8)
    m[list(pins)] = 1
    return m


# ---- the calls -----------------------------------------------------------------------------------------------------------------------------
def _run(mem, call, raw, at_in, opn, live, skip, alias=False):
    """Lay raw [S, T, 480] out at `at_in` in a buffer of garbage, make the call into rows of sentinels, return (talk, dominant, level), each
    [T, S]; the input, the masks and everything outside the rows must come back as they were.  `alias`: d_talk is d_open itself."""
    S, T, _ = raw.shape
    buf = np.full(int(at_in.max()) + 1, np.int16(9999) if raw.dtype == np.int16 else GARBAGE, raw.dtype)
    buf[at_in] = raw
    hin = mem.put(buf, skip)
    ho = None if opn is None else mem.put(np.ascontiguousarray(opn, dtype=np.uint8))
    hl = None if live is None else mem.put(np.ascontiguousarray(live, dtype=np.uint8))
    outs = [mem.put(np.full(T * S + 2 * PAD, sent)) for sent in (SENT_TALK, SENT_DOM, SENT_LEVEL)]
    ptrs = [h.ptr + PAD * np.dtype(type(sent)).itemsize for h, sent in zip(outs, (SENT_TALK, SENT_DOM, SENT_LEVEL))]
    if alias:
        ptrs[0] = ho.ptr
    call(hin.ptr, None if ho is None else ho.ptr, None if hl is None else hl.ptr, *ptrs)
    mem.sync()
    res = []
    for h, sent in zip(outs, (SENT_TALK, SENT_DOM, SENT_LEVEL)):
        a = h.get()
        assert (a[:PAD] == sent).all() and (a[PAD + T * S:] == sent).all(), "a write outside the rows"
        res.append(a[PAD:PAD + T * S].reshape(T, S))
    if alias:
        assert (res[0] == SENT_TALK).all()
        res[0] = ho.get().reshape(T, S)
    elif ho is not None:
        same(ho.get().reshape(T, S), np.ascontiguousarray(opn, dtype=np.uint8), "the open rows")
    same(hin.get(), buf, "the input")
    if hl is not None:
        same(hl.get(), np.ascontiguousarray(live, dtype=np.uint8), "the live mask")
    return tuple(res)


def device_call(p, mem, x, opn=None, live=None, skip=0, alias=False, **layout):
    S, T, _ = x.shape
    at, ss, fs = f32_index(S, T, **layout)
    return _run(mem, lambda i, o, l, tk, dm, lv: p.select_device(i, tk, T, ss, fs, d_open=o, d_live=l, d_dominant=dm, d_level=lv, hip_stream=mem.stream),
                x.astype(np.float32), at, opn, live, skip, alias)


def pcm_call(p, mem, raw, fmt, C, opn=None, live=None, skip=0, **pads):
    S, T, _ = raw.shape
    at, gs, fs = pcm_index(S, T, C, **pads)
    return _run(mem, lambda i, o, l, tk, dm, lv: p.select_pcm_device(i, tk, T, (fmt, C, gs, fs), d_open=o, d_live=l, d_dominant=dm, d_level=lv,
                                                                     hip_stream=mem.stream),
                raw.astype(np.int16 if fmt == I16 else np.float32), at, opn, live, skip)


def same3(got, want, tag=""):
    for g, w, name in zip(got, want, ("talk", "dominant", "level")):
        same(g, w, f"{tag} {name}")


# ---- the checks ----------------------------------------------------------------------------------------------------------------------------
def check_restatement(lib, mem, S, T, k, decay, stick):
    """Three calls of T frames: the second reads the level and the selection the first left, the third comes behind a set_policy to
    other values of all three.  talk, dominant and level equal the restatement; in the largest shape, which has room for rooms of every
    kind, the room-frames show every kind of event the issue lists (a challenger held off needs a stick above 1: the policy of the first
    two calls or of the third)."""
    room, twins, sched, pins = rooms_for(S, k)
    pinned, duel = pin_mask(S, pins), duel_for(S, k)
    p, rs = picker(lib, S, room, pinned, (k, decay, stick)), Restated(S, room, pinned, k, decay, stick)
    for call in range(3):
        if call == 2:
            p.set_policy(*next_policy(k, decay, stick)), rs.set_policy(*next_policy(k, decay, stick))
        x = audio(100 * S + 10 * T + call, S, T, twins, pins, duel=duel, call=call, loud=rs.k)
        opn = open_rows(7 * S + T + call, S, T, call, twins, sched, pins, duel)
        opn = None if (S == 3 and call == 1) else opn
        got = device_call(p, mem, x, opn, layout="frames" if call else "streams")
        same3(got, rs.select(x, opn), f"call {call}")
    if S == 300:
        assert rs.events >= EVENTS, sorted(EVENTS - rs.events)
    p.close()


def check_chunking(lib, mem, S=12, T=11):
    """Eleven frames as one call, as eleven calls of one frame, as 3 + 8 and as 5 + 5 + 1: the same bits."""
    room, twins, sched, pins = rooms_for(S)
    pinned = pin_mask(S, pins)
    x, opn = audio(77, S, T, twins, pins), open_rows(78, S, T, 0, twins, sched, pins)
    want = Restated(S, room, pinned, 2).select(x, opn)
    assert len(set(want[1].reshape(-1).tolist())) > 3 and 0 < want[0].mean() < 1
    for cuts in ([11], [1] * 11, [3, 8], [5, 5, 1]):
        p, parts, t = picker(lib, S, room, pinned, (2, 0.875, 4.0)), [], 0
        for i, n in enumerate(cuts):
            parts.append(device_call(p, mem, x[:, t:t + n], opn[t:t + n], layout="streams" if i & 1 else "frames"))
            t += n
        same3([np.concatenate(c) for c in zip(*parts)], want, f"cuts {cuts}")
        p.close()


def check_layout(lib, mem, S=12, T=3):
    """Padded strides, both orders of streams and frames, the base at every 4-byte offset of a 16-byte line; the packed boundary: the three
    formats at one and two channels with odd paddings and odd int16 bases -- whole-number samples, which all three hold alike, so one
    restatement serves --; d_talk on top of d_open.  (_run checks the input, the masks and the sentinels around the rows.)"""
    room, twins, sched, pins = rooms_for(S)
    pinned = pin_mask(S, pins)
    xs = [audio(5 + c, S, T, twins, pins, whole=True) for c in range(2)]
    opns = [open_rows(15 + c, S, T, c, twins, sched, pins) for c in range(2)]
    rs = Restated(S, room, pinned, 2)
    want = [rs.select(xs[c], opns[c]) for c in range(2)]
    assert np.abs(xs[0]).max() < 32768 and 0 < want[0][0].mean() < 1

    def two_calls(call, tag):
        p = picker(lib, S, room, pinned, (2, 0.875, 4.0))
        for c in range(2):
            same3(call(p, c), want[c], f"{tag} call {c}")
        p.close()

    for lay, skip in (({"layout": "frames"}, 0), ({"layout": "streams", "stream_pad": 8}, 0), ({"layout": "frames", "stream_pad": 1, "frame_pad": 2}, 0),
                      ({"layout": "streams", "frame_pad": 4}, 1), ({"layout": "frames"}, 2), ({"layout": "streams"}, 3),
                      ({"layout": "streams", "frame_pad": 3, "stream_pad": 5}, 1), ({"layout": "frames", "frame_pad": 1}, 3)):
        two_calls(lambda p, c: device_call(p, mem, xs[c], opns[c], skip=skip, **lay), f"{lay} {skip}")
    for fmt in (F32, I16, F32_UNIT):
        raws = [(x / np.float32(32768.0)).astype(np.float32) for x in xs] if fmt == F32_UNIT else xs
        same(load(raws[0], fmt), xs[0], "the formats hold the same samples")
        for C, pads, skip in ((1, {}, 0), (1, {"frame_pad": 3}, 3 if fmt == I16 else 1), (2, {"frame_pad": 5, "group_pad": 3}, 1), (2, {}, 2)):
            two_calls(lambda p, c: pcm_call(p, mem, raws[c], fmt, C, opns[c], skip=skip, **pads), f"format {fmt} channels {C} {pads}")
    two_calls(lambda p, c: device_call(p, mem, xs[c], opns[c], alias=True), "d_talk == d_open")


def check_live(lib, mem, S=12, T=3):
    """Masked streams are no members for the call: their rows keep the sentinels, their inputs and open entries may be anything, their
    state is frozen -- continuing them later equals never having made the masked call --, and the others' bits are those of a room
    without them."""
    room, twins, sched, pins = rooms_for(S)
    pinned = pin_mask(S, pins)
    live = (np.arange(S) % 3 != 1).astype(np.uint8)
    xs = [audio(50 + c, S, T, twins, pins) for c in range(3)]
    opns = [open_rows(60 + c, S, T, c, twins, sched, pins) for c in range(3)]
    p, rs = picker(lib, S, room, pinned, (2, 0.875, 4.0)), Restated(S, room, pinned, 2)
    same3(device_call(p, mem, xs[0], opns[0]), rs.select(xs[0], opns[0]))
    frozen = (rs.level.copy(), rs.sel.copy())
    x1, o1 = xs[1].copy(), opns[1].copy()
    x1[live == 0], o1[:, live == 0] = np.nan, 1
    got = device_call(p, mem, x1, o1, live=live)
    same3(got, rs.select(x1, o1, live=live), "the masked call")
    assert (got[0][:, live == 0] == SENT_TALK).all() and (got[1][:, live == 0] == SENT_DOM).all() and (got[2][:, live == 0] == SENT_LEVEL).all()
    assert np.array_equal(rs.level[live == 0], frozen[0][live == 0]) and (frozen[0][live == 0] > 0).any() and (frozen[1][live == 0] != 0).any()
    # the same bits as a picker in which the masked streams sit alone and closed
    other = picker(lib, S, np.where(live == 0, -1, room).astype(np.int32), pinned, (2, 0.875, 4.0))
    device_call(other, mem, xs[0], opns[0])
    g2 = device_call(other, mem, xs[1], np.where(live == 0, 0, opns[1]).astype(np.uint8))
    for a, b, name in zip(got, g2, ("talk", "dominant", "level")):
        same(a[:, live == 1], b[:, live == 1], f"live streams against a room without the others: {name}")
    # the state was frozen: the third call continues the masked streams from call 0
    same3(device_call(p, mem, xs[2], opns[2]), rs.select(xs[2], opns[2]), "behind the masked call")
    p.close(), other.close()


def check_unread(lib, mem, S=12, T=3):
    """NaN in the input of every closed and every absent stream-frame changes nothing."""
    room, twins, sched, pins = rooms_for(S)
    pinned = pin_mask(S, pins)
    live = (np.arange(S) % 4 != 2).astype(np.uint8)
    x, opn = audio(33, S, T, twins, pins), open_rows(34, S, T, 0, twins, sched, pins)
    opn[:, 0] = [1, 0, 1]
    want = Restated(S, room, pinned, 2).select(x, opn, live=live)
    unread = (opn.T == 0) | (live == 0)[:, None]
    assert unread.sum() > 8 and (~unread).sum() > 8
    xn = x.copy()
    xn[unread] = np.nan
    p = picker(lib, S, room, pinned, (2, 0.875, 4.0))
    same3(device_call(p, mem, xn, opn, live=live), want, "NaN in the unread inputs")
    p.close()


def check_nonfinite(lib, mem, S=12, T=3):
    """NaN and inf samples in open frames make those frames measure silent: every other stream-frame keeps the clean run's bits (where the
    clean run's selection did not rest on the silenced frames: the hit streams talk in rooms of their own here), and the levels stay
    finite afterwards."""
    room = np.array([5, 5, 5, 5, 5, 5, 5, 5, 5, 1, 1, -1], np.int32)       # a room of nine, a pair, a loner
    hit = {(9, 1): np.nan, (10, 0): np.inf, (11, 2): -np.inf, (11, 0): np.nan}
    clean = audio(91, S, T)
    clean[9:] = np.random.default_rng(92).uniform(-270.0, 270.0, (3, T, FRAME)).astype(np.float32) * np.array([2, 4, 6], np.float32)[None, :, None]
    x = clean.copy()                                                       # (the three get louder by the frame: their clean level is the frame's energy)
    for n, ((s, t), v) in enumerate(hit.items()):
        x[s, t, 7 + 60 * n] = v
    p, ref = picker(lib, S, room, None, (2, 0.5, 4.0)), picker(lib, S, room, None, (2, 0.5, 4.0))
    got, want = device_call(p, mem, x), device_call(ref, mem, clean)
    same3(got, Restated(S, room, None, 2, 0.5).select(x), "the restatement")
    for a, b, name in zip(got, want, ("talk", "dominant", "level")):
        same(a[:, :9], b[:, :9], f"the room beside them: {name}")
    same(got[0], want[0], "talk everywhere: a silent candidate of a room of at most k still talks")
    lvl, cl = got[2], want[2]
    assert np.isfinite(lvl).all()
    assert lvl[0, 10] == 0 and lvl[0, 11] == 0 and lvl[1, 9] == cl[0, 9] * 0.5 and lvl[2, 11] == cl[1, 11] * 0.5, "a hit frame measures as silent"
    same(lvl[1, 10], cl[1, 10]), same(lvl[2, 9], cl[2, 9])                  # (the next clean frame is louder than what decayed: the clean bits again)
    got2, want2 = device_call(p, mem, clean), device_call(ref, mem, clean)
    assert np.isfinite(got2[2]).all()
    same(got2[2][1:], want2[2][1:], "the levels afterwards")
    p.close(), ref.close()


def check_consequences(lib, mem):
    """What the header says follows from the rule, each checked on the device's own outputs against numbers made here and not by the
    restatement."""
    S, T, k, stick = 80, 5, 3, 4.0
    room, twins, sched, pins = rooms_for(S, k)
    pinned = pin_mask(S, pins)
    p = picker(lib, S, room, pinned, (k, 0.25, stick))                       # (a fast release: the talkers change often)
    prev = np.zeros(S, np.uint8)
    swaps = 0
    for call in range(3):
        x, opn = audio(300 + call, S, T, twins, pins), open_rows(310 + call, S, T, call, twins, sched, pins)
        talk, dom, lvl = device_call(p, mem, x, opn, layout="frames")
        assert (talk <= opn).all(), "talk is a subset of open"
        for t in range(T):
            for g in groups(room):
                g = np.array(g)
                o, tk = opn[t, g] != 0, talk[t, g] != 0
                assert tk.sum() == min(k, o.sum()), "min(k, candidates) talkers: at most k, and talk == open up to k candidates"
                pin_open = g[o & (pinned[g] != 0)]
                assert len(pin_open) > k or talk[t, pin_open].all(), "a pinned open stream is selected"
                assert (dom[t, g] == (-1 if not o.any() else dom[t, g[0]])).all() and (not o.any() or (opn[t, dom[t, g[0]]] and room[dom[t, g[0]]] == room[g[0]]))
                free = g[pinned[g] == 0]
                new = [c for c in free if talk[t, c] and not prev[c]]
                lost = [i for i in free if prev[i] and opn[t, i] and not talk[t, i]]
                for c in new:
                    for i in lost:
                        swaps += 1
                        assert lvl[t, c] > lvl[t, i] * np.float64(stick) or (lvl[t, c] == lvl[t, i] * np.float64(stick) and c < i), "a challenger displaces an incumbent only above stick x its level"
            prev = talk[t]
        plain = (x.astype(np.float64) ** 2).sum(axis=2).T                      # the energies, in NumPy's own order
        assert np.allclose(lvl[0][opn[0] != 0], plain[0][opn[0] != 0], rtol=1e-12, atol=0) or call
    assert swaps > 3, swaps
    p.close()
    # equal scores go to the lower index: four streams with the same samples, k = 2, whichever order the labels come in
    x = audio(1, 6, 2, twins=[1, 2, 4, 5])
    p = picker(lib, 6, np.array([-1, 3, 3, 0, 3, 3], np.int32), None, (2, 1.0, 1.0))
    talk, dom, _ = device_call(p, mem, x)
    assert talk.tolist() == [[1, 1, 1, 1, 0, 0]] * 2 and dom.tolist() == [[0, 1, 1, 3, 1, 1]] * 2
    p.close()
    # pins beat loudness: two quiet pinned streams among four loud ones, k = 2
    x = audio(2, 6, 3, pins=[2, 5])
    p = picker(lib, 6, np.zeros(6, np.int32), pin_mask(6, [2, 5]), (2, 0.875, 4.0))
    talk, dom, lvl = device_call(p, mem, x)
    assert talk.tolist() == [[0, 0, 1, 0, 0, 1]] * 3 and np.isin(dom, [2, 5]).all() and (lvl[:, [0, 1, 3, 4]].min() > lvl[:, [2, 5]].max())
    p.close()


def check_n_streams(lib, mem, T=3):
    """The bits depend neither on n_streams nor on the labels: a room of five alone in an object of five against the same room spread over
    an object of thirteen whose other streams talk in rooms of their own, and against the same rooms under other labels."""
    at = [2, 5, 6, 9, 12]
    x, opn, pinned = audio(55, 5, T), open_rows(56, 5, T), pin_mask(5, [3])
    small = picker(lib, 5, np.zeros(5, np.int32), pinned, (2, 0.875, 4.0))
    room = np.array([4, 4, 7, 4, -1, 7, 7, 0, 0, 7, 0, 4, 7], np.int32)
    relabel = {4: 0, 7: 12, 0: 5, -1: -1}
    x13, o13, p13 = audio(57, 13, T), open_rows(58, 13, T), pin_mask(13, [0, 8])
    x13[at], o13[:, at], p13[at] = x, opn, pinned
    big = picker(lib, 13, room, p13, (2, 0.875, 4.0))
    other = picker(lib, 13, np.array([relabel[int(r)] for r in room], np.int32), p13, (2, 0.875, 4.0))
    for call in range(2):
        gs, gb, go = device_call(small, mem, x, opn), device_call(big, mem, x13, o13, layout="frames"), device_call(other, mem, x13, o13)
        same(gb[0][:, at], gs[0], f"call {call}: talk of the room inside a larger object"), same(gb[2][:, at], gs[2], "level")
        same(gb[1][:, at], np.where(gs[1] < 0, gs[1], np.array(at, np.int32)[gs[1]]), "dominant, in the larger object's indices")
        same3(go, gb, "relabelled rooms")
    assert 0 < gs[0].mean() < 1
    small.close(), big.close(), other.close()


def check_state(lib, mem, S=12, T=2):
    """reset zeroes level and selected of the listed streams only; the setters take effect at the next call's first frame and read back."""
    room, twins, sched, pins = rooms_for(S)
    pinned = pin_mask(S, pins)
    p, rs = picker(lib, S, room, pinned), Restated(S, room, pinned)
    assert p.policy() == (3, 0.875, 4.0) and p.rooms().tolist() == room.tolist() and p.pinned().tolist() == pinned.tolist()
    xs = [audio(80 + c, S, T, twins, pins) for c in range(4)]
    same3(device_call(p, mem, xs[0]), rs.select(xs[0]))
    p.reset([4, 2]), rs.reset([4, 2])
    want = rs.select(xs[1])
    same3(device_call(p, mem, xs[1]), want, "behind the reset")
    assert not np.array_equal(want[2][0], Restated(S, room, pinned).select(xs[1])[2][0])
    p.set_rooms([1, -1, 3], idx=[0, 7, 5]), p.set_pinned([1, 0], idx=[9, 4]), p.set_policy(2, 0.5, 1.5)
    rs.room[[0, 7, 5]], rs.pinned[[9, 4]] = [1, -1, 3], [1, 0]
    rs.set_policy(2, 0.5, 1.5)
    assert p.rooms().tolist() == rs.room.tolist() and p.rooms([7, 0]).tolist() == [-1, 1] and p.pinned().tolist() == rs.pinned.tolist()
    assert p.pinned([9]).tolist() == [1] and p.policy() == (2, 0.5, 1.5)
    same3(device_call(p, mem, xs[2]), rs.select(xs[2]), "behind the setters")
    p.reset(), rs.reset()
    got = device_call(p, mem, xs[3])
    same3(got, rs.select(xs[3]), "behind the whole reset")
    new = Restated(S, rs.room, rs.pinned, 2, 0.5, 1.5)
    same3(got, new.select(xs[3]), "a reset object is a new one")
    p.close()


def check_host_call(lib, mem, S=12, T=3):
    """The host call (dense [S][T][480]) gives the device-style call's bits, with and without masks and optional outputs; the Python
    mirror hands back zeros where nothing was written."""
    room, twins, sched, pins = rooms_for(S)
    pinned = pin_mask(S, pins)
    live = (np.arange(S) % 4 != 2).astype(np.uint8)
    p, rs = picker(lib, S, room, pinned, (2, 0.875, 4.0)), Restated(S, room, pinned, 2)
    for call, (lv, op) in enumerate(((None, True), (live, True), (None, False))):
        x = audio(20 + call, S, T, twins, pins)
        opn = open_rows(25 + call, S, T, call, twins, sched, pins) if op else None
        got = p.select(x, open=opn, live=lv, want_dominant=True, want_level=True)
        want = [w.copy() for w in rs.select(x, opn, live=lv)]
        if lv is not None:
            for w in want:
                w[:, lv == 0] = 0
        same3(got, want, f"host call {call}")
    x = audio(29, S, T, twins, pins)
    want = rs.select(x)
    talk = p.select(x)
    same(talk, want[0]), same(p.select(x, want_level=True)[0], rs.select(x)[0])
    assert isinstance(talk, np.ndarray) and len(p.select(x, want_dominant=True)) == 2
    rs.select(x)
    # the C call itself leaves what a masked stream owns as it was
    tk, dm, lv = np.full((T, S), SENT_TALK), np.full((T, S), SENT_DOM), np.full((T, S), SENT_LEVEL)
    lib.check(lib.L.nnn_pick_select_host(p._h, _ffi.ptr(x), None, _ffi.ptr(live), _ffi.ptr(tk), _ffi.ptr(dm), _ffi.ptr(lv), T))
    same3((tk, dm, lv), rs.select(x, live=live), "the C host call under a live mask")
    p.close()


def check_refusals(lib, mem):
    """Every refusal of the header with its text; each leaves the object as it was: rooms, pins and policy read back unchanged and a
    following call equals the restatement's (so level and selected did not move either)."""
    import ctypes as C
    import pytest
    from nnnoiseless_amd.pick import TalkerPicker
    L = lib.L

    def refused(rc, text):
        assert rc != 0 and text in lib.error(), (rc, text, lib.error())

    for S in (0, -1):
        assert not L.nnn_pick_create(S, 0) and "n_streams" in lib.error()
    with pytest.raises(RuntimeError, match="n_streams = 0"):
        TalkerPicker(0, lib=lib)
    L.nnn_pick_destroy(None)
    S, T = 4, 2
    room, pinned = np.array([1, 1, -1, 1], np.int32), np.array([0, 0, 0, 1], np.uint8)
    p, rs = picker(lib, S, room, pinned, (1, 0.5, 2.0)), Restated(S, room, pinned, 1, 0.5, 2.0)
    x = audio(1, S, T)
    same3(device_call(p, mem, x), rs.select(x))
    hx, ht, hd = mem.put(x.transpose(1, 0, 2)), mem.put(np.zeros(T * S + 8, np.uint8)), mem.put(np.zeros(2 * T * S + 2, np.float64))
    i, tk, dv, h = hx.ptr, ht.ptr, hd.ptr, p._h
    lay = _ffi.PcmLayout(F32, 1, 0, 0, FRAME, S * FRAME)
    bl = C.byref(lay)
    ri, pu, host_tk = np.zeros(S, np.int32), np.zeros(S, np.uint8), np.zeros((T, S), np.uint8)
    # a NULL object
    refused(L.nnn_pick_select_device(None, i, None, None, tk, None, None, T, FRAME, S * FRAME, None), "null picker")
    refused(L.nnn_pick_select_pcm_device(None, i, None, None, tk, None, None, T, bl, None), "null picker")
    refused(L.nnn_pick_select_host(None, _ffi.ptr(x), None, None, _ffi.ptr(host_tk), None, None, T), "null picker")
    refused(L.nnn_pick_set_rooms(None, None, S, _ffi.ptr(ri)), "null picker"), refused(L.nnn_pick_get_rooms(None, None, S, _ffi.ptr(ri)), "null picker")
    refused(L.nnn_pick_set_pinned(None, None, S, _ffi.ptr(pu)), "null picker"), refused(L.nnn_pick_get_pinned(None, None, S, _ffi.ptr(pu)), "null picker")
    refused(L.nnn_pick_set_policy(None, 3, 0.5, 2.0), "null picker"), refused(L.nnn_pick_get_policy(None, None, None, None), "null picker")
    refused(L.nnn_pick_reset(None, None, 0), "null picker")
    # NULL buffers, the frame count, strides, alignment
    for args, text in (((None, None, None, tk), "null input"), ((i, None, None, None), "null talk rows")):
        refused(L.nnn_pick_select_device(h, *args, None, None, T, FRAME, S * FRAME, None), text)
        refused(L.nnn_pick_select_pcm_device(h, *args, None, None, T, bl, None), text)
    refused(L.nnn_pick_select_host(h, None, None, None, _ffi.ptr(host_tk), None, None, T), "null input")
    refused(L.nnn_pick_select_host(h, _ffi.ptr(x), None, None, None, None, None, T), "null talk rows")
    for n in (0, -3):
        refused(L.nnn_pick_select_device(h, i, None, None, tk, None, None, n, FRAME, S * FRAME, None), f"n_frames = {n}")
        refused(L.nnn_pick_select_pcm_device(h, i, None, None, tk, None, None, n, bl, None), f"n_frames = {n}")
        refused(L.nnn_pick_select_host(h, _ffi.ptr(x), None, None, _ffi.ptr(host_tk), None, None, n), f"n_frames = {n}")
    refused(L.nnn_pick_select_device(h, i, None, None, tk, None, None, T, FRAME, FRAME - 1, None), "frame_stride = 479 is below a frame's 480")
    refused(L.nnn_pick_select_device(h, i + 2, None, None, tk, None, None, T, FRAME, S * FRAME, None), "4-byte samples")
    refused(L.nnn_pick_select_device(h, i, None, None, tk, dv + 2, None, T, FRAME, S * FRAME, None), "dominant rows are not aligned")
    refused(L.nnn_pick_select_device(h, i, None, None, tk, None, dv + 4, T, FRAME, S * FRAME, None), "level rows are not aligned")
    refused(L.nnn_pick_select_pcm_device(h, i, None, None, tk, dv + 1, None, T, bl, None), "dominant rows are not aligned")
    # the packed boundary: layout, format, channels, discard_first, stride, alignment
    refused(L.nnn_pick_select_pcm_device(h, i, None, None, tk, None, None, T, None, None), "null layout")
    for bad, text in ((_ffi.PcmLayout(3, 1, 0, 0, FRAME, S * FRAME), "format 3"), (_ffi.PcmLayout(-1, 1, 0, 0, FRAME, S * FRAME), "format -1"),
                      (_ffi.PcmLayout(F32, 0, 0, 0, FRAME, S * FRAME), "channels = 0"), (_ffi.PcmLayout(I16, 3, 0, 0, FRAME, S * FRAME * 3), "channels = 3"),
                      (_ffi.PcmLayout(F32, 1, 1, 0, FRAME, S * FRAME), "discard_first must be 0"),
                      (_ffi.PcmLayout(F32, 2, 0, 0, 2 * T * FRAME, 2 * FRAME - 1), "frame_stride = 959 is below a frame's 960")):
        refused(L.nnn_pick_select_pcm_device(h, i, None, None, tk, None, None, T, C.byref(bad), None), text)
    i16 = _ffi.PcmLayout(I16, 1, 0, 0, FRAME, S * FRAME)
    refused(L.nnn_pick_select_pcm_device(h, i + 1, None, None, tk, None, None, T, C.byref(i16), None), "2-byte samples")
    refused(L.nnn_pick_select_pcm_device(h, i + 2, None, None, tk, None, None, T, bl, None), "4-byte samples")
    # index lists, rooms, pins and the policy
    with pytest.raises(RuntimeError, match=r"stream 4 outside \[0, 4\)"):
        p.set_rooms(0, idx=[0, 4])
    with pytest.raises(RuntimeError, match="stream -1 outside"):
        p.reset([-1])
    with pytest.raises(RuntimeError, match="stream 7 outside"):
        p.pinned([7])
    with pytest.raises(RuntimeError, match="stream 2 is listed twice"):
        p.set_rooms(0, idx=[2, 1, 2])
    with pytest.raises(RuntimeError, match="stream 1 is listed twice"):
        p.set_pinned(1, idx=[1, 1])
    with pytest.raises(RuntimeError, match="5 entries for 4 streams"):
        lib.check(L.nnn_pick_set_pinned(h, None, 5, _ffi.ptr(np.zeros(5, np.uint8))))
    refused(L.nnn_pick_set_rooms(h, None, S, None), "null rooms"), refused(L.nnn_pick_set_pinned(h, None, S, None), "null pins")
    refused(L.nnn_pick_set_rooms(h, None, -1, _ffi.ptr(ri)), "n = -1")
    for bad, text in ((-2, r"room -2 outside \[-1, 4\)"), (4, "room 4 outside")):
        with pytest.raises(RuntimeError, match="entry 1: " + text):
            p.set_rooms([0, bad], idx=[3, 0])
    for bad in (2, 255):
        with pytest.raises(RuntimeError, match=f"entry 1: pinned {bad} is neither 0 nor 1"):
            p.set_pinned([1, bad], idx=[3, 0])
    nan, inf = float("nan"), float("inf")
    for pol, text in (((0, 0.5, 2.0), r"k = 0 outside \[1, 8\]"), ((9, 0.5, 2.0), "k = 9 outside"), ((-1, 0.5, 2.0), "k = -1 outside"),
                      ((2, -0.25, 2.0), r"decay -0.25 outside \[0, 1\]"), ((2, 1.5, 2.0), "decay 1.5 outside"), ((2, nan, 2.0), "decay nan outside"),
                      ((2, 0.5, 0.5), r"stick 0.5 outside \[1, 16\]"), ((2, 0.5, 16.5), "stick 16.5 outside"), ((2, 0.5, nan), "stick nan outside"),
                      ((2, 0.5, inf), "stick inf outside"), ((2, -inf, 2.0), "decay -inf outside")):
        with pytest.raises(RuntimeError, match=text):
            p.set_policy(*pol)
    with pytest.raises(ValueError):
        p.set_pinned([1, 1, 1], idx=[0, 1])
    with pytest.raises(ValueError):
        p.select(x[:3])
    with pytest.raises(ValueError):
        p.select(x, open=np.ones((T, 3)))
    # nothing of that changed the object
    assert p.rooms().tolist() == room.tolist() and p.pinned().tolist() == pinned.tolist() and p.policy() == (1, 0.5, 2.0)
    x = audio(3, S, T)
    opn = np.array([[1, 0, 1, 1], [1, 1, 1, 0]], np.uint8)
    same3(device_call(p, mem, x, opn), rs.select(x, opn), "after the refusals")
    assert L.nnn_pick_set_rooms(h, None, 0, None) == 0 and L.nnn_pick_reset(h, (C.c_int * 1)(0), 0) == 0
    p.close()
