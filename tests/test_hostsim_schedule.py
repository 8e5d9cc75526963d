"""The stream and event graph of a call (nnn_batch_launch.hip plan_schedule, read through nnn_batch_debug_schedule) orders everything that
must be ordered.  The interpreter cannot see a missing edge -- its streams are one stream and its kernels run in issue order -- so
this file checks the graph itself: for every schedule the hook returns, every required pair (A before B) must follow from stream
order and from event waits whose event the right node recorded last.

The required orderings are restated here from what the stages read and write, not taken from the code under test:
  * a group's stages run hp -> pitch -> fft_xp -> rnn -> synth;
  * hp, pitch, rnn and synth carry state from one group to the next (biquad, last pitch, GRU / cepstral state, overlap memory);
  * group k works in scratch-set block k mod depth, so its pitch stage (the first to write the block) follows the synthesis of group
    k - depth (the last to read it);
  * the high-pass of a group whose newest frame is f overwrites the history-ring slots of frame f - nslot and older, which the frames
    up to 3 later still read: it follows the synthesis of the group that holds frame f + 3 - nslot (nnn_layout.h: nslot =
    (depth + 1) * max_group_frames + 4 slots);
  * everything enqueued before the call comes first, and the caller's stream ends behind the last synthesis.
An event is slot (stage, group mod 16) of a ring the call owns (include/nnn_batch.h), so a wait means the node that recorded the slot
most recently -- which must be the node the wait names, not the one 16 groups before or after it."""
import ctypes as C

import numpy as np
import pytest

HP, PITCH, FFT, RNN, SYN = range(5)
STATEFUL = (HP, PITCH, RNN, SYN)
EVR = 16
CALLER = -1
THIS, PREV, DONE = 0, 1, 2
S = 3                                              # one tile
FRAMES = (1, 31, 32, 33, 48, 96)
SCHEDULES = [("seq", 0), ("lanes", 1), ("lanes", 2), ("lanes", 3), ("stages", 0)]


def query(lib, bd, n):
    cap = 8 + 17 * 5 * n
    buf = (C.c_int32 * cap)()
    lib.check(lib.L.nnn_batch_debug_schedule(bd._h, n, buf, cap))
    head = dict(zip(("nodes", "groups", "pipe", "sched", "lanes", "fill", "fill_after_done", "last_syn"), buf[:8]))
    nodes = []
    for i in range(head["nodes"]):
        v = buf[8 + 17 * i:8 + 17 * (i + 1)]
        nodes.append(dict(zip(("stage", "group", "frames", "first", "stream", "first_use", "record"), v[:7]),
                          waits=[tuple(v[8 + 3 * w:11 + 3 * w]) for w in range(v[7])]))
    return head, nodes


def happens_before(nodes):
    """hb[i]: the nodes (a bit mask) known to be complete when node i starts -- its stream's earlier nodes and, through each wait on
    an event of this call, the node that recorded that slot last, each with what was complete before them.  Also the node that holds
    every slot at the end of the call."""
    hb, last_on, slot = [], {}, {}
    for i, n in enumerate(nodes):
        m = 0
        if n["stream"] in last_on:
            p = last_on[n["stream"]]
            m |= hb[p] | 1 << p
        for origin, s, k in n["waits"]:
            if origin != THIS:
                continue
            assert (s, k % EVR) in slot, (n, "waits for an event no node has recorded")
            r = slot[(s, k % EVR)]
            assert (nodes[r]["stage"], nodes[r]["group"]) == (s, k), (n, nodes[r], "the slot was last recorded by another group")
            m |= hb[r] | 1 << r
        hb.append(m)
        last_on[n["stream"]] = i
        if n["record"]:
            slot[(n["stage"], n["group"] % EVR)] = i
    return hb, slot


def check_call(head, nodes, n_frames, gmax, depth, early=False):
    """One call's graph.  early: the call may start its high-pass chain on internal stream 0 before the caller's stream has seen the
    previous call drain (check_boundary looks at what that chain then waits for)."""
    G = head["groups"]
    assert head["nodes"] == len(nodes) == 5 * G and G >= 1
    at = {(n["stage"], n["group"]): i for i, n in enumerate(nodes)}
    assert len(at) == 5 * G and all((s, k) in at for s in range(5) for k in range(G))
    first, frames = [nodes[at[(HP, k)]]["first"] for k in range(G)], [nodes[at[(HP, k)]]["frames"] for k in range(G)]
    assert first[0] == 0 and all(first[k] + frames[k] == (first[k + 1] if k + 1 < G else n_frames) for k in range(G))
    assert all(1 <= g <= gmax for g in frames)
    assert all((n["frames"], n["first"]) == (frames[n["group"]], first[n["group"]]) for n in nodes)
    if not head["pipe"]:
        assert all(n["stream"] == CALLER for n in nodes)
    hb, slot = happens_before(nodes)

    def need(a, b, why):
        assert hb[at[b]] >> at[a] & 1, (why, a, b, nodes[at[b]])

    nslot = (depth + 1) * gmax + 4
    for k in range(G):
        for s in range(1, 5):
            need((s - 1, k), (s, k), "previous stage")
        if k > 0:
            for s in STATEFUL:
                need((s, k - 1), (s, k), "state of the previous group")
        if k >= depth:
            need((SYN, k - depth), (PITCH, k), "previous user of the scratch-set block")
        edge = first[k] + frames[k] - 1 + 3 - nslot
        if edge >= 0:
            j = max(j for j in range(G) if first[j] <= edge)
            assert j < k
            need((SYN, j), (HP, k), "last reader of the ring slots")
    # everything before the call comes first: the first launch on every internal stream waits for the caller's stream
    seen = set()
    for n in nodes:
        fresh = n["stream"] not in seen
        seen.add(n["stream"])
        exempt = n["stream"] == CALLER or (early and n["stream"] == 0)
        assert n["first_use"] == (1 if fresh and not exempt else 0), n
    # the caller's stream ends behind the last synthesis
    last = at[(SYN, G - 1)]
    if nodes[last]["stream"] != CALLER:
        assert head["last_syn"] == G - 1 and slot.get((SYN, (G - 1) % EVR)) == last
    else:
        assert head["last_syn"] in (-1, G - 1) and (head["last_syn"] < 0 or slot.get((SYN, (G - 1) % EVR)) == last)
    # the parameter table is filled before anything reads it: by the first launch, or ahead of the call's streams
    assert head["fill"] in ((1, 2) if early else (1,)) if head["pipe"] else head["fill"] in (0, 1)
    return first, frames, slot


def make(lib, monkeypatch, gmax, sched, lanes, how):
    """A batch on the schedule, and the groups it keeps in flight: chosen at creation the batch has the second block of scratch sets
    and the longer ring (include/nnn_batch.h: under NNN_LANES >= 2 / NNN_SCHED=stages), set afterwards it works with one."""
    import nnnoiseless_amd as nn
    if how == "create":
        monkeypatch.setenv("NNN_SCHED", sched)
        if lanes:
            monkeypatch.setenv("NNN_LANES", str(lanes))
    bd = nn.BatchDenoiser(S, lib=lib, max_group_frames=gmax)
    monkeypatch.delenv("NNN_SCHED", raising=False)
    monkeypatch.delenv("NNN_LANES", raising=False)
    if how == "set":
        bd.set_schedule(sched, lanes)
    return bd, (2 if how == "create" and (lanes >= 2 or sched == "stages") else 1)


@pytest.mark.parametrize("how", ["create", "set"])
@pytest.mark.parametrize("sched,lanes", SCHEDULES)
@pytest.mark.parametrize("gmax", [1, 8, 24])
def test_every_schedule_orders_what_must_be_ordered(hostsim_lib, monkeypatch, gmax, sched, lanes, how):
    """max_group_frames 1 with 33 frames: 33 groups on a 6- or 7-slot ring -- the event ring is reused and the ring edge is three or
    four groups back; 8 with 48 frames: the ring edge inside the call; 24: before the call."""
    bd, depth = make(hostsim_lib, monkeypatch, gmax, sched, lanes, how)
    for n in FRAMES:
        head, nodes = query(hostsim_lib, bd, n)
        assert head["pipe"] == (1 if sched != "seq" and n >= 32 else 0), (n, head)   # (calls of 32 frames or more spread over streams)
        if head["pipe"]:
            assert (head["sched"], head["lanes"]) == ({"lanes": 1, "stages": 2}[sched], lanes or head["lanes"])
            assert len({m["stream"] for m in nodes}) > 1
        check_call(head, nodes, n, gmax, depth)
        if gmax == 1 and n >= 33:
            assert head["groups"] == n > EVR + 1                                      # (the event ring goes round)


def test_pipeline_off_and_all_held(hostsim_lib, monkeypatch):
    bd, depth = make(hostsim_lib, monkeypatch, 8, "lanes", 2, "create")
    bd.set_pipeline(False)
    for n in FRAMES:
        head, nodes = query(hostsim_lib, bd, n)
        assert head["pipe"] == 0
        check_call(head, nodes, n, 8, depth)
    bd.set_pipeline(True)
    bd.hold_streams([0, 1, 2])                     # every stream held: the call launches nothing
    for n in (1, 48):
        head, nodes = query(hostsim_lib, bd, n)
        assert (head["nodes"], head["pipe"], head["fill"], head["last_syn"]) == (0, 0, 0, -1) and nodes == [] and head["groups"] >= 1
    bd.resume_streams([0, 1, 2])
    head, nodes = query(hostsim_lib, bd, 48)
    assert head["pipe"] == 1
    check_call(head, nodes, 48, 8, depth)


def check_boundary(head, nodes, first, frames, depth, gmax, prev, prev_len, older_call):
    """A call whose high-pass chain does not wait for the caller's stream: what it needs from the calls before it, it waits for by
    event.  prev: (nodes, first, final slots) of the previous call's schedule, a call of prev_len frames; older_call: there was a
    call before that one."""
    pnodes, pfirst, pslot = prev
    pat = {(n["stage"], n["group"]): i for i, n in enumerate(pnodes)}
    assert head["fill"] == 2 and head["fill_after_done"] == (1 if older_call else 0)    # behind the table's previous user
    hp = [n for n in nodes if n["stage"] == HP]
    assert all(n["stream"] == 0 for n in hp) and all(n["stream"] == 0 for n in pnodes if n["stage"] == HP)   # (the biquad state: stream order)
    nslot = (depth + 1) * gmax + 4
    synth_seen, done_seen = -1, False              # what the chain has waited for so far: synthesis of the previous call up to this group
    for k, n in enumerate(hp):
        for origin, s, j in n["waits"]:
            if origin == PREV:
                r = pat[(s, j)]
                assert pnodes[r]["record"] and pslot[(s, j % EVR)] == r, (n, "an event of the previous call that its node does not hold")
                if s == SYN:
                    synth_seen = max(synth_seen, j)
            done_seen |= origin == DONE
        edge = first[k] + frames[k] - 1 + 3 - nslot
        if edge >= 0:
            continue                               # (inside this call: check_call)
        f = prev_len + edge
        if f >= 0:
            assert synth_seen >= max(j for j in range(len(pfirst)) if pfirst[j] <= f), (n, "ring slots the previous call still reads")
        elif older_call:
            assert done_seen, (n, "ring slots the call before the previous one still reads")


@pytest.mark.parametrize("lanes,depth", [(1, 1), (2, 2)])
def test_consecutive_calls_overlap_only_where_they_may(hostsim_lib, monkeypatch, lanes, depth):
    """nnn_batch_set_inputs_ready on the lanes schedule: after a real 34-frame call (and a one-frame call before it, so that there is
    a call two back), the next call's high-pass chain starts without waiting for the caller's stream.  48 frames on the longer ring:
    the first group's ring edge lies before the previous call, the second group's inside it; 96 frames: the fourth group's inside
    this call."""
    from nnnoiseless_amd import _ffi
    from nnnoiseless_amd.synthetic import make_streams
    bd, d = make(hostsim_lib, monkeypatch, 24, "lanes", lanes, "create")
    assert d == depth
    bd.set_inputs_ready(True)
    T = 34
    x = make_streams(5, S, 1 + T)
    out, vad = np.zeros_like(x), np.zeros((1 + T, S), np.float32)
    bd.process_device(_ffi.ptr(x), _ffi.ptr(out), _ffi.ptr(vad), 1, (1 + T) * 480, 480)
    head, pnodes = query(hostsim_lib, bd, T)
    assert head["pipe"] == 1 and head["fill"] == 1                      # (nothing to overlap with: the call before was not spread over streams)
    pfirst, _, pslot = check_call(head, pnodes, T, 24, depth)
    bd.process_device(_ffi.ptr(x[:, 1:]), _ffi.ptr(out[:, 1:]), _ffi.ptr(vad[1:]), T, (1 + T) * 480, 480)
    bd.synchronize()
    for n in (32, 33, 48):
        head, nodes = query(hostsim_lib, bd, n)
        first, frames, _ = check_call(head, nodes, n, 24, depth, early=True)
        check_boundary(head, nodes, first, frames, depth, 24, (pnodes, pfirst, pslot), T, True)
    head, nodes = query(hostsim_lib, bd, 31)                            # a short call does not overlap
    assert head["pipe"] == 0 and head["fill"] == 0
    head, nodes = query(hostsim_lib, bd, 96)                            # nor one longer than any before: growing its parameter table drains the batch
    assert head["pipe"] == 1 and head["fill"] == 1
    check_call(head, nodes, 96, 24, depth)
    bd.reset_streams([1])                                               # nor does a call behind a state call
    head, nodes = query(hostsim_lib, bd, 48)
    assert head["pipe"] == 1 and head["fill"] == 1
    check_call(head, nodes, 48, 24, depth)
