#!/usr/bin/env python3
"""What held streams cost and save (include/nnn_batch.h nnn_batch_hold_streams), on one GPU, timed with HIP events on the stream the calls are made on
(a stream of the caller's: handing the library torch's DEFAULT stream, whose handle is 0, means "the batch's own stream" to it -- include/nnn_batch.h --
and events on the default stream then bracket nothing).

  a --tick-streams (4096) batch ticking one frame per call and a --group-streams (16384) batch in 24-frame calls, with 0, 1/2 and 3/4 of
  the streams held: as whole tiles of 64, as the same number of scattered 16-stream blocks (every second / three of four blocks of every
  tile), and -- expected to save nothing -- as scattered single streams (one or two of every four); three repeats each
  the two ends every held configuration is measured against: the full batch with nothing held, and a batch of only the live stream count
  hold + resume of 4, 64 and 4096 streams between the ticks of the tick batch: the time a pair adds to a tick

A library without the hold entry points (the parent commit's, named by NNN_LIBRARY) runs the two ends alone: that is how the figures of
DESIGN.md section 13 were taken -- this script once per library, same box, same session.

usage: scripts/hold_rates.py [--tick-streams N] [--group-streams N] [--reps K] [--json out.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # (the host's setting, as bench.py)


def held_sets(S):
    tiles = S // 64
    blocks = [list(range(16 * b, 16 * b + 16)) for b in range(S // 16)]
    flat = lambda bs: [s for b in bs for s in b]
    return {
        "tiles_1/2": list(range(0, tiles // 2 * 64)),
        "tiles_3/4": list(range(0, tiles * 3 // 4 * 64)),
        "blocks_1/2": flat(b for i, b in enumerate(blocks) if i % 2 == 0),
        "blocks_3/4": flat(b for i, b in enumerate(blocks) if i % 4 != 3),
        "singles_1/4": list(range(0, S, 4)),
        "singles_1/2": list(range(0, S, 2)),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tick-streams", type=int, default=4096)
    ap.add_argument("--group-streams", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ticks", type=int, default=300)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--json")
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import nnnoiseless_amd as nn
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream()      # (not the default stream: its handle, 0, is the library's "the batch's own stream")
    sp = st.cuda_stream
    can_hold = hasattr(nn.library().L, "nnn_batch_hold_streams")
    res = {"library": os.environ.get("NNN_LIBRARY", "this tree"), "holds": can_hold}

    def timed(fn, sync):
        """ms between two events on the calls' stream around fn() (after one unmeasured fn() and a full wait)."""
        fn()
        sync()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        e1.synchronize()
        sync()
        return e0.elapsed_time(e1)

    def run(S, T, n_calls, mgf, held):
        """us per call of T frames, a.reps repeats, with `held` held (None: nothing, and no mask ever made)."""
        x = torch.randn((S, T, 480), device=dev) * 1000.0
        y = torch.empty_like(x)
        bd = nn.BatchDenoiser(S, max_group_frames=mgf) if mgf else nn.BatchDenoiser(S)
        bd.process_device(x.data_ptr(), y.data_ptr(), 0, T, T * 480, 480, sp)
        if held:
            bd.hold_streams(held)

        def loop():
            for _ in range(n_calls):
                bd.process_device(x.data_ptr(), y.data_ptr(), 0, T, T * 480, 480, sp)
        out = [timed(loop, bd.synchronize) * 1000.0 / n_calls for _ in range(a.reps)]
        bd.synchronize()
        assert not bd.fault()
        return out

    for name, S, T, n_calls, mgf in (("tick", a.tick_streams, 1, a.ticks, 1), ("group24", a.group_streams, 24, a.calls, None)):
        r = {"streams": S, "frames_per_call": T, "us_per_call": {}}
        r["us_per_call"]["full"] = run(S, T, n_calls, mgf, None)
        for frac, live in (("1/2", S // 2), ("1/4", S // 4)):
            r["us_per_call"]["batch_of_live_" + frac] = run(live, T, n_calls, mgf, None)
        if can_hold:
            for key, held in held_sets(S).items():
                r["us_per_call"]["held_" + key] = run(S, T, n_calls, mgf, held)
        res[name] = r
        print(json.dumps({name: r}))

    if can_hold:   # hold + resume between ticks
        S = a.tick_streams
        xt = torch.randn((S, 1, 480), device=dev) * 1000.0
        yt = torch.empty_like(xt)
        tb = nn.BatchDenoiser(S, max_group_frames=1)
        tb.process_device(xt.data_ptr(), yt.data_ptr(), 0, 1, 480, 480, sp)
        out = {}
        for n in (0, 4, 64, S):
            idx = [(k * 977) % S for k in range(n)] if n < S else list(range(S))

            def loop():
                for _ in range(a.ticks):
                    if n:
                        tb.hold_streams(idx)
                        tb.resume_streams(idx)
                    tb.process_device(xt.data_ptr(), yt.data_ptr(), 0, 1, 480, 480, sp)
            out[str(n)] = min(timed(loop, tb.synchronize) for _ in range(a.reps)) * 1000.0 / a.ticks
        res["hold_resume_pair"] = {"streams": S, "us_per_tick": out, "added_us_per_tick": {k: v - out["0"] for k, v in out.items() if k != "0"}}
        print(json.dumps(res["hold_resume_pair"]))
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
