#!/usr/bin/env python3
"""What gain floors cost and save (include/nnn_batch.h nnn_batch_set_gain_floor), on one GPU, timed with HIP events on the stream the calls
are made on (a stream of the caller's: torch's DEFAULT stream has handle 0, which means "the batch's own stream" to the library).

  tick      a --tick-streams (4096) batch of max_group_frames = 1 ticking one frame per process_device call: nothing floored; pattern P on
            the batch (stream 4k off, 4k + 1 one scalar 10^(-18/20), 4k + 2 a 22-band ramp 0.05 .. 0.95, 4k + 3 1.0, the tests' pattern);
            and the same floors through the triple analyze_device -> network_device -> torch.maximum -> synthesize_device per tick
  group24   a --group-streams (16384) batch in 24-frame calls: nothing floored, and P set
Every figure is microseconds per call, --reps (3) repeats; the medians are what DESIGN.md section 17 quotes.

A library without the floor entry points (the parent commit's, named by NNN_LIBRARY) runs the unfloored figures alone: this script once per
library and process, alternating, same box, same session; --merge puts the runs' files together.

usage: scripts/gain_floor_rates.py [--tick-streams N] [--group-streams N] [--reps K] [--json out.json]
       scripts/gain_floor_rates.py --merge run1.json run2.json ... --json profiles/gain_floor_rates.json"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # (the host's setting, as bench.py)


def merge(files, out):
    """Per library and figure: the median of each run's (process's) median, and those medians themselves (their spread is the bar)."""
    runs = [json.load(open(f)) for f in files]
    med = {}
    for r in runs:
        for shape in ("tick", "group24"):
            for k, v in r.get(shape, {}).get("us_per_call", {}).items():
                med.setdefault(r["library"], {}).setdefault(shape + "_" + k, []).append(statistics.median(v))
    med = {lib: {k: {"median": statistics.median(v), "runs": v} for k, v in figs.items()} for lib, figs in med.items()}
    json.dump({"median_us_per_call": med, "runs": runs}, open(out, "w"), indent=1)
    print(json.dumps(med, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tick-streams", type=int, default=4096)
    ap.add_argument("--group-streams", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ticks", type=int, default=300)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--merge", nargs="+")
    ap.add_argument("--json")
    a = ap.parse_args()
    if a.merge:
        return merge(a.merge, a.json)
    import numpy as np
    import torch
    torch.cuda.init()
    import nnnoiseless_amd as nn
    from nnnoiseless_amd import _ffi
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream()      # (not the default stream: its handle, 0, is the library's "the batch's own stream")
    sp = st.cuda_stream
    can_floor = hasattr(nn.library().L, "nnn_batch_set_gain_floor")
    res = {"library": os.environ.get("NNN_LIBRARY", "this tree"), "floors": can_floor}

    def pattern(S):
        p = np.zeros((S, 22), np.float32)
        p[1::4], p[2::4], p[3::4] = 10.0 ** (-18.0 / 20.0), np.linspace(0.05, 0.95, 22), 1.0
        return p

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

    def run(S, T, n_calls, mgf, how):
        """us per call of T frames, a.reps repeats.  how: "unfloored", "floored" (P set, the ordinary call) or "triple" (P through the
        split calls and torch.maximum)."""
        x = torch.randn((S, T, 480), device=dev) * 1000.0
        y = torch.empty_like(x)
        bd = nn.BatchDenoiser(S, max_group_frames=mgf) if mgf else nn.BatchDenoiser(S)
        bd.process_device(x.data_ptr(), y.data_ptr(), 0, T, T * 480, 480, sp)
        if how == "floored":
            bd.set_gain_floor(range(S), pattern(S))
            assert bd.num_floored() == S - (S + 3) // 4
        if how == "triple":
            P = torch.from_numpy(pattern(S)).to(dev)
            F, SIL = torch.zeros((T, S, 42), device=dev), torch.zeros((T, S), dtype=torch.int32, device=dev)
            g, v, gf = torch.zeros((T, S, 22), device=dev), torch.zeros((T, S), device=dev), torch.zeros((T, S, 22), device=dev)

            def loop():
                with torch.cuda.stream(st):
                    for _ in range(n_calls):
                        bd.analyze_device(x.data_ptr(), F.data_ptr(), SIL.data_ptr(), T, _ffi.PCM_F32, 1, T * 480, 480, sp)
                        bd.network_device(F.data_ptr(), SIL.data_ptr(), g.data_ptr(), v.data_ptr(), T, sp)
                        torch.maximum(g, P, out=gf)
                        bd.synthesize_device(gf.data_ptr(), v.data_ptr(), y.data_ptr(), T, _ffi.PCM_F32, 1, T * 480, 480, hip_stream=sp)
        else:
            def loop():
                for _ in range(n_calls):
                    bd.process_device(x.data_ptr(), y.data_ptr(), 0, T, T * 480, 480, sp)
        out = [timed(loop, bd.synchronize) * 1000.0 / n_calls for _ in range(a.reps)]
        bd.synchronize()
        assert not bd.fault()
        return out

    for name, S, T, n_calls, mgf in (("tick", a.tick_streams, 1, a.ticks, 1), ("group24", a.group_streams, 24, a.calls, None)):
        r = {"streams": S, "frames_per_call": T, "us_per_call": {}}
        r["us_per_call"]["unfloored"] = run(S, T, n_calls, mgf, "unfloored")
        if can_floor:
            r["us_per_call"]["floored"] = run(S, T, n_calls, mgf, "floored")
            if name == "tick":
                r["us_per_call"]["triple"] = run(S, T, n_calls, mgf, "triple")
        res[name] = r
        print(json.dumps({name: r}))
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
