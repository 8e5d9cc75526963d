#!/usr/bin/env python3
"""What the VAD gate costs (include/nnn_gate.h), on one GPU, timed with HIP events on the stream the calls are made
on (a stream of the caller's: torch's DEFAULT stream has handle 0, which means "the object's own stream" to the library).

  At 4096 and 65 536 streams, 24 frames a call, audio resident on the device as f32 [24][S][480] (the batch's layout), 16-byte aligned,
  d_open written, no live mask: nnn_gate_apply_device
    in place and out of place,
    with look-back R = 0, 2 and 8 on every stream,
    with every gate open (VAD 1), every gate muted (VAD 0, level 0), every gate closed at level 0.1 (VAD 0: read, multiply, write) and
    mixed (VAD in runs of random length around the threshold, level 0.1: open, closed and ramp frames side by side).
  The yardsticks, in the same run and alternating with them:
    copy      a device-to-device copy of the same audio bytes (3840 B per stream-frame read AND written): the floor of an out-of-place pass
    process   nnn_batch_process_device for the same frames, in place: the tick the gate is added to
  and a one-frame call at 4096 streams (in place, R = 2, mixed) against the one-frame process_device call.
  Every timed figure is the median of --reps (5) repeats with their spread (max - min), which is the bar a difference has to clear.

usage: scripts/gate_rates.py [--reps K] [--streams 4096 65536] [--calls 4] [--out profiles/gate_rates.txt]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # (the host's setting, as bench.py)

FRAME, T = 480, 24
STATES = {"open": (1.0, 0.0), "muted": (0.0, 0.0), "closed": (0.0, 0.1), "mixed": (None, 0.1)}   # name: (VAD, level)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--streams", nargs="+", type=int, default=[4096, 65536])
    ap.add_argument("--calls", type=int, default=4, help="calls inside one timed window")
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import torch
    torch.cuda.init()
    import nnnoiseless_amd as nn
    from nnnoiseless_amd.gate import VadGate
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream()
    sp = st.cuda_stream
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(fn):
        """ms between two events on the calls' stream around fn() (after one unmeasured fn() and a full wait)."""
        with torch.cuda.stream(st):
            fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn()
            e1.record(st)
            e1.synchronize()
            torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def stat(v):
        return f"{statistics.median(v):.4g} (spread {max(v) - min(v):.2g})"

    def mixed_vad(S, frames, seed):
        rng = np.random.default_rng(seed)
        on = rng.random(S) < 0.5
        v = np.zeros((frames, S), np.float32)
        for t in range(frames):
            on ^= rng.random(S) < 0.15
            v[t] = np.where(on, 0.9, 0.1)
        return v

    say(f"# scripts/gate_rates.py: {T} frames a call, {a.calls} calls a window, median of {a.reps} (spread = max - min)")
    for S in a.streams:
        n = T * S * FRAME
        gen = torch.Generator(device=dev).manual_seed(S)
        src, dst = torch.empty(n, device=dev), torch.empty(n, device=dev)
        src.uniform_(-32768.0, 32767.0, generator=gen)
        opn = torch.empty(T * S, dtype=torch.uint8, device=dev)
        vads = {k: (torch.full((T, S), v, device=dev) if v is not None else torch.from_numpy(mixed_vad(S, T, S)).to(dev)) for k, (v, _) in STATES.items()}
        gates = {}
        for R in (0, 2, 8):
            for k, (_, level) in STATES.items():
                g = VadGate(S, 8)
                g.set_params(0.5, 2, R, level)
                gates[(R, k)] = g
        bd = nn.BatchDenoiser(S)
        bvad = torch.empty((T, S), device=dev)
        torch.cuda.synchronize()

        def call(R, k, inplace):
            g, v = gates[(R, k)], vads[k]
            d = src if inplace else dst

            def fn():
                for _ in range(a.calls):
                    g.apply_device(src.data_ptr(), d.data_ptr(), v.data_ptr(), T, FRAME, S * FRAME, d_open=opn.data_ptr(), hip_stream=sp)
            return fn

        def copy():
            for _ in range(a.calls):
                dst.copy_(src)

        def process():
            for _ in range(a.calls):
                bd.process_device(dst.data_ptr(), dst.data_ptr(), bvad.data_ptr(), T, FRAME, S * FRAME, sp)

        # (the in-place calls run on `src`: at level 0.1 it decays towards zero over the repeats, which changes no instruction executed)
        kinds = {"copy": copy, "process": process}
        for inplace in (False, True):
            for R in (0, 2, 8):
                for k in STATES:
                    kinds[f"{'in place' if inplace else 'out of place'} R={R} {k}"] = call(R, k, inplace)
        ms = {k: [] for k in kinds}
        for _ in range(a.reps):   # (alternating, so that a drift of the clock or of the machine's other load lands on all of them)
            for k, fn in kinds.items():
                ms[k].append(timed(fn) / a.calls)
        m = {k: statistics.median(v) for k, v in ms.items()}
        frames, gb = T * S, n * 4 / 1e9
        say(f"{S} streams ({frames} stream-frames, {gb:.3f} GB of audio a call):")
        say(f"  {'copy':26s} {stat(ms['copy'])} ms per call   {2 * gb / (m['copy'] * 1e-3):8.1f} GB/s read + written")
        say(f"  {'process':26s} {stat(ms['process'])} ms per call   {frames / (m['process'] * 1e-3) / 1e6:8.1f} M stream-frames/s")
        for k in kinds:
            if k not in ("copy", "process"):
                say(f"  {k:26s} {stat(ms[k])} ms per call   {m[k] / m['copy']:6.3f} of the copy   {100 * m[k] / m['process']:6.2f} % of process")
        say("  " + json.dumps({"streams": S, "ms_per_call": ms}))
        if S == a.streams[0]:
            g1 = VadGate(S, 8)
            g1.set_params(0.5, 2, 2, 0.1)
            v1 = torch.from_numpy(mixed_vad(S, 64, 1)).to(dev)
            step = [0]

            def gate_tick():
                for _ in range(a.calls):
                    step[0] = (step[0] + 1) % 64
                    g1.apply_device(src.data_ptr(), src.data_ptr(), v1[step[0]].data_ptr(), 1, FRAME, S * FRAME, d_open=opn.data_ptr(), hip_stream=sp)

            def tick():
                for _ in range(a.calls):
                    bd.process_device(dst.data_ptr(), dst.data_ptr(), bvad.data_ptr(), 1, FRAME, S * FRAME, sp)

            one = {"gate": [], "process": []}
            for _ in range(a.reps):
                one["gate"].append(timed(gate_tick) / a.calls)
                one["process"].append(timed(tick) / a.calls)
            mg, mp = statistics.median(one["gate"]), statistics.median(one["process"])
            say(f"  one frame, {S} streams, in place, R=2, mixed: gate {stat(one['gate'])} ms, process {stat(one['process'])} ms: {100 * mg / mp:.2f} % of the tick")
            say("  " + json.dumps({"streams": S, "one_frame_ms": one}))
            g1.close()
        for g in gates.values():
            g.close()
        bd.close()
        del src, dst, opn, vads, bvad
        torch.cuda.empty_cache()
    if a.out:
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
