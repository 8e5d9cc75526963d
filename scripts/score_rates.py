#!/usr/bin/env python3
"""What the scorer costs (include/nnn_score.h), on one GPU, timed with HIP events on the stream the calls are made
on (a stream of the caller's: torch's DEFAULT stream has handle 0, which means "the object's own stream" to the library).

  At 4096 and 65 536 streams, 24 frames a call, reference and test signal resident on the device as f32 [24][S][480] (the batch's
  layout), no mask, frame sums into the object's own table:
    aligned   nnn_score_accumulate_device at delay 0, both signals 16-byte aligned
    delay480  the same at delay 480 (the denoiser's latency: the window is the previous frame, or the history)
    delay1    the same at delay 1 (the reference window begins one float before a 16-byte boundary and crosses two frames)
    dword     delay 0 with both signals starting one float behind a 16-byte boundary (4-byte alignment only)
  and the yardsticks, in the same run and alternating with them:
    copy      a device-to-device copy of the same two arrays: the machine's achieved rate for this many bytes (read AND written)
    torch     the same four sums per stream-frame as a torch float64 expression: what a user would write without this call (its order
              of summation is torch's, not the header's)
  Every timed figure is the median of --reps (5) repeats with their spread (max - min), which is the bar a difference has to clear.

usage: scripts/score_rates.py [--reps K] [--streams 4096 65536] [--calls 4] [--out profiles/score_rates.txt]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # (the host's setting, as bench.py)

FRAME, T = 480, 24
DENOISER = (76.5e6, 79.4e6)   # frames/s at 65 536 streams (README.md), not measured again here


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--streams", nargs="+", type=int, default=[4096, 65536])
    ap.add_argument("--calls", type=int, default=4, help="calls inside one timed window")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    from nnnoiseless_amd import score
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

    say(f"# scripts/score_rates.py: {T} frames a call, {a.calls} calls a window, median of {a.reps} (spread = max - min)")
    for S in a.streams:
        n = T * S * FRAME
        gen = torch.Generator(device=dev).manual_seed(S)
        buf = [torch.empty(n + 4, device=dev) for _ in range(2)]
        for b in buf:
            b.uniform_(-32768.0, 32767.0, generator=gen)
        dst = [torch.empty(n, device=dev) for _ in range(2)]
        al = [b[:n] for b in buf]                       # 16-byte aligned
        od = [b[1:n + 1] for b in buf]                  # one float behind
        scorers = {"aligned": (score.Scorer(S), al, 0), "delay480": (score.Scorer(S), al, 480), "delay1": (score.Scorer(S), al, 1),
                   "dword": (score.Scorer(S), od, 0)}
        for sc, _, d in scorers.values():
            sc.set_delay(None, d)
        torch.cuda.synchronize()

        def call(name):
            sc, (r, y), _ = scorers[name]

            def fn():
                for _ in range(a.calls):
                    sc.accumulate_device(r.data_ptr(), y.data_ptr(), T, FRAME, S * FRAME, hip_stream=sp)
            return fn

        def copy():
            for _ in range(a.calls):
                dst[0].copy_(al[0])
                dst[1].copy_(al[1])

        def in_torch():
            for _ in range(a.calls):
                r, y = al[0].view(T, S, FRAME).double(), al[1].view(T, S, FRAME).double()
                e = r - y
                torch.stack([(r * r).sum(-1), (y * y).sum(-1), (r * y).sum(-1), (e * e).sum(-1)], dim=-1)

        kinds = {k: call(k) for k in scorers}
        kinds["copy"], kinds["torch"] = copy, in_torch
        ms = {k: [] for k in kinds}
        for _ in range(a.reps):   # (alternating, so that a drift of the clock or of the machine's other load lands on all of them)
            for k, fn in kinds.items():
                ms[k].append(timed(fn) / a.calls)
        frames = T * S
        gb = 2 * n * 4 / 1e9      # the two signals, read once
        say(f"{S} streams ({frames} stream-frames, {gb:.3f} GB of samples a call):")
        for k in kinds:
            med = statistics.median(ms[k])
            extra = f"{gb / (med * 1e-3):8.1f} GB/s of samples read" if k != "copy" else f"{2 * gb / (med * 1e-3):8.1f} GB/s read + written"
            say(f"  {k:9s} {stat(ms[k])} ms per call   {frames / (med * 1e-3) / 1e6:9.1f} M stream-frames/s   {extra}")
        m = {k: statistics.median(v) for k, v in ms.items()}
        say(f"  aligned / copy = {m['aligned'] / m['copy']:.3f}; delay480 / aligned = {m['delay480'] / m['aligned']:.3f}; delay1 / aligned = "
            f"{m['delay1'] / m['aligned']:.3f}; dword / aligned = {m['dword'] / m['aligned']:.3f}; torch / aligned = {m['torch'] / m['aligned']:.2f}")
        den = [frames / r * 1e3 for r in DENOISER]
        say(f"  the denoiser's own time for these frames at {DENOISER[0] / 1e6:.1f}-{DENOISER[1] / 1e6:.1f} M frames/s (README.md, 65 536 streams; not "
            f"re-measured): {den[1]:.3g}-{den[0]:.3g} ms; the aligned call is {100 * m['aligned'] / den[0]:.1f}-{100 * m['aligned'] / den[1]:.1f} % of it")
        say("  " + json.dumps({"streams": S, "ms_per_call": ms}))
        for sc, _, _ in scorers.values():
            sc.close()
        del buf, dst, al, od
        torch.cuda.empty_cache()
    if a.out:
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
