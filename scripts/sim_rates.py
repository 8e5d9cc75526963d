#!/usr/bin/env python3
"""What the noise simulator costs (include/nnn_sim.h), on one GPU, timed with HIP events on the stream the calls are
made on (a stream of the caller's: torch's DEFAULT stream has handle 0, which means "the object's own stream" to the library).

  At 4096 and 16 384 triples, 24 frames a call, arenas of 2^26 int16 samples each resident on the device, every triple reading
  consecutive frames from a random (mostly odd) element on, random_params in force:
    k_sim     k_sim alone (nnn_sim_debug_kernel: 24-frame launches into the staging): us per launch and per frame, rows/s
    sim       nnn_sim_process_device: rows/s from offsets to rows
    train     nnn_train_process_device over the same signals, already mixed and resident as f32 (made by nnn_sim_signals_device): the
              parent's code path, the yardstick, measured in the same run and alternating with `sim`
  Every timed figure is the median of --reps (5) repeats with their spread (max - min), which is the bar a difference has to clear.
  The bus-inclusive figure of the parent's host path (scripts/train_host_rate.py, pinned buffers, 4096 triples x 48 frames:
  8.61 M rows/s, profiles/r2_b_host_boundary_pcie.txt) is printed beside them; it is not measured again here.

usage: scripts/sim_rates.py [--reps K] [--triples 4096 16384] [--calls 10] [--out profiles/sim_rates.txt]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # (the host's setting, as bench.py)

FRAME, T = 480, 24
HOST_PATH_PINNED = 8.61e6   # rows/s, profiles/r2_b_host_boundary_pcie.txt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--triples", nargs="+", type=int, default=[4096, 16384])
    ap.add_argument("--calls", type=int, default=10, help="calls (launches for k_sim) inside one timed window")
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import torch
    torch.cuda.init()
    from nnnoiseless_amd import training
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream()
    sp = st.cuda_stream
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(fn):
        """ms between two events on the calls' stream around fn() (after one unmeasured fn() and a full wait)."""
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
        return f"{statistics.median(v):.3g} (spread {max(v) - min(v):.2g})"

    elems = 1 << 26
    gen = torch.Generator(device=dev).manual_seed(1)
    arenas = [(torch.randn(elems, device=dev, generator=gen) * amp).to(torch.int16) for amp in (3000.0, 300.0)]
    say(f"# scripts/sim_rates.py: {T} frames a call, {a.calls} calls a window, median of {a.reps} (spread = max - min); arenas 2 x {elems} int16")
    for S in a.triples:
        rng = np.random.default_rng(S)
        tf = training.TrainingFeatures(S)
        sim = training.NoiseSimulator(tf)
        sim.adopt_device(training.ARENA_SIGNAL, arenas[0].data_ptr(), elems, keep=arenas[0])
        sim.adopt_device(training.ARENA_NOISE, arenas[1].data_ptr(), elems, keep=arenas[1])
        sim.set_params(None, training.random_params(rng, S))
        offs = []
        for _ in range(2):
            base = rng.integers(0, elems - T * FRAME, S)
            offs.append(torch.from_numpy((base[None, :] + FRAME * np.arange(T)[:, None]).astype(np.int64)).to(dev))
        rows = torch.empty((T, S, training.ROW_WIDTH), device=dev)
        audio = torch.empty((3, S, T * FRAME), device=dev)
        cut, vad = torch.empty((T, S), device=dev, dtype=torch.int32), torch.empty((T, S), device=dev)
        sim.signals_device(offs[0].data_ptr(), offs[1].data_ptr(), audio[0].data_ptr(), audio[1].data_ptr(), audio[2].data_ptr(), cut.data_ptr(),
                           vad.data_ptr(), T, T * FRAME, FRAME, sp)
        torch.cuda.synchronize()

        def k_sim():
            sim.debug_kernel(offs[0].data_ptr(), offs[1].data_ptr(), T, a.calls, sp)

        def with_sim():
            for _ in range(a.calls):
                sim.process_device(offs[0].data_ptr(), offs[1].data_ptr(), rows.data_ptr(), T, sp)

        def train_only():
            for _ in range(a.calls):
                tf.process_device(audio[0].data_ptr(), audio[1].data_ptr(), audio[2].data_ptr(), cut.data_ptr(), vad.data_ptr(), rows.data_ptr(), T,
                                  T * FRAME, FRAME, sp)

        ms = {"k_sim": [], "sim": [], "train": []}
        for _ in range(a.reps):   # (alternating, so that a drift of the clock or of the box's other load lands on all three)
            ms["sim"].append(timed(with_sim))
            ms["train"].append(timed(train_only))
            ms["k_sim"].append(timed(k_sim))
        assert not sim.fault()
        n = a.calls * T * S
        rate = {k: [n / (t * 1e-3) / 1e6 for t in v] for k, v in ms.items()}
        us = [t * 1e3 / a.calls for t in ms["k_sim"]]
        say(f"{S} triples:")
        say(f"  k_sim alone          {stat(us)} us per {T}-frame launch, {statistics.median(us) / T:.3g} us per frame; {stat(rate['k_sim'])} M rows/s")
        say(f"  sim   (offsets->rows) {stat(rate['sim'])} M rows/s   [{stat([t / a.calls for t in ms['sim']])} ms per call]")
        say(f"  train (resident f32)  {stat(rate['train'])} M rows/s   [{stat([t / a.calls for t in ms['train']])} ms per call]")
        ratio = statistics.median(rate["sim"]) / statistics.median(rate["train"])
        say(f"  sim / train = {ratio:.3f}; k_sim's time / train's time = {statistics.median(ms['k_sim']) / statistics.median(ms['train']):.3f}; "
            f"host path with the bus (pinned, not re-measured) {HOST_PATH_PINNED / 1e6:.2f} M rows/s")
        say("  " + json.dumps({"triples": S, "ms": ms}))
        sim.close()
        tf.close()
        del rows, audio, cut, vad, offs
        torch.cuda.empty_cache()
    if a.out:
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
