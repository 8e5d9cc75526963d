#!/usr/bin/env python3
"""What the conference mixer costs (include/nnn_mix.h), on one GPU, timed with HIP events on the stream the calls are
made on (a stream of the caller's: torch's DEFAULT stream has handle 0, which means "the object's own stream" to the library).

  At 65 536 x 24, 4096 x 24 and 4096 x 1 (streams x frames a call), audio resident on the device as f32 [T][S][480] (the batch's layout),
  16-byte aligned, d_talk given, d_heard written, no live mask, steady gains (no ramp frame): nnn_mix_apply_device with
    rooms of 2, of 8 and of 64, everybody audible,
    rooms of 64 with 3 audible members each,
    rooms of 4096 (one room at 4096 streams) with 3 audible members each.
  The yardsticks, in the same run and alternating with them:
    copy    a device-to-device copy of the same audio bytes (1920 B per stream-frame read AND written)
    torch   the same mix as a torch expression: the terms in float64, index_add_ into a [T][rooms][480] total, gather, subtract, cast
            (no stated summation order: index_add_ uses atomics)
  and the bytes the rule needs -- every audible stream-frame read once, every stream-frame written once -- against the copy's bytes.
  Every timed figure is the median of --reps (5) repeats with their spread (max - min), which is the bar a difference has to clear.

usage: scripts/mix_rates.py [--reps K] [--sizes 65536x24 4096x24 4096x1] [--calls 4] [--out profiles/mix_rates.txt]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # (the host's setting, as bench.py)

FRAME = 480
CASES = {"rooms of 2, all audible": (2, None), "rooms of 8, all audible": (8, None), "rooms of 64, all audible": (64, None),
         "rooms of 64, 3 audible": (64, 3), "rooms of 4096, 3 audible": (4096, 3)}   # name: (members, audible members or None = all)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", nargs="+", default=["65536x24", "4096x24", "4096x1"])
    ap.add_argument("--calls", type=int, default=4, help="calls inside one timed window")
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import torch
    torch.cuda.init()
    from nnnoiseless_amd.mix import ConferenceMixer
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

    say(f"# scripts/mix_rates.py: {a.calls} calls a window, median of {a.reps} (spread = max - min); GPU_MAX_HW_QUEUES={os.environ['GPU_MAX_HW_QUEUES']}, "
        f"{torch.cuda.get_device_name(0)}")
    for size in a.sizes:
        S, T = (int(v) for v in size.split("x"))
        n = T * S * FRAME
        gen = torch.Generator(device=dev).manual_seed(S + T)
        src, dst = torch.empty(n, device=dev), torch.empty(n, device=dev)
        src.uniform_(-8192.0, 8191.0, generator=gen)
        heard = torch.empty(T * S, dtype=torch.int32, device=dev)
        x3 = src.view(T, S, FRAME)
        mixers, talks, rooms, audible = {}, {}, {}, {}
        for k, (members, aud) in CASES.items():
            room = (np.arange(S) // min(members, S)).astype(np.int32)
            talk = np.ones((T, S), np.uint8) if aud is None else np.tile((np.arange(S) % min(members, S) < aud).astype(np.uint8), (T, 1))
            m = ConferenceMixer(S)
            m.set_rooms(room)
            mixers[k], talks[k], rooms[k] = m, torch.from_numpy(talk).to(dev), torch.from_numpy(room.astype(np.int64)).to(dev)
            audible[k] = int(talk.sum())
        torch.cuda.synchronize()

        def call(k):
            m, tk = mixers[k], talks[k]

            def fn():
                for _ in range(a.calls):
                    m.apply_device(src.data_ptr(), dst.data_ptr(), T, FRAME, S * FRAME, FRAME, S * FRAME, d_talk=tk.data_ptr(), d_heard=heard.data_ptr(),
                                   hip_stream=sp)
            return fn

        def torch_mix(k):
            tk, room = talks[k], rooms[k]
            n_rooms = int(room.max()) + 1

            def fn():
                for _ in range(a.calls):
                    c = x3.double() * tk.double()[:, :, None]
                    tot = torch.zeros((T, n_rooms, FRAME), dtype=torch.float64, device=dev).index_add_(1, room, c)
                    dst.view(T, S, FRAME).copy_((tot[:, room] - c).float())
            return fn

        def copy():
            for _ in range(a.calls):
                dst.copy_(src)

        kinds = {"copy": copy}
        for k in CASES:
            kinds[k] = call(k)
            kinds["torch: " + k] = torch_mix(k)
        ms = {k: [] for k in kinds}
        for _ in range(a.reps):   # (alternating, so that a drift of the clock or of the machine's other load lands on all of them)
            for k, fn in kinds.items():
                ms[k].append(timed(fn) / a.calls)
        med = {k: statistics.median(v) for k, v in ms.items()}
        gb = n * 4 / 1e9
        say(f"{S} streams x {T} frames ({T * S} stream-frames, {gb:.4f} GB of audio a call):")
        say(f"  {'copy':34s} {stat(ms['copy'])} ms per call   {2 * gb / (med['copy'] * 1e-3):8.1f} GB/s read + written")
        for k in CASES:
            need = (audible[k] + T * S) * FRAME * 4 / 1e9
            say(f"  {k:34s} {stat(ms[k])} ms per call   {med[k] / med['copy']:6.3f} of the copy   bytes needed {need / (2 * gb):5.3f} of the copy's"
                f"   {need / (med[k] * 1e-3):8.1f} GB/s of them   torch {stat(ms['torch: ' + k])} ms = {med['torch: ' + k] / med[k]:6.1f} x")
        say("  " + json.dumps({"streams": S, "frames": T, "ms_per_call": ms}))
        for m in mixers.values():
            m.close()
        del src, dst, heard, x3, talks, rooms
        torch.cuda.empty_cache()
    if a.out:
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
