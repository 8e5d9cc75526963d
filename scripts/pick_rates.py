#!/usr/bin/env python3
"""What the talker picker costs (include/nnn_pick.h), on one GPU, timed with HIP events on the stream the calls are
made on (a stream of the caller's: torch's DEFAULT stream has handle 0, which means "the object's own stream" to the library).

  At 65 536 x 24, 4096 x 24 and 4096 x 1 (streams x frames a call), audio resident on the device as f32 [T][S][480] (the batch's layout),
  16-byte aligned, d_open given, d_talk, d_dominant and d_level written, no live mask, k 3, decay 0.875, stick 4: nnn_pick_select_device with
    rooms of 2, of 8 and of 64, every gate open,
    rooms of 64 with 3 open gates each,
    rooms of 4096 (one room at 4096 streams) with 12 open gates each.
  The yardsticks, in the same run and alternating with them:
    copy    a device-to-device copy of the same audio bytes (1920 B per stream-frame read AND written)
    torch   the same selection as a torch expression: the samples squared and summed in float64, a top-k per room over the open gates
            (no level carried, no hysteresis, no pins, no stated summation order)
  and the bytes the rule needs -- every open stream-frame read once -- against the copy's bytes.
  The payoff, in rooms of 64 with every gate open: select + ConferenceMixer.apply(talk = picked) against ConferenceMixer.apply(talk = open).
  Every timed figure is the median of --reps (5) repeats with their spread (max - min), which is the bar a difference has to clear.

  The split of a call into its two kernels comes from a kernel trace, taken in a run of its own:
    rocprofv3 --kernel-trace -d DIR -- python scripts/pick_rates.py --dispatch-only     (each case 1 + --calls times, nothing else)
    python scripts/pick_rates.py --from-trace DIR/.../*_kernel_trace.csv                 (the calls told apart by their order)

usage: scripts/pick_rates.py [--reps K] [--sizes 65536x24 4096x24 4096x1] [--calls 4] [--out profiles/pick_rates.txt]"""
import argparse
import csv
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # (the host's setting, as bench.py)

FRAME = 480
K = 3
CASES = {"rooms of 2, all open": (2, None), "rooms of 8, all open": (8, None), "rooms of 64, all open": (64, None),
         "rooms of 64, 3 open": (64, 3), "rooms of 4096, 12 open": (4096, 12)}   # name: (members, open members or None = all)
PAYOFF = "rooms of 64, all open"


def from_trace(path, sizes, calls):
    """The kernel trace of a --dispatch-only run: per size and case 1 + calls pairs of (k_pick_level, k_pick_rank), in the order made."""
    rows = list(csv.DictReader(open(path)))
    col = lambda name: next(c for c in rows[0] if name.lower() in c.lower())   # noqa: E731
    kn, t0, t1 = col("kernel_name"), col("start_timestamp"), col("end_timestamp")
    rows = sorted((r for r in rows if "k_pick_level" in r[kn] or "k_pick_rank" in r[kn]), key=lambda r: int(r[t0]))
    assert len(rows) == len(sizes) * len(CASES) * (1 + calls) * 2, (len(rows), "dispatches of the picker's kernels in the trace")
    at = 0
    print(f"# scripts/pick_rates.py --from-trace: kernel times of {calls} calls a case (the first, unmeasured one left out), median, in ms")
    for size in sizes:
        print(f"{size}:")
        for k in CASES:
            mine = rows[at + 2:at + 2 * (1 + calls)]
            at += 2 * (1 + calls)
            ms = {"k_pick_level": [], "k_pick_rank": []}
            for r in mine:
                ms["k_pick_level" if "k_pick_level" in r[kn] else "k_pick_rank"].append((int(r[t1]) - int(r[t0])) * 1e-6)
            print(f"  {k:26s} k_pick_level {statistics.median(ms['k_pick_level']):.4g}   k_pick_rank {statistics.median(ms['k_pick_rank']):.4g}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", nargs="+", default=["65536x24", "4096x24", "4096x1"])
    ap.add_argument("--calls", type=int, default=4, help="calls inside one timed window")
    ap.add_argument("--out")
    ap.add_argument("--dispatch-only", action="store_true", help="each case 1 + --calls times and nothing else: for a kernel trace")
    ap.add_argument("--from-trace", help="a kernel trace (csv) of a --dispatch-only run with the same --sizes and --calls: print the split")
    a = ap.parse_args()
    if a.from_trace:
        return from_trace(a.from_trace, a.sizes, a.calls)
    import numpy as np
    import torch
    torch.cuda.init()
    from nnnoiseless_amd.mix import ConferenceMixer
    from nnnoiseless_amd.pick import TalkerPicker
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

    say(f"# scripts/pick_rates.py: {a.calls} calls a window, median of {a.reps} (spread = max - min); GPU_MAX_HW_QUEUES={os.environ['GPU_MAX_HW_QUEUES']}, "
        f"{torch.cuda.get_device_name(0)}")
    for size in a.sizes:
        S, T = (int(v) for v in size.split("x"))
        n = T * S * FRAME
        gen = torch.Generator(device=dev).manual_seed(S + T)
        src, dst = torch.empty(n, device=dev), torch.empty(n, device=dev)
        src.uniform_(-8192.0, 8191.0, generator=gen)
        src.view(T, S, FRAME).mul_(torch.rand((T, S, 1), device=dev, generator=gen) * 4 + 0.25)   # (levels differ: the talkers change)
        talk = torch.empty(T * S, dtype=torch.uint8, device=dev)
        dom = torch.empty(T * S, dtype=torch.int32, device=dev)
        lvl = torch.empty(T * S, dtype=torch.float64, device=dev)
        x3 = src.view(T, S, FRAME)
        pickers, opens, n_open, members_of = {}, {}, {}, {}
        for k, (members, op) in CASES.items():
            members = min(members, S)
            room = (np.arange(S) // members).astype(np.int32)
            o = np.ones((T, S), np.uint8) if op is None else np.tile((np.arange(S) % members < op).astype(np.uint8), (T, 1))
            p = TalkerPicker(S)
            p.set_rooms(room), p.set_policy(K, 0.875, 4.0)
            pickers[k], opens[k], n_open[k], members_of[k] = p, torch.from_numpy(o).to(dev), int(o.sum()), members
        mixer = ConferenceMixer(S)
        mixer.set_rooms((np.arange(S) // min(64, S)).astype(np.int32))
        torch.cuda.synchronize()

        def select(k):
            p, o = pickers[k], opens[k]

            def fn():
                for _ in range(a.calls):
                    p.select_device(src.data_ptr(), talk.data_ptr(), T, FRAME, S * FRAME, d_open=o.data_ptr(), d_dominant=dom.data_ptr(),
                                    d_level=lvl.data_ptr(), hip_stream=sp)
            return fn

        if a.dispatch_only:
            for k in CASES:
                for _ in range(1 + a.calls):
                    pickers[k].select_device(src.data_ptr(), talk.data_ptr(), T, FRAME, S * FRAME, d_open=opens[k].data_ptr(), d_dominant=dom.data_ptr(),
                                             d_level=lvl.data_ptr(), hip_stream=sp)
                torch.cuda.synchronize()
            continue

        def torch_pick(k):
            o, m = opens[k], members_of[k]

            def fn():
                for _ in range(a.calls):
                    e = (x3.double() ** 2).sum(dim=2) * o.double() - (1 - o.double())          # closed gates below every energy
                    top = e.view(T, S // m, m).topk(min(K, m), dim=2)
                    tk = torch.zeros((T, S // m, m), dtype=torch.uint8, device=dev).scatter_(2, top.indices, (top.values >= 0).to(torch.uint8))
                    talk.view(T, S // m, m).copy_(tk)
            return fn

        def mix(tk):
            def fn():
                for _ in range(a.calls):
                    mixer.apply_device(src.data_ptr(), dst.data_ptr(), T, FRAME, S * FRAME, FRAME, S * FRAME, d_talk=tk.data_ptr(), hip_stream=sp)
            return fn

        def pick_and_mix():
            p, o = pickers[PAYOFF], opens[PAYOFF]
            for _ in range(a.calls):
                p.select_device(src.data_ptr(), talk.data_ptr(), T, FRAME, S * FRAME, d_open=o.data_ptr(), hip_stream=sp)
                mixer.apply_device(src.data_ptr(), dst.data_ptr(), T, FRAME, S * FRAME, FRAME, S * FRAME, d_talk=talk.data_ptr(), hip_stream=sp)

        def copy():
            for _ in range(a.calls):
                dst.copy_(src)

        kinds = {"copy": copy}
        for k in CASES:
            kinds[k] = select(k)
            if S % members_of[k] == 0:
                kinds["torch: " + k] = torch_pick(k)
        kinds["mix, talk = open"], kinds["select + mix, talk = picked"] = mix(opens[PAYOFF]), pick_and_mix
        ms = {k: [] for k in kinds}
        for _ in range(a.reps):   # (alternating, so that a drift of the clock or of the machine's other load lands on all of them)
            for k, fn in kinds.items():
                ms[k].append(timed(fn) / a.calls)
        med = {k: statistics.median(v) for k, v in ms.items()}
        gb = n * 4 / 1e9
        say(f"{S} streams x {T} frames ({T * S} stream-frames, {gb:.4f} GB of audio a call):")
        say(f"  {'copy':34s} {stat(ms['copy'])} ms per call   {2 * gb / (med['copy'] * 1e-3):8.1f} GB/s read + written")
        for k in CASES:
            need = n_open[k] * FRAME * 4 / 1e9
            tor = f"torch {stat(ms['torch: ' + k])} ms = {med['torch: ' + k] / med[k]:6.1f} x" if "torch: " + k in ms else "torch: not measured"
            say(f"  {k:34s} {stat(ms[k])} ms per call   {med[k] / med['copy']:6.3f} of the copy   bytes needed {need / (2 * gb):5.3f} of the copy's"
                f"   {need / (med[k] * 1e-3):8.1f} GB/s of them   {tor}")
        a_, b_ = "mix, talk = open", "select + mix, talk = picked"
        say(f"  rooms of 64, all open, k = {K}: {a_} {stat(ms[a_])} ms per call;  {b_} {stat(ms[b_])} ms per call = {med[b_] / med[a_]:.3f} of it")
        say("  " + json.dumps({"streams": S, "frames": T, "ms_per_call": ms}))
        for p in pickers.values():
            p.close()
        mixer.close()
        del src, dst, talk, dom, lvl, x3, opens
        torch.cuda.empty_cache()
    if a.out:
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
