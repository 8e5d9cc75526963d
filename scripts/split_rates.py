#!/usr/bin/env python3
"""What the split calls cost (include/nnn_batch.h "Split calls"), on one GPU, timed with HIP events on a stream of the caller's (not
torch's default stream: its handle, 0, means "the batch's own stream" to the library, and events on it would bracket nothing).

  analyze + synthesize of 24 frames with features and gains resident -- gains computed once beforehand, no network in between --
  against process_device of the same tree on the same input, at 4096 x 24 and 65 536 x 24, under NNN_SCHED=seq (one stream, in order:
  what a split pair always is), three repeats each
  the per-kernel split of both with nnn_batch_set_profiling: the kernels of the timing table, and for the pair the remainder of its
  event-timed total -- k_features, k_features_out and k_gains_in, which the table does not list

usage: scripts/split_rates.py [--streams N N ...] [--frames T] [--reps K] [--calls N] [--json out.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # (the host's setting, as bench.py)
os.environ["NNN_SCHED"] = "seq"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--json")
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import nnnoiseless_amd as nn
    from nnnoiseless_amd import _ffi
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream()
    sp = st.cuda_stream
    T = a.frames
    res = {"frames_per_call": T, "sched": "seq", "sizes": {}}

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

    for S in a.streams:
        x = torch.randn((S, T, 480), device=dev) * 1000.0
        y = torch.empty_like(x)
        F = torch.empty((T, S, 42), device=dev)
        SIL = torch.empty((T, S), dtype=torch.int32, device=dev)
        G = torch.rand((T, S, 22), device=dev)
        V = torch.rand((T, S), device=dev)
        torch.cuda.synchronize()

        def whole(bd):
            bd.process_device(x.data_ptr(), y.data_ptr(), 0, T, T * 480, 480, sp)

        def pair(bd):
            bd.analyze_device(x.data_ptr(), F.data_ptr(), SIL.data_ptr(), T, _ffi.PCM_F32, 1, T * 480, 480, sp)
            bd.synthesize_device(G.data_ptr(), V.data_ptr(), y.data_ptr(), T, _ffi.PCM_F32, 1, T * 480, 480, hip_stream=sp)

        r = {}
        for name, one in (("process_device", whole), ("analyze+synthesize", pair)):
            bd = nn.BatchDenoiser(S)

            def loop():
                for _ in range(a.calls):
                    one(bd)
            us = [timed(loop, bd.synchronize) * 1000.0 / a.calls for _ in range(a.reps)]
            # the per-kernel split: profiling waits after every call, so its sum is of kernels alone
            bd.set_profiling(True)
            bd.kernel_times()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(st)
            one(bd)
            e1.record(st)
            e1.synchronize()
            kt = {k: round(ms * 1000.0, 1) for k, (ms, n) in bd.kernel_times().items() if n}
            bd.set_profiling(False)
            bd.synchronize()
            assert not bd.fault()
            r[name] = {"us_per_call": [round(u, 1) for u in us], "M_frames_per_s": round(S * T / min(us), 2), "kernel_us": kt,
                       "profiled_call_us": round(e0.elapsed_time(e1) * 1000.0, 1)}
            if name != "process_device":
                r[name]["untimed_kernels_us"] = round(r[name]["profiled_call_us"] - sum(kt.values()), 1)   # k_features, k_features_out, k_gains_in (and gaps)
            del bd
        r["pair_over_whole"] = round(min(r["analyze+synthesize"]["us_per_call"]) / min(r["process_device"]["us_per_call"]), 3)
        res["sizes"][str(S)] = r
        print(json.dumps({str(S): r}))
        del x, y, F, SIL, G, V
        torch.cuda.empty_cache()
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
