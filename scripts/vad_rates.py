#!/usr/bin/env python3
"""What a VAD-only call costs (include/nnn_batch.h "VAD-only calls") against the ordinary call it replaces, on one GPU.

  nnn_batch_vad_device and nnn_batch_process_device of this tree, and nnn_batch_process_device of the PARENT commit's library (--parent-lib:
  a build of the commit before the VAD calls), at 4096 x 1, 4096 x 24 and 65 536 x 24 (streams x frames per call), under NNN_SCHED=seq,
  timed with HIP events on the calls' own stream (not torch's default stream: its handle, 0, means "the batch's own stream" to the library)
  around `--calls` back-to-back calls; three repeats, the median and the spread (max - min) of the repeats
  the per-kernel split of one profiled VAD call: the timed kernels of the front (k_hp, k_lpc, k_pitch) and the remainder -- k_fft_feat,
  k_features and k_vad, which the timing table does not list

Each library runs in a child process of its own, one after the other in the same session; the parent's child is given the library through
NNN_LIBRARY.  The bar (printed as `faster_than_parent`): the VAD call's median is below the parent's process_device median by more than
the larger of the two spreads.

usage: scripts/vad_rates.py [--parent-lib libparent.so] [--shapes 4096x1 4096x24 65536x24] [--reps 3] [--calls N] [--json out.json] [--md]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # (the host's setting, as bench.py)
os.environ["NNN_SCHED"] = "seq"


def child(a):
    """One library (the one NNN_LIBRARY names, or this tree's): every shape, process_device and -- where the library has it -- vad_device."""
    import torch
    torch.cuda.init()
    import nnnoiseless_amd as nn
    from nnnoiseless_amd import _ffi
    has_vad = hasattr(nn.library().L, "nnn_batch_vad_device")
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream()
    sp = st.cuda_stream

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

    out = {}
    for shape in a.shapes:
        S, T = (int(v) for v in shape.split("x"))
        calls = a.calls or (200 if S * T <= 4096 else 20 if S * T <= 4096 * 24 else 5)
        x = torch.randn((S, T, 480), device=dev) * 1000.0
        y = torch.empty_like(x)
        V = torch.empty((T, S), device=dev)
        torch.cuda.synchronize()
        kinds = [("process_device", lambda bd: bd.process_device(x.data_ptr(), y.data_ptr(), V.data_ptr(), T, T * 480, 480, sp))]
        if has_vad:
            kinds.append(("vad_device", lambda bd: bd.vad_device(x.data_ptr(), V.data_ptr(), T, _ffi.PCM_F32, 1, T * 480, 480, sp)))
        r = {"calls_per_repeat": calls}
        for name, one in kinds:
            bd = nn.BatchDenoiser(S)

            def loop():
                for _ in range(calls):
                    one(bd)
            us = [timed(loop, bd.synchronize) * 1000.0 / calls for _ in range(a.reps)]
            r[name] = {"us_per_call": [round(u, 1) for u in us], "median_us": round(statistics.median(us), 1), "spread_us": round(max(us) - min(us), 1)}
            if name == "vad_device":   # the per-kernel split: profiling waits after every call, so its sum is of kernels alone
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
                r[name]["kernel_us"] = kt
                r[name]["fft_feat_features_vad_us"] = round(e0.elapsed_time(e1) * 1000.0 - sum(kt.values()), 1)   # (and the gaps between launches)
            bd.synchronize()
            assert not bd.fault()
            del bd
        out[shape] = r
        del x, y, V
        torch.cuda.empty_cache()
    print("VAD_RATES " + json.dumps(out))


def run_child(a, lib, limit):
    env = dict(os.environ)
    if lib:
        env["NNN_LIBRARY"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--calls", str(a.calls), "--shapes"] + a.shapes
    txt = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=limit).stdout
    return json.loads([ln for ln in txt.splitlines() if ln.startswith("VAD_RATES ")][-1][len("VAD_RATES "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["4096x1", "4096x24", "65536x24"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=0, help="calls per repeat (0: by shape)")
    ap.add_argument("--parent-lib", help="a build of the parent commit's library")
    ap.add_argument("--limit", type=int, default=240, help="seconds each child may take")
    ap.add_argument("--json")
    ap.add_argument("--md", action="store_true", help="print the table of DESIGN.md section 15")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    res = {"sched": "seq", "repeats": a.reps, "this_tree": run_child(a, None, a.limit)}
    if a.parent_lib:
        res["parent"] = run_child(a, a.parent_lib, a.limit)
    for shape, r in res["this_tree"].items():
        v = r["vad_device"]
        line = {"shape": shape, "vad_us": v["median_us"], "vad_spread_us": v["spread_us"], "process_us": r["process_device"]["median_us"]}
        if "parent" in res:
            p = res["parent"][shape]["process_device"]
            line.update(parent_process_us=p["median_us"], parent_spread_us=p["spread_us"],
                        faster_than_parent=bool(p["median_us"] - v["median_us"] > max(p["spread_us"], v["spread_us"])))
            r["faster_than_parent"] = line["faster_than_parent"]
        print(json.dumps(line))
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)
    if a.md:
        print("(us per call: median (max - min of the repeats))")
        print("| streams x frames | process_device, parent (us) | process_device, this tree (us) | vad_device (us) | vad / parent | k_hp + k_lpc | k_pitch | k_fft_feat + k_features + k_vad |")
        print("|---|---|---|---|---|---|---|---|")
        for shape, r in res["this_tree"].items():
            v, p = r["vad_device"], res.get("parent", {}).get(shape, {}).get("process_device")
            k = v["kernel_us"]
            print(f"| {shape.replace('x', ' x ')} | " + (f"{p['median_us']} ({p['spread_us']})" if p else "-") +
                  f" | {r['process_device']['median_us']} ({r['process_device']['spread_us']}) | {v['median_us']} ({v['spread_us']}) | " +
                  (f"{v['median_us'] / p['median_us']:.2f}" if p else "-") +
                  f" | {round(k.get('k_hp', 0) + k.get('k_lpc', 0), 1)} | {k.get('k_pitch', 0)} | {v['fft_feat_features_vad_us']} |")


if __name__ == "__main__":
    main()
