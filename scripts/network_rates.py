#!/usr/bin/env python3
"""What a network-only call costs (include/nnn_batch.h "Network-only calls"), on one GPU.

  the triple analyze_device -> network_device -> synthesize_device with the rows resident, against nnn_batch_process_device of this tree
  and of the PARENT commit's library (--parent-lib: a build of the commit before the network calls) and against the split pair alone
  (analyze + synthesize, gains computed beforehand: scripts/split_rates.py's shape), at 4096 x 1, 4096 x 24 and 65 536 x 24 (streams x
  frames per call), under NNN_SCHED=seq, timed with HIP events on the calls' own stream (not torch's default stream: its handle, 0, means
  "the batch's own stream" to the library) around `--calls` back-to-back calls; three repeats, the median and the spread (max - min)
  network_device alone against the RNN launch of a processing call of the same shape: the K_RNN entry of the timing table of one profiled
  process_device call with the unfused back end (nnn_batch_set_back_end(0): a one-frame call would otherwise run the fused k_back, which
  has no RNN launch of its own).  The library does not report which kernel a launch was; the name printed beside the entry is
  plan_group's rule for the built-in model on a lone batch (no other batch ticking beside it), restated here and labelled as such:
  k_rnn_wf for every group but a lone frame on 1024 or more 16-row blocks, k_rnn there, NNN_RNN_WF_MIN_G honoured.  NNN_RNN_ROWS
  (16 / 32) in the environment picks k_net's rows per block -- and forces k_rnn for the processing calls, which the output then says.

Each library runs in a child process of its own, one after the other in the same session; the parent's child is given the library through
NNN_LIBRARY.

usage: scripts/network_rates.py [--parent-lib libparent.so] [--shapes 4096x1 4096x24 65536x24] [--reps 3] [--calls N] [--json out.json] [--md]"""
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


def rnn_kernel_name(S, T):
    """The kernel behind the K_RNN entry of an unfused processing call of the built-in model on a lone batch, BY plan_group's RULE
    (nnn_batch_launch.hip) as it stands -- inferred, not read from the library: check it against plan_group when that changes."""
    if os.environ.get("NNN_RNN_ROWS") in ("16", "32"):
        return "k_rnn"
    blocks16 = (S + 63) // 64 * 4
    min_g = int(os.environ.get("NNN_RNN_WF_MIN_G", "0") or 0)
    if min_g <= 0:
        min_g = 2 if blocks16 >= 1024 else 1
    return "k_rnn_wf" if T >= min_g else "k_rnn"


def child(a):
    """One library (the one NNN_LIBRARY names, or this tree's): every shape; the network calls where the library has them."""
    import torch
    torch.cuda.init()
    import nnnoiseless_amd as nn
    from nnnoiseless_amd import _ffi
    has_net = hasattr(nn.library().L, "nnn_batch_network_device")
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
        F = torch.empty((T, S, 42), device=dev)
        SIL = torch.empty((T, S), dtype=torch.int32, device=dev)
        G = torch.rand((T, S, 22), device=dev)
        torch.cuda.synchronize()
        lay = (_ffi.PCM_F32, 1, T * 480, 480)

        def process(bd):
            bd.process_device(x.data_ptr(), y.data_ptr(), V.data_ptr(), T, T * 480, 480, sp)

        def pair(bd):
            bd.analyze_device(x.data_ptr(), F.data_ptr(), SIL.data_ptr(), T, *lay, sp)
            bd.synthesize_device(G.data_ptr(), V.data_ptr(), y.data_ptr(), T, *lay, hip_stream=sp)

        def triple(bd):
            bd.analyze_device(x.data_ptr(), F.data_ptr(), SIL.data_ptr(), T, *lay, sp)
            bd.network_device(F.data_ptr(), SIL.data_ptr(), G.data_ptr(), V.data_ptr(), T, sp)
            bd.synthesize_device(G.data_ptr(), V.data_ptr(), y.data_ptr(), T, *lay, hip_stream=sp)

        def network(bd):
            bd.network_device(F.data_ptr(), SIL.data_ptr(), G.data_ptr(), V.data_ptr(), T, sp)

        kinds = [("process_device", process)]
        if has_net:   # (pair first: it leaves real feature rows in F for the network-alone timing)
            kinds += [("split_pair", pair), ("triple", triple), ("network_device", network)]
        r = {"calls_per_repeat": calls}
        for name, one in kinds:
            bd = nn.BatchDenoiser(S)

            def loop():
                for _ in range(calls):
                    one(bd)
            us = [timed(loop, bd.synchronize) * 1000.0 / calls for _ in range(a.reps)]
            r[name] = {"us_per_call": [round(u, 1) for u in us], "median_us": round(statistics.median(us), 1), "spread_us": round(max(us) - min(us), 1)}
            bd.synchronize()
            assert not bd.fault()
            del bd
        if has_net:   # the RNN launch of an unfused processing call, from the timing table (profiling waits after every call)
            bd = nn.BatchDenoiser(S)
            bd.set_back_end(0)
            process(bd)
            bd.synchronize()
            bd.set_profiling(True)
            bd.kernel_times()
            for _ in range(a.reps):
                process(bd)
            ms, n = bd.kernel_times()["k_rnn"]
            bd.set_profiling(False)
            r["rnn_launch"] = {"kernel_by_plan_group_rule": rnn_kernel_name(S, T), "us_per_launch": round(ms * 1000.0 / max(n, 1), 1), "launches": int(n)}
            del bd
        out[shape] = r
        del x, y, V, F, SIL, G
        torch.cuda.empty_cache()
    print("NETWORK_RATES " + json.dumps(out))


def run_child(a, lib, limit):
    env = dict(os.environ)
    if lib:
        env["NNN_LIBRARY"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--calls", str(a.calls), "--shapes"] + a.shapes
    txt = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=limit).stdout
    return json.loads([ln for ln in txt.splitlines() if ln.startswith("NETWORK_RATES ")][-1][len("NETWORK_RATES "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["4096x1", "4096x24", "65536x24"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=0, help="calls per repeat (0: by shape)")
    ap.add_argument("--parent-lib", help="a build of the parent commit's library")
    ap.add_argument("--limit", type=int, default=240, help="seconds each child may take")
    ap.add_argument("--json")
    ap.add_argument("--md", action="store_true", help="print the table of DESIGN.md section 16")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    res = {"sched": "seq", "repeats": a.reps, "rnn_rows": os.environ.get("NNN_RNN_ROWS", "auto"), "this_tree": run_child(a, None, a.limit)}
    if a.parent_lib:
        res["parent"] = run_child(a, a.parent_lib, a.limit)
    for shape, r in res["this_tree"].items():
        line = {"shape": shape, **{k: r[k]["median_us"] for k in ("process_device", "split_pair", "triple", "network_device")},
                "rnn_launch": r["rnn_launch"]}
        if "parent" in res:
            line["parent_process_us"] = res["parent"][shape]["process_device"]["median_us"]
        print(json.dumps(line))
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)
    if a.md:
        ms = lambda d: f"{d['median_us']} ({d['spread_us']})"
        print("(us per call: median (max - min of the repeats))")
        print("| streams x frames | process_device, parent | process_device, this tree | split pair | triple | triple / parent | network_device alone | RNN launch of a processing call (kernel by plan_group's rule for a lone batch) |")
        print("|---|---|---|---|---|---|---|---|")
        for shape, r in res["this_tree"].items():
            p = res.get("parent", {}).get(shape, {}).get("process_device")
            print(f"| {shape.replace('x', ' x ')} | " + (ms(p) if p else "-") + f" | {ms(r['process_device'])} | {ms(r['split_pair'])} | {ms(r['triple'])} | " +
                  (f"{r['triple']['median_us'] / p['median_us']:.2f}" if p else "-") +
                  f" | {ms(r['network_device'])} | {r['rnn_launch']['us_per_launch']} ({r['rnn_launch']['kernel_by_plan_group_rule']}) |")


if __name__ == "__main__":
    main()
