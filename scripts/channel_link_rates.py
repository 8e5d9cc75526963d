#!/usr/bin/env python3
"""What channel-linked gains cost and save (include/nnn_batch.h nnn_batch_set_channel_link), on one GPU under NNN_SCHED=seq, timed with HIP
events on the stream the calls are made on (a stream of the caller's: torch's DEFAULT stream has handle 0, which means "the batch's own
stream" to the library).

  process_device at 4096 x 1 (a max_group_frames = 1 batch ticking), 4096 x 24 and 65 536 x 24 frames per call: never linked; linked at 2
  channels (max); linked at 4 channels (max); and at 4096 x 24 the same 2-channel link through the triple analyze_device -> network_device
  -> the link formula in torch -> synthesize_device.
Every figure is microseconds per call: the median of --reps (3) repeats and their spread (max - min), which is the bar a difference has to
clear.

A library without the link entry points (the parent commit's, named by NNN_LIBRARY) runs the never-linked figures alone: this script once
per library and process, same box, same session; --merge puts the runs' files together (profiles/channel_link_rates.json, DESIGN.md
section 18).

usage: scripts/channel_link_rates.py [--reps K] [--json out.json]
       scripts/channel_link_rates.py --merge run1.json run2.json ... --json profiles/channel_link_rates.json"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # (the host's setting, as bench.py)
os.environ["NNN_SCHED"] = "seq"

SHAPES = (("4096x1", 4096, 1, 300, 1), ("4096x24", 4096, 24, 20, None), ("65536x24", 65536, 24, 5, None))   # name, streams, frames, calls per repeat, max_group_frames


def merge(files, out):
    """Per library, shape and figure: every run's median and spread, and the median of the runs' medians."""
    runs = [json.load(open(f)) for f in files]
    fig = {}
    for r in runs:
        for shape, by in r["us_per_call"].items():
            for how, v in by.items():
                fig.setdefault(r["library"], {}).setdefault(shape, {}).setdefault(how, []).append(
                    {"median": statistics.median(v), "spread": max(v) - min(v)})
    for lib in fig.values():
        for shape in lib.values():
            for how, v in shape.items():
                shape[how] = {"median": statistics.median(x["median"] for x in v), "runs": v}
    json.dump({"median_us_per_call": fig, "runs": runs}, open(out, "w"), indent=1)
    print(json.dumps(fig, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--merge", nargs="+")
    ap.add_argument("--json")
    a = ap.parse_args()
    if a.merge:
        return merge(a.merge, a.json)
    import torch
    torch.cuda.init()
    import nnnoiseless_amd as nn
    from nnnoiseless_amd import _ffi
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream()      # (not the default stream: its handle, 0, is the library's "the batch's own stream")
    sp = st.cuda_stream
    can_link = hasattr(nn.library().L, "nnn_batch_set_channel_link")
    res = {"library": os.environ.get("NNN_LIBRARY", "this tree"), "links": can_link, "sched": "seq", "us_per_call": {}}

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

    def link_torch(g, sil, channels, out):
        T, S = sil.shape
        mm = (sil == 0).reshape(T, S // channels, channels, 1)
        gg = g.reshape(T, S // channels, channels, 22)
        r = torch.where(mm, gg, torch.full_like(gg, -float("inf"))).amax(dim=2, keepdim=True)
        out.copy_(torch.where(mm, r, gg).reshape(T, S, 22))

    def run(x, y, S, T, n_calls, mgf, how):
        """us per call of T frames, a.reps repeats.  how: "unlinked", "link2", "link4" (the ordinary call) or "triple2"."""
        bd = nn.BatchDenoiser(S, max_group_frames=mgf) if mgf else nn.BatchDenoiser(S)
        bd.process_device(x.data_ptr(), y.data_ptr(), 0, T, T * 480, 480, sp)
        if how in ("link2", "link4"):
            bd.set_channel_link(int(how[-1]), "max")
        if how == "triple2":
            F, SIL = torch.zeros((T, S, 42), device=dev), torch.zeros((T, S), dtype=torch.int32, device=dev)
            g, v, gl = torch.zeros((T, S, 22), device=dev), torch.zeros((T, S), device=dev), torch.zeros((T, S, 22), device=dev)

            def loop():
                with torch.cuda.stream(st):
                    for _ in range(n_calls):
                        bd.analyze_device(x.data_ptr(), F.data_ptr(), SIL.data_ptr(), T, _ffi.PCM_F32, 1, T * 480, 480, sp)
                        bd.network_device(F.data_ptr(), SIL.data_ptr(), g.data_ptr(), v.data_ptr(), T, sp)
                        link_torch(g, SIL, 2, gl)
                        bd.synthesize_device(gl.data_ptr(), v.data_ptr(), y.data_ptr(), T, _ffi.PCM_F32, 1, T * 480, 480, hip_stream=sp)
        else:
            def loop():
                for _ in range(n_calls):
                    bd.process_device(x.data_ptr(), y.data_ptr(), 0, T, T * 480, 480, sp)
        out = [timed(loop, bd.synchronize) * 1000.0 / n_calls for _ in range(a.reps)]
        bd.synchronize()
        assert not bd.fault()
        return out

    for name, S, T, n_calls, mgf in SHAPES:
        x = torch.randn((S, T, 480), device=dev) * 1000.0
        y = torch.empty_like(x)
        r = {"unlinked": run(x, y, S, T, n_calls, mgf, "unlinked")}
        if can_link:
            r["link2"] = run(x, y, S, T, n_calls, mgf, "link2")
            r["link4"] = run(x, y, S, T, n_calls, mgf, "link4")
            if name == "4096x24":
                r["triple2"] = run(x, y, S, T, n_calls, mgf, "triple2")
        res["us_per_call"][name] = r
        print(json.dumps({name: r}), flush=True)
        del x, y
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
