#!/usr/bin/env python3
"""What the rate adapter costs (include/nnn_rate.h), on one GPU under NNN_SCHED=seq, timed with HIP events on the stream the calls are
made on (a stream of the caller's: torch's DEFAULT stream has handle 0, which means "the batch's own stream" to the library).

  Shapes: 4096 streams x one 10 ms tick on a max_group_frames = 1 batch, and 4096 streams x 24 frames' worth of samples, each at 16 kHz
  and at 44.1 kHz.
  Figures, microseconds per call:
    adapter       nnn_rate_process_device: source-rate samples in, source-rate samples out
    plain48       nnn_batch_process_device of the same number of frames, 48 kHz in and out (what the adapter adds to is this)
    composition   what a host writes without the adapter: nnn_resampler_process_device up, a torch repack of carried + new samples
                  into frames, nnn_batch_process_device, nnn_resampler_process_device at ratio 48000 / rate down
    tables_us     host microseconds per adapter call spent building schedule tables, [up-leg, down-leg] (0 where the key recurs)
Every timed figure is the median of --reps (3) repeats and their spread (max - min), which is the bar a difference has to clear.

A library without the adapter (the parent commit's, named by NNN_LIBRARY) runs plain48 and composition alone: this script once per
library and process, same box, same session; --merge puts the runs' files together (profiles/rate_rates.json).

usage: scripts/rate_rates.py [--reps K] [--shapes 4096x1 ...] [--rates 16000 ...] [--figures plain48 composition adapter] [--json out.json]
       scripts/rate_rates.py --merge run1.json run2.json ... --json profiles/rate_rates.json"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # (the host's setting, as bench.py)
os.environ["NNN_SCHED"] = "seq"

SHAPES = (("4096x1", 4096, 1, 200, 1), ("4096x24", 4096, 24, 20, None))   # name, streams, frames, calls per repeat, max_group_frames
RATES = (16000, 44100)


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
                shape[how] = {"median": statistics.median(x["median"] for x in v), "spread": max(x["spread"] for x in v), "runs": v}
    json.dump({"median_us_per_call": fig, "runs": runs}, open(out, "w"), indent=1)
    print(json.dumps(fig, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--merge", nargs="+")
    ap.add_argument("--json")
    ap.add_argument("--shapes", nargs="+", default=[s[0] for s in SHAPES], help="of " + " ".join(s[0] for s in SHAPES))
    ap.add_argument("--rates", nargs="+", type=int, default=list(RATES))
    ap.add_argument("--figures", nargs="+", default=["plain48", "composition", "adapter"])
    a = ap.parse_args()
    if a.merge:
        return merge(a.merge, a.json)
    import torch
    torch.cuda.init()
    import nnnoiseless_amd as nn
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream()      # (not the default stream: its handle, 0, is the library's "the batch's own stream")
    sp = st.cuda_stream
    lib = nn.library()
    L = lib.L
    has_rate = hasattr(L, "nnn_rate_create")
    res = {"library": os.path.basename(os.environ.get("NNN_LIBRARY", "this tree")), "adapter": has_rate, "sched": "seq", "us_per_call": {}, "tables_us_per_call": {}}

    def timed(fn, sync):
        """ms between two events on the calls' stream around fn() (after one unmeasured fn() and a full wait)."""
        torch.cuda.synchronize()   # (the buffers were filled on torch's default stream)
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

    def batch(S, mgf):
        return nn.BatchDenoiser(S, max_group_frames=mgf) if mgf else nn.BatchDenoiser(S)

    def run_plain(S, T, n_calls, mgf):
        bd = batch(S, mgf)
        x = torch.randn((S, T * 480), device=dev) * 1000.0
        y, vad = torch.empty_like(x), torch.empty((T, S), device=dev)

        def loop():
            for _ in range(n_calls):
                bd.process_device(x.data_ptr(), y.data_ptr(), vad.data_ptr(), T, T * 480, 480, sp)
        out = [timed(loop, bd.synchronize) * 1000.0 / n_calls for _ in range(a.reps)]
        assert not bd.fault()
        return out

    def run_adapter(S, T, n_calls, mgf, rate):
        from nnnoiseless_amd.pcm import RateAdapter
        bd = batch(S, mgf)
        n_in = T * rate // 100
        ra = RateAdapter(bd, float(rate), n_in)
        cap, capf = ra.max_output(n_in), ra.max_frames(n_in)
        x = torch.randn((S, n_in), device=dev) * 1000.0
        y, vad = torch.empty((S, cap), device=dev), torch.empty((capf, S), device=dev)
        frames = [0]

        def loop():
            for _ in range(n_calls):
                frames[0] += ra.process_device(x.data_ptr(), n_in, n_in, y.data_ptr(), cap, cap, vad.data_ptr(), capf, hip_stream=sp)[1]
        loop()   # (the first calls build the recurring tables)
        bd.synchronize()
        frames[0] = 0
        t0 = ra.tables_built()
        out = [timed(loop, bd.synchronize) * 1000.0 / n_calls for _ in range(a.reps)]
        t1 = ra.tables_built()
        calls = n_calls * 2 * a.reps
        assert not bd.fault() and abs(frames[0] - calls * T) <= 1, (frames[0], calls * T)   # a call of T frames' worth completes T frames
        tables = {"built_per_call": [(t1[0][k] - t0[0][k]) / calls for k in range(2)], "host_us_per_call": [(t1[1][k] - t0[1][k]) / calls for k in range(2)]}
        ra.close()
        return out, tables

    def run_composition(S, T, n_calls, mgf, rate):
        """The glue a host writes today, on the same stream: up, repack into frames behind the carried samples, denoise, down."""
        bd = batch(S, mgf)
        n_in = T * rate // 100
        up = L.nnn_resampler_create(S, rate / 48000.0, 0)
        dn = L.nnn_resampler_create(S, 48000.0 / rate, 0)
        cap_up = L.nnn_resampler_max_output(up, n_in)
        TF = (479 + cap_up) // 480
        cap_dn = L.nnn_resampler_max_output(dn, TF * 480)
        x = torch.randn((S, n_in), device=dev) * 1000.0
        u = torch.empty((S, cap_up), device=dev)
        buf = torch.zeros((S, TF * 480 + 480), device=dev)
        o48 = torch.empty_like(buf)   # (process_device has ONE stream stride for input and output: the rows of both are buf's)
        y, vad = torch.empty((S, cap_dn), device=dev), torch.empty((TF, S), device=dev)
        carried = [0]
        n = C.c_long(0)

        def loop():
            with torch.cuda.stream(st):
                for _ in range(n_calls):
                    lib.check(L.nnn_resampler_process_device(up, x.data_ptr(), n_in, n_in, u.data_ptr(), cap_up, cap_up, C.byref(n), sp))
                    total = carried[0] + n.value
                    buf[:, carried[0]:total] = u[:, :n.value]
                    Tn = total // 480
                    if Tn:
                        bd.process_device(buf.data_ptr(), o48.data_ptr(), vad.data_ptr(), Tn, buf.shape[1], 480, sp)
                        rem = total - Tn * 480
                        if rem:
                            buf[:, :rem] = buf[:, Tn * 480:total].clone()
                        carried[0] = rem
                    else:
                        carried[0] = total
                    lib.check(L.nnn_resampler_process_device(dn, o48.data_ptr(), Tn * 480, o48.shape[1], y.data_ptr(), cap_dn, cap_dn, C.byref(n), sp))
        out = [timed(loop, bd.synchronize) * 1000.0 / n_calls for _ in range(a.reps)]
        assert not bd.fault()
        L.nnn_resampler_destroy(up)
        L.nnn_resampler_destroy(dn)
        return out

    for name, S, T, n_calls, mgf in SHAPES:
        if name not in a.shapes:
            continue
        plain = run_plain(S, T, n_calls, mgf) if "plain48" in a.figures else None
        for rate in a.rates:
            key = f"{name}@{rate}"
            r = {}
            if plain:
                r["plain48"] = plain
            if "composition" in a.figures:
                r["composition"] = run_composition(S, T, n_calls, mgf, rate)
            if has_rate and "adapter" in a.figures:
                r["adapter"], res["tables_us_per_call"][key] = run_adapter(S, T, n_calls, mgf, rate)
            res["us_per_call"][key] = r
            print(json.dumps({key: r, "tables": res["tables_us_per_call"].get(key)}), flush=True)
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
