#!/usr/bin/env python3
"""Rates of the per-stream state calls (include/nnn_batch.h nnn_batch_*_streams) on one GPU, timed with HIP events on the call's stream.

  whole-batch export / import, device to device, at --streams (default 65536) after one 48-frame call: ms per call, state bytes read +
  written per direction and the rate
  the reset of 4 streams per tick in a --tick-streams (default 4096) one-frame tick loop: the time it adds per tick

usage: scripts/stream_state_rates.py [--streams N] [--tick-streams N] [--reps K] [--json out.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # (the host's setting, as bench.py)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--tick-streams", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--ticks", type=int, default=400)
    ap.add_argument("--json")
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import nnnoiseless_amd as nn
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream()
    sp = st.cuda_stream
    res = {}

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        torch.cuda.synchronize()
        e0.record(st)
        for _ in range(reps):
            fn()
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    # ---- whole batch, device to device
    S, T = a.streams, 48
    x = torch.randn((S, T, 480), device=dev) * 1000.0
    y = torch.empty_like(x)
    bd = nn.BatchDenoiser(S)
    bd.process_device(x.data_ptr(), y.data_ptr(), 0, T, T * 480, 480, sp)
    rec = torch.empty((S, nn.STREAM_STATE_BYTES), dtype=torch.uint8, device=dev)
    idx = list(range(S))
    ms_exp = timed(lambda: bd.export_streams_device(idx, rec.data_ptr(), sp), a.reps)
    ms_imp = timed(lambda: bd.import_streams_device(idx, rec.data_ptr(), sp), a.reps)
    bd.synchronize()
    shape = nn.RnnModel.default().shape()
    gru = sum(shape[1:4]) * 4
    state = (1728 + 480 + 2 + 1 + 1 + 1 + 176 + 22) * 4 + gru                      # what export reads
    exp_bytes = S * (state + nn.STREAM_STATE_BYTES)
    dec = 720 * 4 * (1 + 4 / (bd.max_group_frames() * 3 + 4))                         # decimated values (+ their share of the mirror)
    imp_bytes = S * (nn.STREAM_STATE_BYTES + state + dec + 8 + 4)                       # + x_lp[0], hp_last, the check's header reads
    res["whole_batch"] = {"streams": S, "export_ms": ms_exp, "import_ms": ms_imp, "export_bytes": exp_bytes, "import_bytes": int(imp_bytes),
                          "export_TBps": exp_bytes / ms_exp / 1e9, "import_TBps": imp_bytes / ms_imp / 1e9}
    print(json.dumps(res["whole_batch"]))
    del bd, x, y, rec
    torch.cuda.empty_cache()

    # ---- tick loop with resets
    S = a.tick_streams
    xt = torch.randn((S, 1, 480), device=dev) * 1000.0
    yt = torch.empty_like(xt)
    tb = nn.BatchDenoiser(S, max_group_frames=1)
    ticks = a.ticks

    def loop(reset):
        for t in range(ticks):
            if reset:
                tb.reset_streams([(4 * t + k * 977) % S for k in range(4)])
            tb.process_device(xt.data_ptr(), yt.data_ptr(), 0, 1, 480, 480, sp)

    out = {}
    for name, reset in (("plain", False), ("reset4", True), ("plain_again", False), ("reset4_again", True)):
        out[name] = timed(lambda: loop(reset), 1) * 1000.0 / ticks
    plain = min(out["plain"], out["plain_again"])
    withr = min(out["reset4"], out["reset4_again"])
    res["tick"] = {"streams": S, "us_per_tick": out, "added_us_per_tick": withr - plain}
    print(json.dumps(res["tick"]))
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
