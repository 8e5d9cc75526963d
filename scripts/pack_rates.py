#!/usr/bin/env python3
"""What the file packer costs (include/nnn_pack.h), on one GPU under NNN_SCHED=seq, timed with HIP events on the stream the calls are made
on (a stream of the caller's: torch's DEFAULT stream has handle 0, which means "the batch's own stream" to the library).

  At 4096 and 65 536 streams, int16 in and out:
    packer    useful stream-frames per second of one packer run over 2 x n_streams mono files with a spread of lengths (4 to 60 frames,
              uniform), longest first, arenas resident on the device, at step_frames 24 and 8; with each run's summary
    plain     stream-frames per second of the batch's own nnn_batch_process_pcm_device over the same number of frames per stream, in
              equal-length rows and 24-frame calls: the parent's code path, the yardstick
    kernels   k_pack_in and k_pack_out alone (nnn_pack_debug_kernels: full 24-frame steps on every slot), GB/s of the bytes each moves
              (int16 on the arena side, f32 on the staging side: 6 bytes an element)
Every timed figure is the median of --reps (3) repeats with their spread (max - min), which is the bar a difference has to clear.

usage: scripts/pack_rates.py [--reps K] [--streams 4096 65536] [--steps 24 8] [--json profiles/pack_rates.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # (the host's setting, as bench.py)
os.environ["NNN_SCHED"] = "seq"

FRAME = 480


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--streams", nargs="+", type=int, default=[4096, 65536])
    ap.add_argument("--steps", nargs="+", type=int, default=[24, 8], help="step_frames of the packer runs")
    ap.add_argument("--json")
    a = ap.parse_args()
    import numpy as np
    import torch
    torch.cuda.init()
    import nnnoiseless_amd as nn
    from nnnoiseless_amd import _ffi, pcm
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream()      # (not the default stream: its handle, 0, is the library's "the batch's own stream")
    sp = st.cuda_stream

    def timed(fn, sync):
        """ms between two events on the calls' stream around fn() (after one unmeasured fn() and a full wait)."""
        torch.cuda.synchronize()
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

    def stat(v):
        return {"median": statistics.median(v), "spread": max(v) - min(v), "runs": v}

    res = {"sched": "seq", "format": "int16 in and out", "by_streams": {}}
    for S in a.streams:
        rng = np.random.default_rng(S)
        frames = np.sort(rng.integers(4, 61, 2 * S))[::-1]            # longest first
        n = frames * FRAME + rng.integers(0, FRAME, frames.size)       # a partial frame behind each
        in_off = np.concatenate([[0], np.cumsum(n)])
        out_off = np.concatenate([[0], np.cumsum((frames - 1) * FRAME)])
        vad_off = np.concatenate([[0], np.cumsum(frames)])
        x = (torch.randn(int(in_off[-1]), device=dev) * 3000.0).to(torch.int16)
        y = torch.zeros(int(out_off[-1]), device=dev, dtype=torch.int16)
        vad = torch.zeros(int(vad_off[-1]), device=dev)
        table = (_ffi.PackFile * frames.size)()
        for i in range(frames.size):
            table[i] = _ffi.PackFile(int(in_off[i]), int(n[i]), int(out_off[i]), int(vad_off[i]))
        bd = nn.BatchDenoiser(S)
        r = {"files": int(frames.size)}
        for step in a.steps:   # (padding is at most step - 1 frames a file: short files favour short steps, the kernels long ones)
            fp = pcm.FilePacker(bd, 1, step)
            summary = {}

            def run():
                summary.update(fp.run_device(x.data_ptr(), x.numel(), pcm.PCM_I16, y.data_ptr(), y.numel(), pcm.PCM_I16, vad.data_ptr(), vad.numel(), table, sp))
            ms = [timed(run, bd.synchronize) for _ in range(a.reps)]
            assert not bd.fault()
            useful = summary["useful"]
            r[f"step{step}"] = {"summary": dict(summary), "packer_ms": stat(ms), "packer_useful_frames_per_s": stat([useful / (t * 1e-3) for t in ms]),
                                "useful_share_of_launched": useful / summary["launched"]}
            fp.close()
        fp = pcm.FilePacker(bd, 1, 24)
        # the two kernels alone: full 24-frame steps on every slot, 20 launches
        reps, T = 20, 24
        dense_in = (torch.randn(S * T * FRAME, device=dev) * 3000.0).to(torch.int16)
        dense_out = torch.zeros(S * T * FRAME, device=dev, dtype=torch.int16)
        for which, name in ((0, "k_pack_in"), (1, "k_pack_out")):
            t = [timed(lambda: fp.debug_kernels(which, dense_in.data_ptr(), pcm.PCM_I16, dense_out.data_ptr(), pcm.PCM_I16, T, reps, sp), bd.synchronize)
                 for _ in range(a.reps)]
            r[name + "_GB_per_s"] = stat([reps * S * T * FRAME * 6 / (v * 1e-3) / 1e9 for v in t])
        fp.close()
        bd.close()
        del x, y, vad, dense_in, dense_out
        # the yardstick: the batch's own int16 call over the same number of frames per stream, 24 frames a call
        calls = max(1, round(useful / S / T))
        bd = nn.BatchDenoiser(S)
        xi = (torch.randn((S, T * FRAME), device=dev) * 3000.0).to(torch.int16)
        yi, v = torch.empty_like(xi), torch.empty((T, S), device=dev)

        def plain():
            for _ in range(calls):
                bd.process_pcm_device(xi.data_ptr(), yi.data_ptr(), v.data_ptr(), T, pcm.PCM_I16, 1, T * FRAME, FRAME, hip_stream=sp)
        ms = [timed(plain, bd.synchronize) for _ in range(a.reps)]
        assert not bd.fault()
        bd.close()
        r["plain_calls"], r["plain_ms"] = calls, stat(ms)
        r["plain_frames_per_s"] = stat([calls * T * S / (t * 1e-3) for t in ms])
        for step in a.steps:
            r[f"step{step}"]["packer_over_plain"] = r[f"step{step}"]["packer_useful_frames_per_s"]["median"] / r["plain_frames_per_s"]["median"]
        res["by_streams"][str(S)] = r
        print(json.dumps({str(S): r}), flush=True)
        del xi, yi, v
        torch.cuda.empty_cache()
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
