#!/usr/bin/env python
"""bench.py -- 480-sample frames/sec of the batched process_frame path on MI355X.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--config C] [--full] [--dump-outputs DIR]

`--gpus N` with N > 1 may be started either way: under torch.distributed.run (RANK / LOCAL_RANK / WORLD_SIZE in the
environment, what the driver does) or as a plain `python bench.py --gpus N`, in which case this script re-executes itself
under `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1`.  One rank per GPU, rank r
on device LOCAL_RANK; the line is refused (exit 2) when the ranks actually seen (an all-reduce of ones over RCCL) differ
from --gpus.

A "step" is one pass of the hot path over one batch: every stream of this rank's shard advances by `--frames-per-step`
frames (default 48 = 0.48 s of audio per stream per call).  Workloads are BASELINE.json's configs (0-based index):

  --config 2  (default)  65536 concurrent streams on one GPU, built-in model, GRU as batched MFMA GEMM
                         (configs[2]: the largest single-GPU configuration, the headline `value`)
  --config 1             4096 concurrent mono streams per GPU, built-in model           (configs[1])
  --config 3             262144 streams sharded over the node = 32768 per GPU at 8 GPUs (configs[3]; per-GPU share fixed)
  --config 4             65536 streams, custom model (--model, default tests/golden/sh.rnn: GregorR's rnnoise-models
                         "sh" converted to .rnn)                                        (configs[4])
  --config 0             the reference's CPU-runnable case (testing.raw through the CPU oracle; no GPU, plumbing only)

Synthetic 48 kHz sine + noise per stream, inputs resident in HBM before the timed region.  Streams are
independent, so ranks shard them with no data-path collective (weak scaling); the only collective aggregates the result.

Prints ONE JSON line on rank 0 (contract in the task statement).  A plain run sets up, warms up, times the K steps of the
headline workload and prints the line; everything else it can measure runs only with --full, which adds these objects:
  tick          the same workload at one frame per call (the default batch, and a batch sized for ticks)
  roofline      dominant kernel: algorithmic bytes per launch / its average duration measured live with HIP events on
                the launch stream (a second, event-instrumented pass over the same workload)
  cpu_baseline  the CPU oracle (scalar C port of the reference, f32 FFT) on the host's cores: the synthetic mix at
                several thread counts (best reported, scaling table alongside) and the reference's own bench shape
                (benches/sin.rs: 100 frames of a 440 Hz sine, fresh state per iteration, one thread).  The genuine Rust
                reference cannot be built here (no cargo), hence kind "port".
  also          (default N=1 run only) the same measurement on configs[1] and configs[4], so the driver's line carries them
                (each timed for at least 0.5 s)
  default_semantics  (default N=1 run only) the headline workload under the library's default call ordering
  host_boundary (default N=1 run only) the headline workload through the host-buffer entry point: PCIe-inclusive, never `value`
The --no-* options leave out single parts of a --full run.

--dump-outputs DIR writes what the timed path computed in its last timed step, as a caller receives it, before anything else
touches the buffers: DIR/out.npy (float32 [streams, frames, 480], the denoised audio) and DIR/vad.npy (float32 [streams, frames])
of a fixed sample of rank 0's streams (the same streams for the same arguments; at most 64 MB in all).  The inputs are seeded,
so two builds run with the same arguments can be compared output for output.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
# The bench is the HOST of the library: the HIP runtime's hardware-queue count is the host's setting (the library and the
# package no longer export it behind the host's back).  It matters for the side-by-side ticking measurements only.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

HBM_PEAK_GBS = 8000.0          # MI355X spec, /opt/skills/guides/MI355X_MICROARCH.md
FP32_PEAK_TFLOPS = 157.3
BYTES_PER_FRAME_FUSED = 16948  # I/O + resident-state touch of one process_frame
FLOPS_PER_FRAME = 0.42e6

# The issue ceiling: the vector-ALU time a kernel's ARITHMETIC needs per stream-frame on CDNA4 if every SIMD did nothing else.
# Issue costs measured on an MI355X (scripts/ubench/valu_issue.hip, profiles/r6_valu_issue.txt; round 5 assumed 4 cycles for every instruction): with
# two or more waves on a SIMD a plain two-operand f32 instruction (v_add / v_mul / v_max) takes 2.27 cycles, a packed or three-operand one
# (v_pk_*, v_fma) 4.2 -- so an exact multiply-add (no FMA upstream of the pitch index) costs 4.5 cycles per 64 lanes either way, a fused one 2.1
# (v_pk_fma_f32).  Arithmetic per stream-frame:
#   k_pitch   multiply-adds of the certified search (round 6): FIR 864 x 5, fine search 10 x 480, remove_doubling 25 x 480 (+ 3 x 480 when a block
#             refines), exact coarse sums ~5 x 240, the three energy scans 240 + 2 x 147, 480 + 2 x 294, 480 + 2 x 384 -- 2.6e4, all exact (4.5 cycles / 64)
#   k_fft_xp, k_synth   the arithmetic column of scripts/isa_mix.py (profiles/r6_isa_mix.json, written at build time: straight-line kernels, static
#             count = issued count), at the packed / fused cost
#   k_rnn     551 activations x ~25 plain instructions / 64 lanes beside 32 MFMAs per stream-frame (x 16 cycles, hidden under them)
#   k_lpc     5 x 860 exact multiply-adds;  k_hp  its HBM bytes (its 90 f64 instructions per stream-frame issue in less)
CYC_PLAIN, CYC_PACKED = 2.27, 4.2
PITCH_MACS = 864 * 5 + 10 * 480 + 25 * 480 + 5 * 240 + (240 + 2 * 147) + (480 + 2 * 294) + (480 + 2 * 384)
KERNEL_MIN_CYCLES = {   # SIMD cycles per stream-frame (already divided by the 64 lanes of a wave instruction)
    "k_pitch": PITCH_MACS * 2 * CYC_PLAIN / 64,
    "k_rnn": 215 * CYC_PLAIN,
    "k_lpc": 5 * 860 * 2 * CYC_PLAIN / 64,
    "k_hp": 90 * CYC_PACKED,
}
SIMDS, CLOCK_HZ = 1024, 2.4e9

# Algorithmic HBM bytes per stream-frame of each kernel (its own inputs + outputs, each counted once; per-group state traffic
# divided by the G frames of a full group; derivation in DESIGN.md "Kernels")
G = 24   # frames of a full group (a 48-frame call is two of them)
KERNEL_BYTES = {
    "k_hp": 1920 + 1920 + 960 + 960 // 5 + 4 + (16 + 8) // G,     # input, history slot, 240 decimated values (+ mirrored share), x_lp[0]; biquad state per group
    "k_lpc": (864 + 7 * 240) * 4 // 8 + 4 + 40,                     # decimated windows of eight consecutive frames read once by their wave (1272 B per frame; small launches
                                                                   # take fewer frames per wave, up to 3456 B) + x_lp[0] in; autocorrelation and FIR taps out
    "k_pitch": 3456 + 4 + 20 + 8 + 16 // G,                         # decimated window + x_lp[0] + FIR taps in; pitch index + gain out; last pitch per group
                                                                   # (pitch_buf, coarse xcorr, the running energies and their check points never leave LDS)
    "k_fft_xp": 3840 + 1200 + 4 + 3856 + 3344 + 264 + 112 + 4,     # 960 + (mean lag 300) history samples; X as 241 (bin k, bin 480 - k) pairs of 16 bytes, P as 64 lone bins + 177 pairs; band energies, cepstrum head out
    "k_rnn": 120 + 88 + 4 + 2 * 88 + 2 * 88 + (704 + 2 * 672 + 8) // G,   # features head in; ring row, vad, gains, last gains; ring + GRU states per group
    "k_synth": 3856 + 3344 + 440 + 8 + 1920 + 8 + 3840 // G,       # X (bin pairs), P (64 bins + 177 pairs), band quantities in; audio, vad, branch out; overlap memory per group
    # the fused back end (transforms + features + RNN + synthesis in one launch, the spectra in registers): history samples and pitch in; band
    # quantities (parity taps), ring row, vad, gains, last gains, branch, audio out; overlap memory in and out per frame; ring + GRU states per launch
    "k_back": 3840 + 1200 + 4 + 268 + 88 + 4 + 2 * 88 + 2 * 88 + 4 + 1920 + 3840 + (704 + 2 * 672 + 8) // 1,
}

# Useful arithmetic per stream-frame of each kernel (SURVEY.md 8(d)'s break-down of the 0.42 MFLOP) and the roof that applies to
# it (TFLOP/s): the pitch analysis may not fuse a multiply with an add (bit-exact sums in the reference's order), so its roof
# is half the FP32 vector peak; the transforms run at the full FP32 vector peak; the RNN's products run as three bf16 planes
# per f32 activation on the matrix cores (dense bf16 peak / 3); the biquad is an f64 chain.
KERNEL_FLOPS = {"k_hp": 480 * 13, "k_lpc": 8.7e3, "k_pitch": 126e3, "k_fft_xp": 66e3, "k_rnn": 174e3, "k_synth": 42e3, "k_back": 66e3 + 174e3 + 42e3}
KERNEL_ROOF_TFLOPS = {"k_hp": FP32_PEAK_TFLOPS / 2, "k_lpc": FP32_PEAK_TFLOPS / 2, "k_pitch": FP32_PEAK_TFLOPS / 2, "k_fft_xp": FP32_PEAK_TFLOPS, "k_synth": FP32_PEAK_TFLOPS,
                      "k_rnn": 2500.0 / 3, "k_back": FP32_PEAK_TFLOPS}
KERNEL_ROOF_NAME = {"k_hp": "f64 vector, serial chain", "k_lpc": "FP32 vector without FMA (exact sums)", "k_pitch": "FP32 vector without FMA (exact sums)", "k_fft_xp": "FP32 vector",
                    "k_synth": "FP32 vector", "k_rnn": "bf16 MFMA / 3 planes",
                    "k_back": "FP32 vector (transforms and synthesis; its RNN stretch runs on bf16 MFMA / 3 planes)"}

CONFIGS = {
    1: {"streams": 4096, "model": None, "name": "configs[1]: 4096 concurrent mono streams per GPU, built-in weights.rnn"},
    2: {"streams": 65536, "model": None, "name": "configs[2]: 65536 concurrent streams on one GPU, built-in weights.rnn, GRU as batched MFMA GEMM"},
    3: {"streams": 32768, "model": None, "name": "configs[3]: 262144 streams sharded over 8 GPUs = 32768 per GPU, built-in weights.rnn"},
    4: {"streams": 65536, "model": os.path.join(ROOT, "tests", "golden", "sh.rnn"),
        "name": "configs[4]: custom model (GregorR rnnoise-models 'sh' converted to .rnn), 65536 streams",
        "parity": "oracle-only: the reference holds no output for sh.rnn (SURVEY 8(c)), so this configuration is checked device-against-oracle, "
                  "never against a reference-issued vector"},
}


def host_info():
    """What the CPU baseline ran on: logical CPUs, affinity, cgroup quota, model name, load."""
    info = {"nproc": os.cpu_count()}
    if hasattr(os, "sched_getaffinity"):
        info["affinity"] = len(os.sched_getaffinity(0))
    for p in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            info["cgroup_" + os.path.basename(p)] = open(p).read().strip()
        except OSError:
            pass
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                info["cpu_model"] = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    try:
        info["loadavg"] = open("/proc/loadavg").read().split()[:3]
    except OSError:
        pass
    return info


def cpu_baseline(budget_s=16.0):
    """Time the CPU oracle (f32-FFT build) on the host's cores: nothing but process_frame in the timed region (one
    state and one input buffer per thread, made before the clock starts; oracle/nnn_oracle.c nnno_bench)."""
    from oracle import oracle as O
    model = O.Model(open(os.path.join(ROOT, "nnnoiseless_amd", "data", "weights.rnn"), "rb").read(), f32_fft=True)
    info = host_info()
    cores = info.get("affinity") or info.get("nproc") or 1
    w1, _ = O.bench(model, 1, 10, 0)
    one = 1000.0 / w1                                  # frames/s, one thread, synthetic mix, continuing state
    ws, _ = O.bench(model, 1, 10, 1)
    sin440 = 1000.0 / ws                              # frames/s, the reference's benches/sin.rs shape
    counts = sorted({c for c in (2, 4, 8, 16, 32, 64, 128, cores // 2, cores) if 1 < c <= cores})
    per = max(1.0, (budget_s - 2.0) / max(1, len(counts)))
    table = {"1": one}
    best_n, best = 1, one
    for n in counts:
        wall, _ = O.bench(model, n, 2, 0)                        # pilot: how fast do n threads really go here
        iters = max(2, min(400, int(per / (wall / 2.0))))        # then ~`per` seconds at that rate
        wall, secs = O.bench(model, n, iters, 0)
        v = n * iters * 100.0 / wall
        table[str(n)] = v
        if v > best:
            best_n, best = n, v
    eff = best / (best_n * one)
    note = "genuine Rust reference not buildable here (no cargo/rustc)"
    if eff < 0.7:
        note += (f"; threads scale {eff:.2f}x of linear at the best count ({best_n}): the timed region holds only process_frame "
                 "(private state and input per thread, no allocation, no shared writes), so the loss is the host's -- a CPU quota / "
                 "shared cores of the container (see host), not the port")
    return {"value": best, "unit": "frames/s", "cores": best_n, "kind": "port",
            "sample": f"synthetic sine+noise, one continuing state per thread, {best_n} threads; oracle/nnn_oracle.c -O3 -march=x86-64-v3, f32 FFT",
            "single_thread": one, "scaling_frames_per_s_by_threads": table, "thread_efficiency": eff,
            "sin_440": {"value": sin440, "unit": "frames/s", "cores": 1,
                        "sample": "benches/sin.rs shape: 100 frames of a 440 Hz sine at amplitude 32767, fresh state per iteration, 10 iterations"},
            "host": info, "note": note}


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--config", type=int, default=2, choices=[0, 1, 2, 3, 4], help="BASELINE.json configs[i] (see the module docstring)")
    ap.add_argument("--streams", type=int, default=None, help="concurrent streams PER GPU (overrides the config's)")
    ap.add_argument("--model", default=None, help=".rnn model file (configs[4]; default for --config 4: tests/golden/sh.rnn)")
    ap.add_argument("--frames-per-step", type=int, default=48,
                    help="frames per stream per call (0.48 s of audio by default); the same JSON line also reports the one-frame-per-call rate (`tick`)")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--no-overlap", action="store_true",
                    help="do not tell the library that inputs are final at call time (nnn_batch_set_inputs_ready): every call then "
                         "waits for the previous one to drain before it reads its input")
    ap.add_argument("--workload", choices=["denoise", "train", "resample"], default="denoise",
                    help="denoise = process_frame (the headline); train = 87-column training rows (SURVEY 8(f) #3); "
                         "resample = the CLI's 16-tap sinc resampler 44.1 -> 48 kHz (SURVEY 8(f) #4)")
    ap.add_argument("--pcm", choices=["f32", "i16", "unit"], default="f32",
                    help="boundary sample format (SURVEY 8(f) #1): f32 = process_frame's own (headline), i16 = the CLI's "
                         "packed int16, unit = DenoiseSignal's [-1, 1] floats")
    ap.add_argument("--channels", type=int, default=1, help="interleaved channels per group (with --pcm i16/unit)")
    ap.add_argument("--layout", choices=["stream-major", "frame-major"], default="stream-major",
                    help="resident buffers as [stream][frame][480] (one stream's audio contiguous, the reference's per-stream slices side by "
                         "side) or [frame][stream][480] (the batch's frames interleaved); f32 mono only")
    ap.add_argument("--full", action="store_true",
                    help="also run every measurement beside the headline (tick, roofline pass, configs[1] / configs[4], default call "
                         "ordering, host boundary, CPU baseline); a plain run times the headline workload only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs (a fixed sample of streams) to DIR/out.npy and DIR/vad.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-roofline", action="store_true", help="with --full: skip the event-instrumented roofline pass")
    ap.add_argument("--no-host", action="store_true", help="with --full: skip the PCIe-inclusive host-buffer measurement of the default run")
    ap.add_argument("--no-tick", action="store_true", help="with --full: skip the one-frame-per-call measurement")
    ap.add_argument("--no-also", action="store_true", help="with --full: skip the extra configs[1] / configs[4] measurements of the default run")
    ap.add_argument("--min-timed-s", type=float, default=0.5, help="the `also` entries run enough steps to be timed for at least this long")
    ap.add_argument("--pool-bytes", type=float, default=6.5e9, help="HBM budget for the resident input pool (and as much again for the output)")
    ap.add_argument("--single-process", action="store_true",
                    help="all --gpus devices from ONE process through the library's node object (include/nnn_node.h: one batch and one host "
                         "thread per device, the stream split inside the library) instead of one rank per GPU under torch.distributed")
    ap.add_argument("--dry-run", action="store_true",
                    help="plumbing check without a GPU: gloo backend, CPU tensors, the library named by NNN_LIBRARY (the tests "
                         "point it at the SIMT-interpreter build), a few streams; the numbers mean nothing")
    args = ap.parse_args(argv)
    if args.dump_outputs and (args.config == 0 or args.single_process or args.workload != "denoise"):
        ap.error("--dump-outputs: the denoise workload of configs 1-4 under one process per GPU only")
    return args


def pmc_profile(kind, S):
    """The newest committed rocprofv3 --pmc summary for this stream count (profiles/r<round>_pmc_<kind>_<S>streams.json) or None; the
    summary's file name travels with it (`file`)."""
    import glob
    best = None
    for path in glob.glob(os.path.join(ROOT, "profiles", f"r*_pmc_{kind}_{S}streams.json")):
        try:
            rnd = int(os.path.basename(path).split("_")[0][1:])
        except ValueError:
            continue
        if best is None or rnd > best[0]:
            best = (rnd, path)
    if best is None:
        return None
    try:
        d = json.load(open(best[1]))
    except Exception:
        return None
    if d.get("streams") != S:
        return None
    d["file"] = "profiles/" + os.path.basename(best[1])
    return d


def isa_arithmetic():
    """Arithmetic vector instructions per stream-frame of the straight-line kernels, from the newest committed scripts/isa_mix.py --json summary
    (static count = what a wave issues per stream-frame there; written at build time, see __graft_entry__.build / scripts/isa_mix.py)."""
    import glob
    paths = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_isa_mix.json")), key=lambda q: int(os.path.basename(q).split("_")[0][1:]))
    if not paths:
        return {}, None
    try:
        d = json.load(open(paths[-1]))
    except Exception:
        return {}, None
    out = {}
    for k, v in d.get("kernels", {}).items():   # (k_synth<true> is the instantiation of the plain boundary format: the one the headline runs)
        out[k.replace("<true>", "")] = v.get("arith_cycles")
    return out, "profiles/" + os.path.basename(paths[-1])


DUMP_BYTES = 64 << 20   # --dump-outputs: the most it writes


def dump_outputs(path, torch, y, vad, S, pool, layout, channels, positions):
    """--dump-outputs: the outputs at the absolute frame positions `positions` (the last timed step) of a fixed, seeded sample of
    streams, as float32 out.npy [streams, frames, 480] and vad.npy [streams, frames].  `layout`: "stream" ([S, pool, 480]), "frame"
    ([pool, S, 480]) or "packed" ([S // channels, pool * 480, channels]) -- the resident buffers of measure()."""
    import numpy as np
    positions = positions[-min(pool, DUMP_BYTES // (481 * 4)):]   # a step longer than the pool has overwritten its own first frames
    n = max(1, min(S, 256, DUMP_BYTES // (len(positions) * 481 * 4)))
    streams = torch.as_tensor(np.sort(np.random.default_rng(0).choice(S, n, replace=False)), device=y.device)
    frames = torch.as_tensor([p % pool for p in positions], device=y.device)
    if layout == "frame":
        out = y[:, streams][frames].transpose(0, 1)
    elif layout == "packed":
        out = y.reshape(S // channels, pool, 480, channels)[streams // channels, :, :, streams % channels][:, frames]
    else:
        out = y[streams][:, frames]
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "out.npy"), out.float().cpu().numpy())
    np.save(os.path.join(path, "vad.npy"), vad[:, streams][frames].t().float().cpu().numpy())


def measure(args, S, model_path, rank, world, dev, local_rank, dist, torch, want_tick=True, want_roofline=True, min_timed_s=0.0,
            dump_dir=None):
    """One workload on this rank's device.  Returns (dict of measured quantities aggregated over ranks, roofline pass): the
    second is a callable (or None) that runs the event-instrumented pass on this rank and returns the extra fields -- rank 0
    calls it after the ranks have parted, so that nobody idles behind it.  `dump_dir`: rank 0 writes the last timed step's
    outputs there (dump_outputs) before anything else runs on the buffers."""
    import nnnoiseless_amd as nn
    from nnnoiseless_amd.shard import aggregate, gather
    from nnnoiseless_amd.synthetic import make_streams_device
    fps, K, W = args.frames_per_step, args.steps, args.warmup
    fmt = {"f32": 0, "i16": 1, "unit": 2}[args.pcm]
    Cc = args.channels
    assert S % Cc == 0
    esz = 2 if fmt == 1 else 4
    # distinct audio for every step while it fits the pool budget, else cycle through a pool of frames
    pool = max(1, min((K + W) * fps, int(args.pool_bytes // (S * 480 * esz))))
    if pool >= fps:
        pool -= pool % fps   # whole steps: a step never straddles the end of the pool (no call is cut in two)
    x = make_streams_device(torch, dev, S, pool, seed=rank)               # [S, pool, 480] f32, resident
    if fmt or Cc > 1:   # packed PCM: [groups][pool * 480][channels], channel-interleaved
        x = x.reshape(S // Cc, Cc, pool * 480).permute(0, 2, 1)
        x = (x.to(torch.int16) if fmt == 1 else (x / 32768.0 if fmt == 2 else x)).contiguous()
    fm = args.layout == "frame-major" and not fmt and Cc == 1
    if fm:
        x = x.permute(1, 0, 2).contiguous()   # [pool, S, 480]
    y = torch.empty_like(x)
    vad = torch.empty((pool, S), dtype=torch.float32, device=dev)
    model = None
    if model_path:
        model = nn.RnnModel.from_bytes(open(model_path, "rb").read())
        if model is None:
            raise SystemExit(f"bench: {model_path} is not a valid .rnn model")
    bd = nn.BatchDenoiser(S, model=model, device=0 if args.dry_run else local_rank)   # the interpreter build has one device
    if args.no_graph:
        bd.set_graph(False)
    if not args.no_overlap:
        # the input pool is resident and final before the timed region starts: consecutive calls may overlap at their boundary
        # (the next call's high-pass chain starts while the previous call drains; outputs stay ordered on the stream)
        bd.set_inputs_ready(True)
    stream = torch.cuda.current_stream().cuda_stream if dev.type == "cuda" else 0

    def run(f0, n, bd=bd):   # n frames of every stream starting at frame f0 of the pool: never past its end
        assert 0 <= f0 and n > 0 and f0 + n <= pool, (f0, n, pool)
        off = f0 * 480 * Cc * esz
        if fmt or Cc > 1:
            bd.process_pcm_device(x.data_ptr() + off, y.data_ptr() + off, vad.data_ptr() + f0 * S * 4, n, fmt, Cc,
                                  pool * 480 * Cc, 480 * Cc, False, stream)
        elif fm:
            offm = f0 * S * 480 * 4
            bd.process_device(x.data_ptr() + offm, y.data_ptr() + offm, vad.data_ptr() + f0 * S * 4, n, 480, S * 480, stream)
        else:
            bd.process_device(x.data_ptr() + off, y.data_ptr() + off, vad.data_ptr() + f0 * S * 4, n, pool * 480, 480, stream)

    def run_span(pos, n, bd=bd):   # n frames starting at absolute frame `pos`, wrapping around the pool as often as needed
        while n > 0:
            f0 = pos % pool
            m = min(n, pool - f0)
            run(f0, m, bd)
            pos += m
            n -= m

    def sync():
        if dev.type == "cuda":
            torch.cuda.synchronize()
        else:
            bd.synchronize()

    def barrier():
        sync()
        if world > 1:
            dist.barrier()
        sync()

    barrier()
    tw = time.perf_counter()
    for i in range(W):
        run_span(i * fps, fps)
    barrier()
    tw = time.perf_counter() - tw
    if min_timed_s > 0 and W > 0 and world == 1:
        # an `also` entry: enough steps for the timed region to last min_timed_s (the warm-up's own rate is the estimate)
        K = max(K, int(np_ceil(1.2 * min_timed_s / max(tw / W, 1e-6))))
    t0 = time.perf_counter()
    for i in range(W, W + K):
        run_span(i * fps, fps)
    t_enq = time.perf_counter() - t0          # host time to enqueue everything (the calls are asynchronous)
    if not args.dry_run:
        torch.cuda.synchronize()
    local = time.perf_counter() - t0          # this rank's own GPU done (before it waits for the others): per-rank rates below
    barrier()
    elapsed = time.perf_counter() - t0
    if bd.fault():                            # (a caller that synchronises its own stream has to ask: nnn_batch_fault)
        raise SystemExit("bench: the library reports a frame hand-off fault (nnn_batch_fault): results invalid")
    if dump_dir and rank == 0:
        dump_outputs(dump_dir, torch, y, vad, S, pool, "packed" if fmt or Cc > 1 else ("frame" if fm else "stream"), Cc,
                     list(range((W + K - 1) * fps, (W + K) * fps)))
    d = dist if world > 1 else None
    frames_done, elapsed_max = aggregate(d, S * fps * K, elapsed, dev)
    per_rank = [round(v) for v in gather(d, S * fps * K / max(local, 1e-9), dev)]   # frames/s of every rank on its own clock
    if os.environ.get("NNN_PMC_CALIB"):   # a kernel of known traffic (reads N bytes, writes N bytes) for the PMC passes' calibration
        torch.abs(x)
    res = {"value": frames_done / elapsed_max, "ms_per_step": elapsed_max * 1e3 / K, "timed_s": elapsed_max, "steps": K,
           "host_enqueue_ms_per_step": t_enq * 1e3 / K, "pool_frames": pool, "per_rank_frames_per_s": per_rank,
           "outputs_finite": bool(torch.isfinite(y.float()).all().item())}

    # the same workload at one frame per call (live 10 ms tick)
    if want_tick and fps != 1:
        kt = min(200, max(20, K * fps // 4))
        pos = (W + K) * fps
        for j in range(10):
            run_span(pos + j, 1)
        barrier()
        t1 = time.perf_counter()
        for j in range(10, 10 + kt):
            run_span(pos + j, 1)
        barrier()
        tt = time.perf_counter() - t1
        tf, tmax = aggregate(d, S * kt, tt, dev)
        res["tick"] = {"frames_per_step": 1, "value": tf / tmax, "unit": "frames/s", "ms_per_step": tmax * 1e3 / kt, "steps": kt,
                       "kb_per_stream": round(bd.device_bytes() / S / 1024, 1)}
        # ... and on a batch created for it (nnn_batch_opts.max_group_frames = 1: scratch and history rings for one-frame groups)
        bd1 = nn.BatchDenoiser(S, model=model, device=0 if args.dry_run else local_rank, max_group_frames=1)
        if not args.no_overlap:
            bd1.set_inputs_ready(True)
        for j in range(10):
            run_span(pos + j, 1, bd1)
        barrier()
        t1 = time.perf_counter()
        for j in range(10, 10 + kt):
            run_span(pos + j, 1, bd1)
        barrier()
        tt = time.perf_counter() - t1
        tf, tmax = aggregate(d, S * kt, tt, dev)
        res["tick"]["batch_sized_for_ticks"] = {"value": tf / tmax, "ms_per_step": tmax * 1e3 / kt,
                                                "kb_per_stream": round(bd1.device_bytes() / S / 1024, 1)}
        bd1.close()

    def close():
        nonlocal x, y, vad
        bd.close()
        del x, y, vad
        if dev.type == "cuda":
            torch.cuda.empty_cache()

    if not (want_roofline and rank == 0 and dev.type == "cuda"):
        close()
        return res, None
    per_gpu = res["value"] / world

    def roofline_pass():
        # second pass over the same workload with HIP events around every launch, on the stream they are launched on
        bd.set_profiling(True)
        kp = min(K, 12)
        for i in range(kp):
            run_span((W + K + i) * fps, fps)
        sync()
        times = bd.kernel_times()
        bd.set_profiling(False)
        close()
        frames_prof = kp * fps
        kern = {k: {"avg_us": 1e3 * ms / max(n, 1), "launches": n, "us_per_frame": 1e3 * ms / frames_prof}
                for k, (ms, n) in times.items() if n}
        for k, v in kern.items():   # each kernel's useful arithmetic against the roof that applies to it, and its algorithmic bytes against HBM
            sec_per_stream_frame = v["us_per_frame"] * 1e-6 / S
            v["useful_tflops"] = KERNEL_FLOPS.get(k, 0) / sec_per_stream_frame / 1e12
            v["roof_tflops"] = KERNEL_ROOF_TFLOPS.get(k)
            v["roof"] = KERNEL_ROOF_NAME.get(k)
            v["frac_of_roof"] = v["useful_tflops"] / KERNEL_ROOF_TFLOPS[k] if k in KERNEL_ROOF_TFLOPS else None
            v["hbm_frac"] = KERNEL_BYTES.get(k, 0) / sec_per_stream_frame / 1e9 / HBM_PEAK_GBS
        dom = max(kern, key=lambda k: kern[k]["us_per_frame"])
        # one launch of the dominant kernel covers frames_prof / launches frames of every stream
        frames_per_launch = frames_prof / kern[dom]["launches"]
        avg_s = kern[dom]["avg_us"] * 1e-6
        bytes_per_launch = KERNEL_BYTES.get(dom, 0) * S * frames_per_launch
        achieved = bytes_per_launch / avg_s / 1e9
        # HBM-side bytes from the committed rocprofv3 --pmc passes at this stream count, per stream-frame there and scaled to THIS run's
        # launch (streams x frames per launch) so that `traffic` and `bytes_per_launch` describe the same launch; the per-stream-frame
        # pair is printed beside them (the PMC passes' own group length: `traffic_source`)
        traffic = traffic_psf = traffic_src = None
        pm = pmc_profile("traffic", S)
        if pm and dom in pm["kernels"]:
            traffic_psf = pm["kernels"][dom]["hbm_bytes_per_stream_frame"]
            traffic = traffic_psf * S * frames_per_launch
            traffic_src = f"{pm.get('file')} (2*FETCH_SIZE+WRITE_SIZE, separate passes, {pm.get('frames_per_launch')}-frame launches there)"
        # what binds the dominant kernel: the busiest on-chip resource of the committed SQ counter pass at this stream count
        binding = None
        sq = pmc_profile("sq", S)
        if sq and dom in sq.get("kernels", {}):
            q = sq["kernels"][dom]
            cand = {"vector ALU issue": q.get("valu_busy"), "LDS": q.get("lds_busy")}
            cand = {k: v for k, v in cand.items() if v is not None}
            if cand:
                top = max(cand, key=cand.get)
                binding = {"resource": top, "busy": cand[top], "valu_busy": q.get("valu_busy"), "lds_busy": q.get("lds_busy"),
                           "lds_conflict_share": q.get("lds_conflict_share"), "waiting_share": q.get("wait_share"), "source": f"{sq.get('file')} (rocprofv3 --pmc SQ_* passes)"}
        # the whole path's HBM traffic from the counters against its algorithmic bytes (16 948 B), and the issue ceiling
        path_traffic = None
        if pm:
            tot = sum(v.get("hbm_bytes_per_stream_frame", 0.0) for v in pm["kernels"].values())
            path_traffic = {"pmc_bytes_per_stream_frame_all_kernels": tot, "algorithmic_bytes_per_stream_frame": BYTES_PER_FRAME_FUSED,
                            "traffic_over_algorithmic": tot / BYTES_PER_FRAME_FUSED,
                            "per_kernel": {k: round(v.get("hbm_bytes_per_stream_frame", 0.0)) for k, v in pm["kernels"].items()},
                            "note": "the excess is the spectra X and P crossing HBM between k_fft_xp and k_synth (the fused back end keeps them in registers: one-frame calls only)"}
        ceiling = None
        if sq:
            fl = sq.get("frames_per_launch", 24)
            arith, arith_src = isa_arithmetic()
            min_cycles = dict(KERNEL_MIN_CYCLES)
            for k in ("k_fft_xp", "k_synth"):   # straight-line kernels: the static arithmetic count IS the issued count, each instruction at its class's cost
                if arith.get(k):
                    min_cycles[k] = arith[k]
            rows, t_min = {}, 0.0
            for k, v in kern.items():
                issued = sq["kernels"].get(k, {}).get("counters", {}).get("SQ_INSTS_VALU")
                need = min_cycles.get(k)
                if need is None:
                    continue
                us_issue = need * S / (SIMDS * CLOCK_HZ) * 1e6
                us_hbm = KERNEL_BYTES.get(k, 0) * S / (HBM_PEAK_GBS * 1e9) * 1e6
                us_min = max(us_issue, us_hbm)
                t_min += us_min
                rows[k] = {"valu_issued_per_stream_frame": round(issued * 32 / (S * fl)) if issued else None, "arithmetic_simd_cycles_per_stream_frame": round(need, 1),
                           "us_per_frame_floor": round(us_min, 1), "floor_set_by": "hbm" if us_hbm > us_issue else "vector issue",
                           "us_per_frame_measured": round(v["us_per_frame"], 1)}
            ceiling = {"kernels": rows, "sum_floor_us_per_frame": round(t_min, 1), "frames_per_s_at_the_floor": S / (t_min * 1e-6) if t_min else None,
                       "measured_over_floor": per_gpu / (S / (t_min * 1e-6)) if t_min else None,
                       "hbm_frac_at_the_floor": (S / (t_min * 1e-6)) * BYTES_PER_FRAME_FUSED / 1e9 / HBM_PEAK_GBS if t_min else None,
                       "issue_cycles": {"plain_f32": CYC_PLAIN, "packed_or_fused": CYC_PACKED, "source": "profiles/r6_valu_issue.txt (scripts/ubench/valu_issue.hip)"},
                       "arithmetic_source": {"k_fft_xp, k_synth": arith_src, "others": "bench.py KERNEL_MIN_CYCLES (derivations in the comment above it)"},
                       "note": "floor = every SIMD issuing only the kernel's arithmetic at the measured issue cost, or its algorithmic bytes at 8 TB/s; issued "
                               f"counts from {sq.get('file')} (SQ_INSTS_VALU x 32 shader engines / stream-frames)"}
        return {"kernels": kern, "roofline": {
            "bound": "hbm", "kernel": dom, "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": achieved / HBM_PEAK_GBS, "traffic": traffic,
            "frac_by_counters": (traffic / avg_s / 1e9 / HBM_PEAK_GBS) if traffic else None,
            "measured_binder": (binding or {}).get("resource"),
            "kernels_us_per_frame": {k: round(v["us_per_frame"], 1) for k, v in kern.items()},
            "alg_bytes_per_stream_frame": KERNEL_BYTES.get(dom, 0), "traffic_per_stream_frame": traffic_psf, "traffic_source": traffic_src,
            "avg_kernel_us": avg_s * 1e6, "frames_per_launch": frames_per_launch, "bytes_per_launch": bytes_per_launch,
            "binding": binding, "path_traffic": path_traffic, "issue_ceiling": ceiling,
            "useful_tflops": kern[dom]["useful_tflops"], "roof_tflops": kern[dom]["roof_tflops"], "roof": kern[dom]["roof"],
            "frac_of_applicable_roof": kern[dom]["frac_of_roof"],
            "sum_kernel_us_per_frame": sum(v["us_per_frame"] for v in kern.values()),
            "pipeline_fused_bytes_GBs": per_gpu * BYTES_PER_FRAME_FUSED / 1e9,
            "pipeline_hbm_frac": per_gpu * BYTES_PER_FRAME_FUSED / 1e9 / HBM_PEAK_GBS,
            "pipeline_fp32_frac": per_gpu * FLOPS_PER_FRAME / 1e12 / FP32_PEAK_TFLOPS,
            "note": "`bound`: the roof north_star asks the fraction of (HBM); `frac` by the kernel's algorithmic bytes, `frac_by_counters` by the bytes "
                    "the PMC passes saw.  The path sits at 23-100 FLOP/B (SURVEY 8d) and its dominant kernel hardly touches HBM: `measured_binder` / "
                    "`binding` name the on-chip resource the SQ counters show busiest, `frac_of_applicable_roof` the kernel's useful arithmetic "
                    "against the roof that applies to it.  `avg_kernel_us`: HIP events around every launch with the launches IN ORDER (the "
                    "library's profiling pass; rocprofv3 --kernel-trace --stats with NNN_SCHED=seq reproduces it: profiles/r<round>_kernel_stats_*_"
                    "sequential.md).  The timed loop of a big batch overlaps its kernels (round 6): there a kernel's wall time includes the time it "
                    "shares the GPU with its neighbours (profiles/r<round>_kernel_stats_*streams_48fps.md), and the per-kernel times no longer sum to "
                    "ms_per_step -- `overlap_gain` = the in-order sum / ms_per_step",
            "overlap_gain": sum(v["us_per_frame"] for v in kern.values()) * fps / 1e3 / res["ms_per_step"]}}
    return res, roofline_pass


def np_ceil(v):
    import math
    return math.ceil(v)


def config0():
    """configs[0]: the reference's own CPU-runnable case, on the CPU oracle (plumbing; no GPU involved)."""
    import numpy as np
    from oracle import oracle as O
    g = os.path.join(ROOT, "tests", "golden")
    inp = np.fromfile(os.path.join(g, "testing.raw"), dtype="<i2").astype(np.float32)
    ref = np.fromfile(os.path.join(g, "reference_output.raw"), dtype="<i2")
    n = len(inp) // 480
    model = O.Model(open(os.path.join(ROOT, "nnnoiseless_amd", "data", "weights.rnn"), "rb").read(), f32_fft=True)
    t0 = time.perf_counter()
    out = O.run_streams(model, inp[: n * 480].reshape(1, n, 480), want=("out",))["out"][0, 1:].reshape(-1)
    dt = time.perf_counter() - t0
    o16 = np.clip(np.trunc(out), -32768, 32767)
    err = float(((ref - o16) ** 2).sum() / (o16 ** 2).sum())
    print(json.dumps({"metric": "480-sample frames/sec (whole node) at N concurrent streams", "value": n / dt, "unit": "frames/s",
                      "n_gpus": 0, "steps": 1, "warmup": 0, "ms_per_step": dt * 1e3, "higher_is_better": True, "scaling": "weak",
                      "vs_baseline": None, "dtype": "f32", "data": "test_data/testing.raw (reference golden input)",
                      "config": {"workload": "configs[0]: 1 stream, built-in weights.rnn, testing.raw on the CPU oracle (port of the reference; plumbing, no GPU)"},
                      "golden_metric": err}), flush=True)


def host_boundary_child(argv):
    """bench.py --host-boundary-child: the host-buffer entry point in a process of its own (no torch, nothing else resident), one JSON line.
    The workload through nnn_batch_process_pcm_host from page-locked buffers at 4096 and 65 536 streams, f32 and packed int16, and --
    the same process, the same buffers' sizes -- what the link itself gives: hipMemcpyAsync up, down and both ways at once on two streams."""
    import ctypes as C
    import numpy as np
    import nnnoiseless_amd as nn
    from nnnoiseless_amd import _ffi
    fps = int(argv[0]) if argv else 48
    lib = nn.library()
    hip = C.CDLL("libamdhip64.so")
    vp, sz = C.c_void_p, C.c_size_t
    hip.hipMalloc.argtypes = [C.POINTER(vp), sz]
    hip.hipFree.argtypes = [vp]
    hip.hipMemcpyAsync.argtypes = [vp, vp, sz, C.c_int, vp]
    hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(vp), C.c_uint]
    hip.hipStreamSynchronize.argtypes = [vp]
    s_in, s_out = vp(), vp()
    assert hip.hipStreamCreateWithFlags(C.byref(s_in), 1) == 0 and hip.hipStreamCreateWithFlags(C.byref(s_out), 1) == 0
    out = {"unit": "frames/s", "frames_per_call": fps,
           "note": "PCIe-inclusive: upload + kernels + download per call, page-locked host buffers (nnn_host_alloc), chunks overlapped; "
                   "bus = hipMemcpyAsync of the same byte counts in the same process, both directions at once on two streams; never `value`"}
    block = (np.random.default_rng(0).standard_normal((64, fps * 480), dtype=np.float32) * 3000)
    # Right after the parent bench has freed tens of gigabytes of device memory the driver is still clearing them with the copy engines, and
    # for a second or two the two directions of the link take turns (57 GB/s both ways instead of 97; the same child started from an idle
    # parent measures 97 from its first copy): copy both ways until the rate has settled (three rounds within 2 %, at most 5 s).
    wn = 64 << 20
    wh0, wh1 = nn.pinned_empty((wn,), np.uint8), nn.pinned_empty((wn,), np.uint8)
    wd0, wd1 = vp(), vp()
    assert hip.hipMalloc(C.byref(wd0), wn) == 0 and hip.hipMalloc(C.byref(wd1), wn) == 0
    rates, t_start = [], time.perf_counter()
    while time.perf_counter() - t_start < 5.0:
        t0 = time.perf_counter()
        for _ in range(8):
            assert hip.hipMemcpyAsync(wd0, wh0.ctypes.data, wn, 1, s_in) == 0 and hip.hipMemcpyAsync(wh1.ctypes.data, wd1, wn, 2, s_out) == 0
        hip.hipStreamSynchronize(s_in); hip.hipStreamSynchronize(s_out)
        rates.append(2 * wn * 8 / (time.perf_counter() - t0) / 1e9)
        if len(rates) >= 4 and max(rates[-3:]) - min(rates[-3:]) <= 0.02 * rates[-1] and rates[-1] >= 0.98 * max(rates):
            break
    out["link_settled_after_s"] = round(time.perf_counter() - t_start, 2)
    hip.hipFree(wd0); hip.hipFree(wd1)
    del wh0, wh1
    for S, calls in ((4096, 4), (65536, 2)):
        for fmt, name in ((0, "f32"), (1, "i16")):
            dt = np.float32 if fmt == 0 else np.int16
            px, po, pv = nn.pinned_empty((S, fps * 480), dt), nn.pinned_empty((S, fps * 480), dt), nn.pinned_empty((fps, S))
            px.reshape(S // 64, 64, -1)[:] = block.astype(dt)[None]
            n = px.nbytes
            # the link: both directions at once, the call's byte counts
            d0, d1 = vp(), vp()
            assert hip.hipMalloc(C.byref(d0), n) == 0 and hip.hipMalloc(C.byref(d1), n) == 0

            def both():
                assert hip.hipMemcpyAsync(d0, px.ctypes.data, n, 1, s_in) == 0 and hip.hipMemcpyAsync(po.ctypes.data, d1, n, 2, s_out) == 0
            both(); hip.hipStreamSynchronize(s_in); hip.hipStreamSynchronize(s_out)
            t0 = time.perf_counter()
            for _ in range(3):
                both()
            hip.hipStreamSynchronize(s_in); hip.hipStreamSynchronize(s_out)
            bus = 2 * n * 3 / (time.perf_counter() - t0) / 1e9
            hip.hipFree(d0); hip.hipFree(d1)
            bd = nn.BatchDenoiser(S)
            L = _ffi.PcmLayout(fmt, 1, 0, 0, fps * 480, 480)
            call = lambda: lib.check(lib.L.nnn_batch_process_pcm_host(bd._h, _ffi.ptr(px), _ffi.ptr(po), _ffi.ptr(pv), fps, C.byref(L)))
            call()
            t0 = time.perf_counter()
            for _ in range(calls):
                call()
            dt_s = (time.perf_counter() - t0) / calls
            gbs = 2 * n / dt_s / 1e9
            out[f"{name}_{S}"] = {"streams": S, "value": S * fps / dt_s, "ms_per_call": dt_s * 1e3, "bus_GBps_both_ways": gbs,
                                  "link_peak_GBps_both_ways": bus, "frac_of_link": gbs / bus}
            bd.close()
            del px, po, pv
    out["f32"], out["i16"] = out["f32_4096"], out["i16_4096"]   # (the keys earlier rounds' lines carried)
    print(json.dumps(out), flush=True)


def host_boundary(fps):
    """The host-buffer entry point (the shape of the reference's own process_frame: host slices in, host slices out) measured in a child
    process: this one holds torch's runtime and gigabytes of resident pools, which cost the transfers a quarter of their rate (round 4's
    line said 14.6 M f32 where a clean process measures 20)."""
    time.sleep(3.0)   # (the driver clears the tens of gigabytes this process has just freed with the copy engines: let it finish, see the child)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--host-boundary-child", str(fps)], capture_output=True, text=True, timeout=600)
    for ln in reversed(r.stdout.strip().split("\n")):
        if ln.startswith("{"):
            return json.loads(ln)
    return {"error": (r.stderr or r.stdout)[-400:]}


def single_process(args):
    """--single-process: the node object (nnn_node_*) drives every GPU of the node from this one process; buffers resident on each
    shard's own device, calls asynchronous, one synchronize per step batch.  Same metric, same per-GPU share as the launcher path."""
    import torch
    import nnnoiseless_amd as nn
    from nnnoiseless_amd.synthetic import make_streams_device
    cfg = CONFIGS[args.config]
    N, S1, fps, K, W = args.gpus, args.streams or cfg["streams"], args.frames_per_step, args.steps, args.warmup
    if torch.cuda.device_count() < N:
        raise SystemExit(f"bench: --gpus {N} --single-process but only {torch.cuda.device_count()} devices visible")
    model = nn.RnnModel.from_bytes(open(args.model or cfg["model"], "rb").read()) if (args.model or cfg["model"]) else None
    node = nn.NodeDenoiser(S1 * N, list(range(N)), model=model)
    pool = 2 * fps
    parts = []
    for i, (d, lo, hi) in enumerate(node.shards()):
        dev = torch.device("cuda", d)
        x = make_streams_device(torch, dev, hi - lo, pool, seed=i)
        parts.append((x, torch.empty_like(x), torch.empty((pool, hi - lo), dtype=torch.float32, device=dev)))
    for i in range(N):
        nn.library().check(nn.library().L.nnn_batch_set_inputs_ready(node.batch_handle(i), 1))

    def step(j):
        f0 = (j % 2) * fps
        node.process_device([p[0].data_ptr() + f0 * 480 * 4 for p in parts], [p[1].data_ptr() + f0 * 480 * 4 for p in parts],
                            [p[2].data_ptr() + f0 * (p[2].shape[1]) * 4 for p in parts], fps, pool * 480, 480)

    def sync():
        node.synchronize()
        for d in range(N):
            torch.cuda.synchronize(d)

    sync()
    for j in range(W):
        step(j)
    sync()
    t0 = time.perf_counter()
    for j in range(W, W + K):
        step(j)
    # every shard's own finishing time, taken in shard order (shard i's stamp is an upper bound: it is read after shards < i have
    # drained): a slow GPU shows as a low rate from its index on
    lib = nn.library()
    shard_dt = []
    for i in range(N):
        lib.check(lib.L.nnn_batch_synchronize(node.batch_handle(i)))
        shard_dt.append(time.perf_counter() - t0)
    sync()
    dt = time.perf_counter() - t0
    if node.fault():
        raise SystemExit("bench: the library reports a frame hand-off fault: results invalid")
    line = {"metric": "480-sample frames/sec (whole node) at N concurrent streams", "value": S1 * N * fps * K / dt, "unit": "frames/s", "n_gpus": N,
            "steps": K, "warmup": W, "ms_per_step": dt * 1e3 / K, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32",
            "data": "synthetic",
            "config": {"workload": f"{cfg['name']}, synthetic 48 kHz sine+noise, {fps} frame(s) per stream per step", "baseline_config_index": args.config,
                       "streams_per_gpu": S1, "streams_total": S1 * N, "frames_per_step": fps,
                       "parallelism": f"streams sharded x{N} inside the library (nnn_node_*: one batch and one host thread per device), ONE process, "
                                      "no data-path collective", "shards": node.shards()},
            "per_rank_frames_per_s": [round(S1 * fps * K / max(t, 1e-9)) for t in shard_dt],
            "worker_cpus": [node.shard_cpus(i) for i in range(N)],
            "outputs_finite": all(bool(torch.isfinite(p[1]).all().item()) for p in parts), "timed_s": dt}
    print(json.dumps(line), flush=True)
    node.close()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--host-boundary-child":
        return host_boundary_child(sys.argv[2:])
    args = parse_args()
    if args.config == 0:
        return config0()
    if args.single_process:
        return single_process(args)
    env_world = os.environ.get("WORLD_SIZE")
    if args.gpus > 1 and env_world is None:
        # not under a launcher: start one rank per GPU ourselves
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        sys.exit(subprocess.call(cmd, env=env))
    world = int(env_world or "1")
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if rank == 0:
            print(f"bench: --gpus {args.gpus} but WORLD_SIZE={world}: refusing to report a line whose n_gpus is not the number of ranks", file=sys.stderr)
        sys.exit(2)

    import torch
    import torch.distributed as dist
    if args.dry_run:
        dev = torch.device("cpu")
        if world > 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            dist.init_process_group(backend="gloo")
    else:
        if torch.cuda.device_count() <= local_rank:
            print(f"bench: rank {rank} wants GPU {local_rank} but only {torch.cuda.device_count()} visible", file=sys.stderr)
            sys.exit(2)
        torch.cuda.set_device(local_rank)
        dev = torch.device("cuda", local_rank)
        if world > 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            dist.init_process_group(backend="nccl", device_id=dev)   # "nccl" is RCCL on ROCm
    ranks_seen = 1
    if world > 1:
        one = torch.ones(1, dtype=torch.int32, device=dev)
        dist.all_reduce(one)
        ranks_seen = int(one.item())
        if ranks_seen != args.gpus:
            if rank == 0:
                print(f"bench: all-reduce saw {ranks_seen} ranks, --gpus says {args.gpus}", file=sys.stderr)
            sys.exit(2)

    if args.workload == "train":
        return bench_train(args, rank, world, dev, local_rank, dist)
    if args.workload == "resample":
        return bench_resample(args, rank, world, dev, local_rank, dist)
    cfg = CONFIGS[args.config]
    S = args.streams or cfg["streams"]
    if args.dry_run:
        S = args.streams or 6
        args.frames_per_step = min(args.frames_per_step, 3)
        args.steps, args.warmup = min(args.steps, 2), min(args.warmup, 1)
    model_path = args.model or cfg["model"]
    res, roof = measure(args, S, model_path, rank, world, dev, local_rank, dist, torch, want_tick=args.full and not args.no_tick,
                        want_roofline=args.full and not args.no_roofline, dump_dir=args.dump_outputs)
    # Every collective of the run is behind us (the aggregation inside measure): the ranks part here, and what only rank 0
    # reports -- the event-instrumented pass, the other configurations, the host-buffer rates, the CPU baseline -- runs with no
    # other rank waiting behind a barrier for it.
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if rank != 0:
        return
    if roof:
        res.update(roof())

    default_run = (args.full and args.config == 2 and args.streams is None and args.model is None and world == 1 and args.pcm == "f32"
                   and args.channels == 1 and not args.dry_run)
    also = None
    if default_run and not args.no_also:
        # the other single-GPU configurations of BASELINE.json, measured the same way (each for at least --min-timed-s), so the
        # driver's line carries them
        also = {}
        for c in (1, 4):
            a = argparse.Namespace(**vars(args))
            a.steps, a.warmup = min(args.steps, 12), max(2, min(args.warmup, 6))
            r, rf = measure(a, CONFIGS[c]["streams"], CONFIGS[c]["model"], rank, world, dev, local_rank, dist, torch, want_tick=(c == 1 and not args.no_tick),
                            want_roofline=not args.no_roofline, min_timed_s=args.min_timed_s)
            if rf:
                r.update(rf())
            also[f"configs[{c}]"] = {
                "workload": CONFIGS[c]["name"], "parity": CONFIGS[c].get("parity", "oracle pinned by the reference's golden pair (built-in model)"),
                "value": r["value"], "unit": "frames/s", "steps": r["steps"], "warmup": a.warmup,
                "ms_per_step": r["ms_per_step"], "timed_s": r["timed_s"], "frames_per_step": args.frames_per_step,
                "outputs_finite": r["outputs_finite"], "pool_frames": r["pool_frames"], "tick": r.get("tick"),
                "pipeline_hbm_frac": r["value"] * BYTES_PER_FRAME_FUSED / 1e9 / HBM_PEAK_GBS,
                "kernels_us_per_frame": {k: round(v["us_per_frame"], 2) for k, v in r.get("kernels", {}).items()},
                "roofline": r.get("roofline")}

    default_semantics = None
    if default_run and not args.no_overlap and not args.no_also:
        # the same headline workload under the library's default call ordering (no promise about the inputs: every call waits for
        # the previous one to drain before it reads its input), quoted beside the headline
        a = argparse.Namespace(**vars(args))
        a.no_overlap = True
        a.steps, a.warmup = min(args.steps, 12), min(args.warmup, 2)
        r, _ = measure(a, S, model_path, rank, world, dev, local_rank, dist, torch, want_tick=False, want_roofline=False, min_timed_s=args.min_timed_s)
        default_semantics = {"inputs_ready": False, "value": r["value"], "unit": "frames/s", "steps": r["steps"], "ms_per_step": r["ms_per_step"],
                             "timed_s": r["timed_s"]}

    host = None
    if default_run and not args.no_host:
        host = host_boundary(args.frames_per_step)

    cpu = None
    if args.full and not args.no_cpu_baseline and not args.dry_run:
        cpu = cpu_baseline()

    fps = args.frames_per_step
    line = {
        "metric": "480-sample frames/sec (whole node) at N concurrent streams", "value": res["value"], "unit": "frames/s",
        "n_gpus": args.gpus, "steps": args.steps, "warmup": args.warmup, "ms_per_step": res["ms_per_step"], "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": f"{cfg['name'] if S == cfg['streams'] else f'{S} concurrent mono streams per GPU (custom --streams)'}"
                               f"{'' if model_path == cfg['model'] else ', model ' + os.path.basename(model_path or 'built-in')}, "
                               f"synthetic 48 kHz sine+noise, {fps} frame(s) per stream per step",
                   "baseline_config_index": args.config,
                   "parity": cfg.get("parity", "oracle pinned by the reference's golden pair (built-in model)"),
                   "model": os.path.basename(model_path) if model_path else "built-in weights.rnn",
                   "boundary_format": {"f32": "f32 planar (process_frame's own)", "i16": "packed int16",
                                       "unit": "unit-range f32"}[args.pcm] + (f", {args.channels} interleaved channels" if args.channels > 1 else ""),
                   "streams_per_gpu": S, "streams_total": S * world, "frames_per_step": fps,
                   "inputs_ready": not args.no_overlap,
                   # the library's own choice unless the environment asks: up to 16 384 streams the high-pass chain on a stream of its own ahead of
                   # one lane; above that two groups in flight -- one stream per stage for calls of two groups, two lanes for longer ones (round 6)
                   "schedule": os.environ.get("NNN_SCHED", "lanes" if ((S + 63) // 64 * 64 <= 16384 or "NNN_LANES" in os.environ)
                                              else ("stages" if fps <= 48 else "lanes")) if fps >= 32 else "seq",
                   "lanes": int(os.environ.get("NNN_LANES", "1" if (S + 63) // 64 * 64 <= 16384 else "2")),
                   "inputs": "resident in HBM and final before the timed region" + ("" if args.no_overlap else "; declared to the library "
                             "(nnn_batch_set_inputs_ready): with the lanes schedule consecutive calls overlap at their boundary, outputs stay stream-ordered"),
                   "parallelism": f"streams sharded x{world}, one process per GPU, no data-path collective"},
        "ranks_seen": ranks_seen, "per_rank_frames_per_s": res["per_rank_frames_per_s"], "timed_s": res["timed_s"], "pool_frames": res["pool_frames"],
        "tick": res.get("tick"),
        "host_enqueue_ms_per_step": res["host_enqueue_ms_per_step"],
        "outputs_finite": res["outputs_finite"],
        "roofline": res.get("roofline"), "cpu_baseline": cpu, "kernels": res.get("kernels", {}), "also": also,
        "default_semantics": default_semantics, "host_boundary": host,
        # like-for-like across rounds whatever the default --config is: configs[1] (4096 streams x 48 frames) under a key that never moves
        "configs1_value": (res["value"] if args.config == 1 and S == CONFIGS[1]["streams"] else (also or {}).get("configs[1]", {}).get("value")),
    }
    if args.dry_run:
        line["dry_run"] = "gloo + CPU tensors + NNN_LIBRARY build: plumbing only, numbers meaningless"
    print(json.dumps(line), flush=True)


def bench_train(args, rank, world, dev, local_rank, dist):
    """Training-feature rows per second: three feature states per stream, no RNN, no synthesis."""
    import torch
    from nnnoiseless_amd.shard import aggregate
    from nnnoiseless_amd.synthetic import make_streams_device
    from nnnoiseless_amd.training import ROW_WIDTH, TrainingFeatures
    S, fps, K, W = args.streams or 4096, args.frames_per_step, args.steps, args.warmup
    pool = max(fps, 16)
    sig = make_streams_device(torch, dev, S, pool, seed=rank)
    noise = make_streams_device(torch, dev, S, pool, seed=1000 + rank) * 0.3
    comb = sig + noise
    cutoff = torch.full((pool, S), 20, dtype=torch.int32, device=dev)
    vad = torch.ones((pool, S), dtype=torch.float32, device=dev)
    rows = torch.empty((pool, S, ROW_WIDTH), dtype=torch.float32, device=dev)
    tf = TrainingFeatures(S, device=local_rank)
    stream = torch.cuda.current_stream().cuda_stream

    def step():
        tf.process_device(sig.data_ptr(), noise.data_ptr(), comb.data_ptr(), cutoff.data_ptr(), vad.data_ptr(), rows.data_ptr(),
                          fps, pool * 480, 480, stream)

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(W):
        step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(K):
        step()
    barrier()
    elapsed = time.perf_counter() - t0
    done, tmax = aggregate(dist if world > 1 else None, S * fps * K, elapsed, dev)
    if rank == 0:
        print(json.dumps({
            "metric": "training rows/sec (87 columns; 3 feature states per row)", "value": done / tmax, "unit": "rows/s",
            "n_gpus": args.gpus, "steps": K, "warmup": W, "ms_per_step": tmax * 1e3 / K, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"{S} (clean, noise, mix) stream triples per GPU, {fps} frame(s) per step (src/training.rs:113-160)",
                       "streams_per_gpu": S, "frames_per_step": fps},
            "outputs_finite": bool(torch.isfinite(rows).all().item())}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()




def bench_resample(args, rank, world, dev, local_rank, dist):
    """Output samples per second of the batched 16-tap sinc resampler (src/nnnoiseless.rs:106-131), 44.1 kHz -> 48 kHz, device
    buffers: one step = every stream fed 0.48 s of source audio (21 168 samples).  Per output sample the kernel reads 16 taps
    (from L1 / L2: 4 new source bytes per output from HBM) and 16 f64 weights shared by all streams, and writes 4 bytes."""
    import ctypes as C
    import torch
    import nnnoiseless_amd as nn
    from nnnoiseless_amd.shard import aggregate
    lib = nn.library()
    S, K, W = args.streams or 4096, args.steps, args.warmup
    n_in = 21168
    r = lib.L.nnn_resampler_create(S, 44100.0 / 48000.0, local_rank)
    if not r:
        raise SystemExit("bench: " + lib.error())
    cap = lib.L.nnn_resampler_max_output(r, n_in)
    x = torch.randn((S, n_in), device=dev) * 3000.0
    y = torch.empty((S, cap), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    n_out = C.c_long(0)

    def step():
        lib.check(lib.L.nnn_resampler_process_device(r, x.data_ptr(), n_in, n_in, y.data_ptr(), cap, cap, C.byref(n_out), stream))
        return n_out.value

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(W):
        step()
    barrier()
    t0 = time.perf_counter()
    produced = sum(step() for _ in range(K))
    barrier()
    elapsed = time.perf_counter() - t0
    done, tmax = aggregate(dist if world > 1 else None, S * produced, elapsed, dev)
    lib.L.nnn_resampler_destroy(r)
    if rank == 0:
        bytes_per_out = 4 + 4 * 44100.0 / 48000.0      # one output written, 0.92 new source samples read
        print(json.dumps({
            "metric": "resampler output samples/sec (44.1 kHz -> 48 kHz, 16-tap sinc)", "value": done / tmax, "unit": "samples/s",
            "n_gpus": args.gpus, "steps": K, "warmup": W, "ms_per_step": tmax * 1e3 / K, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32 (f64 tap weights)", "data": "synthetic",
            "config": {"workload": f"{S} mono streams per GPU, {n_in} source samples (0.48 s) per stream per step (src/nnnoiseless.rs:106-131)",
                       "streams_per_gpu": S},
            "equivalent_frames_per_s": done / tmax / 480.0,
            "roofline": {"bound": "hbm", "achieved": done / tmax * bytes_per_out / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": done / tmax * bytes_per_out / 1e9 / HBM_PEAK_GBS, "traffic": None,
                         "note": "algorithmic bytes: 4 written + 3.7 read per output sample; the position schedule and tap weights of a call "
                                 "are computed on the host (f64) and uploaded per call"},
            "outputs_finite": bool(torch.isfinite(y[:, :n_out.value]).all().item())}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()

if __name__ == "__main__":
    main()
