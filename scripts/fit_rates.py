#!/usr/bin/env python3
"""What the network trainer costs (include/nnn_fit.h), on one GPU, timed with HIP events on the stream the calls
are made on (a stream of the caller's: torch's DEFAULT stream has handle 0, which means "the object's own stream" to the library).

  At 32 x 2000 (the reference's batch) and 256 x 2000 rows, Glorot parameters, random rows resident on the device:
    step      nnn_fit_grad_device + nnn_fit_step: ms per step and rows/s
    fwd, bwd  the recurrence kernels alone per GRU (nnn_fit_debug_recurrence): ms per launch and us per time step
    eager     the yardstick, in the same run: the same step (forward, loss, backward, Adam, clip) as a plain PyTorch float32 eager
              loop over time with autograd on the same GPU.  The reference's Keras script cannot run here, and a new call has no
              parent-commit number.
  Every timed figure is the median of --reps (5; --eager-reps 2 for the eager loop) repeats with their spread (max - min).

usage: scripts/fit_rates.py [--reps K] [--eager-reps K] [--shapes 32x2000 256x2000] [--out profiles/fit_rates.txt]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # (the host's setting, as bench.py)

NF, NB = 42, 22


def eager_step(torch, P, adam, rows, w, t):
    """One training step of the header's network and loss in eager PyTorch float32 (activations tanh, tanh, ReLU, tanh)."""
    def gru(xin, W, U, b, act):
        n = U.shape[0]
        Pj = xin @ W + b
        h = torch.zeros(xin.shape[1], n, device=xin.device)
        out = []
        for k in range(xin.shape[0]):
            z = torch.sigmoid(Pj[k][:, :n] + h @ U[:, :n])
            r = torch.sigmoid(Pj[k][:, n:2 * n] + h @ U[:, n:2 * n])
            c = act(Pj[k][:, 2 * n:] + (r * h) @ U[:, 2 * n:])
            h = z * h + (1 - z) * c
            out.append(h)
        return torch.stack(out)

    x, y, v = rows[..., :NF], rows[..., NF:NF + NB], rows[..., 86]
    d = torch.tanh(x @ P["in.W"] + P["in.b"])
    hv = gru(d, P["vad.W"], P["vad.U"], P["vad.b"], torch.tanh)
    hn = gru(torch.cat([d, hv, x], -1), P["noise.W"], P["noise.U"], P["noise.b"], torch.relu)
    hd = gru(torch.cat([hv, hn, x], -1), P["dn.W"], P["dn.U"], P["dn.b"], torch.tanh)
    g = torch.sigmoid(hd @ P["out.W"] + P["out.b"])
    p = torch.sigmoid(hv @ P["vout.W"] + P["vout.b"])[..., 0]
    lo, hi = 1e-7, 1.0 - 2.0 ** -23
    ce = lambda a, o: -(a * torch.log(o) + (1 - a) * torch.log(1 - o))
    m = torch.clamp(y + 1, max=1.0)
    e = torch.sqrt(g) - torch.sqrt(torch.clamp(y, min=0))
    Lg = (m * (10 * e ** 4 + e ** 2 + 0.01 * ce(g, torch.clamp(y, lo, hi)))).mean(-1)
    Lv = 2 * torch.abs(v - 0.5) * ce(p, torch.clamp(v, lo, hi))
    sq = sum((P[f"{l}.{k}"] ** 2).sum() for l in ("vad", "noise", "dn") for k in ("W", "U"))
    total = 10 * (w * Lg).mean() + 0.5 * (w * Lv).mean() + 1e-6 * sq
    grads = torch.autograd.grad(total, list(P.values()))
    lr_t = 1e-3 * (1 - 0.999 ** t) ** 0.5 / (1 - 0.9 ** t)
    with torch.no_grad():
        for (name, q), gq in zip(P.items(), grads):
            mo, ve = adam[name]
            mo.mul_(0.9).add_(gq, alpha=0.1)
            ve.mul_(0.999).addcmul_(gq, gq, value=0.001)
            q.sub_(lr_t * mo / (ve.sqrt() + 1e-7)).clamp_(-0.499, 0.499)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--eager-reps", type=int, default=2)
    ap.add_argument("--shapes", nargs="+", default=["32x2000", "256x2000"])
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import torch
    torch.cuda.init()
    from nnnoiseless_amd import _ffi, fit
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream()
    sp = st.cuda_stream
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(fn, stream=st):
        """ms between two events on the calls' stream around fn() (after one unmeasured fn() and a full wait)."""
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def stat(v):
        return f"{statistics.median(v):.4g} (spread {max(v) - min(v):.2g})"

    names = {"input_dense": "in", "vad_gru": "vad", "noise_gru": "noise", "denoise_gru": "dn", "denoise_output": "out", "vad_output": "vout"}
    say(f"# scripts/fit_rates.py: median of {a.reps} (eager loop: {a.eager_reps}), spread = max - min")
    for shape in a.shapes:
        S, T = (int(x) for x in shape.split("x"))
        rng = np.random.default_rng(S)
        rows_h = np.zeros((T, S, 87), np.float32)
        rows_h[..., :NF] = rng.normal(0, 1.4, (T, S, NF))
        rows_h[..., NF:NF + NB] = rng.uniform(0, 1, (T, S, NB))
        rows_h[..., 86] = rng.choice([0.0, 0.5, 1.0], (T, S))
        rows = torch.from_numpy(rows_h).to(dev)
        w = torch.from_numpy(rng.uniform(0, 2, (T, S)).astype(np.float32)).to(dev)
        params = fit.glorot_params(rng)
        tr = fit.Trainer(None, max_seq=S, max_window=T)
        tr.set_params(params)
        torch.cuda.synchronize()

        def step():
            tr.grad_device(rows.data_ptr(), S, T, w.data_ptr(), hip_stream=sp)
            tr.step(sp)

        ms = {"step": [timed(step) for _ in range(a.reps)]}
        for layer, lname in enumerate(("vad", "noise", "denoise")):
            for backward in (0, 1):
                key = f"{lname}.{'bwd' if backward else 'fwd'}"
                tr.set_params(params)   # (steps have moved the parameters; the recurrence's time does not depend on them, its NaNs might)
                tr.grad_device(rows.data_ptr(), S, T, w.data_ptr(), hip_stream=sp)
                ms[key] = [timed(lambda: tr.debug_recurrence(layer, backward, S, T, 1, sp)) for _ in range(a.reps)]
        tr.close()
        # the yardstick: the same step as an eager float32 loop, on torch's own stream
        P = {f"{names[k.split('.')[0]]}.{k.split('.')[1]}": torch.from_numpy(params[off:off + int(np.prod(shp))].reshape(shp).copy()).to(dev).requires_grad_(True)
             for k, (off, shp) in _ffi.FIT_TENSORS.items()}
        adam = {k: (torch.zeros_like(q), torch.zeros_like(q)) for k, q in P.items()}
        count = [0]

        def eager():
            count[0] += 1
            eager_step(torch, P, adam, rows, w, count[0])

        cur = torch.cuda.current_stream()
        ms["eager"] = [timed(eager, cur) for _ in range(a.eager_reps)]
        n = S * T
        say(f"{S} x {T} rows:")
        say(f"  step  (grad + step)    {stat(ms['step'])} ms; {n / statistics.median(ms['step']) / 1e3:.4g} M rows/s")
        for key in [k for k in ms if "." in k]:
            say(f"  {key:<22} {stat(ms[key])} ms a launch, {statistics.median(ms[key]) * 1e3 / T:.3g} us a time step")
        rec = sum(statistics.median(ms[k]) for k in ms if "." in k)
        say(f"  recurrence kernels together {rec:.4g} ms = {rec / statistics.median(ms['step']):.2f} of the step")
        say(f"  eager (PyTorch f32)    {stat(ms['eager'])} ms; {n / statistics.median(ms['eager']) / 1e3:.4g} M rows/s; "
            f"eager / step = {statistics.median(ms['eager']) / statistics.median(ms['step']):.1f}")
        say("  " + json.dumps({"shape": shape, "ms": ms}))
        del rows, w, P, adam
        torch.cuda.empty_cache()
    if a.out:
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
