"""Shared by the trainer's tests (include/nnn_fit.h): the restatement of the network, the loss and the gradient
in PyTorch autograd on the CPU, in float64 (the checker) and float32 (the yardstick of the checker's own arithmetic), Adam and the
quantisation in NumPy, the case builders, and the checks the interpreter tests and the GPU tests both make.

The rule for everything compared with float64: relative error (L2 norm of the difference over the L2 norm of the float64 value) at
most 8 x the float32 restatement's error against the same float64 values, the bound never taken below 1e-6.  Per tensor for the
fifteen gradient tensors, per output array for the outputs, per term for the loss terms.  Every check prints both errors."""
import functools
import os

import numpy as np

from conftest import GOLDEN, WEIGHTS

NP_, NF, NB = 87503, 42, 22
FACTOR, FLOOR = 8.0, 1e-6
HEADER_AT = (0, 3 + 1032, 6 + 4560, 9 + 24576, 12 + 85344, 15 + 87478)   # where the six layer headers lie in a .rnn file
REF_ACTS = (0, 0, 2, 0)                                                  # train/rnn_train.py:66-75: tanh, tanh, ReLU, tanh


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def tensors():
    from nnnoiseless_amd import _ffi
    return _ffi.FIT_TENSORS


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def _acts(torch):
    return {0: torch.tanh, 1: torch.sigmoid, 2: torch.relu}


def _unpack(p):
    return {name: p[off:off + int(np.prod(shape))].reshape(shape) for name, (off, shape) in tensors().items()}


def _gru(torch, xin, W, U, b, act):
    n = U.shape[0]
    P = xin @ W + b
    h = torch.zeros(xin.shape[1], n, dtype=xin.dtype)
    out = []
    for t in range(xin.shape[0]):
        z = torch.sigmoid(P[t][:, :n] + h @ U[:, :n])
        r = torch.sigmoid(P[t][:, n:2 * n] + h @ U[:, n:2 * n])
        c = act(P[t][:, 2 * n:] + (r * h) @ U[:, 2 * n:])
        h = z * h + (1 - z) * c
        out.append(h)
    return torch.stack(out)


def network(torch, p, x, acts):
    """p: the parameter vector (tensor); x [T, S, 42]; acts: the four hidden activations' codes.  -> gains [T, S, 22], vad [T, S]."""
    A, q = _acts(torch), _unpack(p)
    d = A[acts[0]](x @ q["input_dense.W"] + q["input_dense.b"])
    hv = _gru(torch, d, q["vad_gru.W"], q["vad_gru.U"], q["vad_gru.b"], A[acts[1]])
    hn = _gru(torch, torch.cat([d, hv, x], -1), q["noise_gru.W"], q["noise_gru.U"], q["noise_gru.b"], A[acts[2]])
    hd = _gru(torch, torch.cat([hv, hn, x], -1), q["denoise_gru.W"], q["denoise_gru.U"], q["denoise_gru.b"], A[acts[3]])
    g = torch.sigmoid(hd @ q["denoise_output.W"] + q["denoise_output.b"])
    v = torch.sigmoid(hv @ q["vad_output.W"] + q["vad_output.b"])[..., 0]
    return g, v


def loss_terms(torch, p, g, pv, rows, w, reg):
    """The five figures of nnn_fit_losses, as the header states them."""
    dt = g.dtype
    lo = torch.tensor(float(np.float32(1e-7)), dtype=dt)
    hi = torch.tensor(float(np.float32(1) - np.float32(1e-7)), dtype=dt)
    y, v = rows[..., NF:NF + NB], rows[..., 86]

    def ce(a, o):
        return -(a * torch.log(o) + (1 - a) * torch.log(1 - o))

    m = torch.minimum(y + 1, torch.ones((), dtype=dt))
    e = torch.sqrt(g) - torch.sqrt(torch.clamp(y, min=0))
    Lg = (m * (10 * e ** 4 + e ** 2 + 0.01 * ce(g, torch.minimum(torch.maximum(y, lo), hi)))).mean(-1)
    Lv = 2 * torch.abs(v - 0.5) * ce(pv, torch.minimum(torch.maximum(v, lo), hi))
    msse = (m * e ** 2).mean(-1)
    q = _unpack(p)
    sq = sum((q[f"{l}_gru.{k}"] ** 2).sum() for l in ("vad", "noise", "denoise") for k in ("W", "U"))
    gain, vad, regt = 10 * (w * Lg).mean(), 0.5 * (w * Lv).mean(), float(np.float32(reg)) * sq
    return gain + vad + regt, gain, vad, regt, (w * msse).mean()


def restate(params, rows, w, acts, dtype, reg=1e-6):
    """Forward, loss and gradient in `dtype` ("float64" / "float32").  rows [T, S, 87], w [T, S] or None.  Everything as float64 arrays."""
    import torch
    dt = getattr(torch, dtype)
    p = torch.tensor(np.asarray(params, np.float32), dtype=dt, requires_grad=True)
    r = torch.tensor(np.asarray(rows, np.float32), dtype=dt)
    wt = torch.ones(r.shape[:2], dtype=dt) if w is None else torch.tensor(np.asarray(w, np.float32), dtype=dt)
    g, pv = network(torch, p, r[..., :NF], acts)
    terms = loss_terms(torch, p, g, pv, r, wt, reg)
    terms[0].backward()
    return {"gains": g.detach().numpy().astype(np.float64), "vad": pv.detach().numpy().astype(np.float64),
            "losses": np.array([float(t.detach()) for t in terms]), "grad": p.grad.numpy().astype(np.float64)}


def adam_restated(p, m, v, grad, t, lr=1e-3, b1=0.9, b2=0.999, eps=1e-7, clip=0.499):
    """One step of k_fit_adam in NumPy float32: lr_t in float64 from the float32 settings, then one IEEE operation per statement."""
    f = np.float32
    lr, b1, b2, eps, clip = f(lr), f(b1), f(b2), f(eps), f(clip)
    lr_t = f(np.float64(lr) * np.sqrt(1.0 - np.float64(b2) ** t) / (1.0 - np.float64(b1) ** t))
    g = grad.astype(f)
    m = b1 * m + (f(1) - b1) * g
    v = b2 * v + (f(1) - b2) * (g * g)
    p = p - (lr_t * m) / (np.sqrt(v) + eps)
    p = np.minimum(np.maximum(p, -clip), clip)
    assert p.dtype == m.dtype == v.dtype == np.float32
    return p, m, v


def dump_restated(params, header):
    """train/dump_rnn.py in NumPy: clip(round-half-even(256 x), -128, 127) behind each layer's three header bytes."""
    q = np.clip(np.rint(256.0 * np.asarray(params, np.float64)), -128, 127).astype(np.int8)
    first = [0, 1032, 4560, 24576, 85344, 87478, NP_]
    out = bytearray()
    for l in range(6):
        out += bytes(header[l]) + q[first[l]:first[l + 1]].tobytes()
    return bytes(out)


def header_of(rnn):
    return [tuple(rnn[a:a + 3]) for a in HEADER_AT]


def params_of(rnn):
    """The int8 values of a .rnn file in parameter order."""
    b = np.frombuffer(rnn, np.int8)
    first = [0, 1032, 4560, 24576, 85344, 87478, NP_]
    return np.concatenate([b[HEADER_AT[l] + 3:HEADER_AT[l] + 3 + first[l + 1] - first[l]] for l in range(6)])


# ---- case builders ------------------------------------------------------------------------------------------------------------------------
def make_rows(seed, S, T):
    """Features N(0, variance 2); targets uniform in [0, 1] with a fifth at -1 and a twentieth each at exactly 0 and exactly 1 (the
    clip bounds); labels from {0, 0.5, 1}; weights uniform in [0, 2] with a tenth at 0.  All float32."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((T, S, 87), np.float32)
    rows[..., :NF] = rng.normal(0.0, np.sqrt(2.0), (T, S, NF))
    y = rng.uniform(0, 1, (T, S, NB))
    u = rng.uniform(0, 1, (T, S, NB))
    y[u < 0.2] = -1.0
    y[(u >= 0.2) & (u < 0.25)] = 0.0
    y[(u >= 0.25) & (u < 0.3)] = 1.0
    rows[..., NF:NF + NB] = y
    rows[..., 64:86] = rng.uniform(0, 1, (T, S, NB))
    rows[..., 86] = rng.choice([0.0, 0.5, 1.0], (T, S))
    w = rng.uniform(0, 2, (T, S))
    w[rng.uniform(0, 1, (T, S)) < 0.1] = 0.0
    return rows, w.astype(np.float32)


def template_bytes(kind):
    if kind == "builtin":
        return open(WEIGHTS, "rb").read()
    if kind == "sh":
        return open(os.path.join(GOLDEN, "sh.rnn"), "rb").read()
    return None


def make_params(kind, seed=7):
    """Glorot parameters with the reference's activations, or a model / 256 plus up to +-1/1024 (no multiples of 1/256) with its own."""
    from nnnoiseless_amd import fit
    rng = np.random.default_rng(seed)
    if kind == "glorot":
        return fit.glorot_params(rng), REF_ACTS
    rnn = template_bytes(kind)
    p = params_of(rnn).astype(np.float32) / np.float32(256) + rng.uniform(-1 / 1024, 1 / 1024, NP_).astype(np.float32)
    return p.astype(np.float32), tuple(h[2] for h in header_of(rnn)[:4])


class Case:
    pass


@functools.lru_cache(maxsize=None)
def case(S, T, kind="glorot", seed=3):
    c = Case()
    c.S, c.T, c.kind = S, T, kind
    c.rows, c.w = make_rows(seed + 100 * S + T, S, T)
    c.params, c.acts = make_params(kind)
    c.ref64 = restate(c.params, c.rows, c.w, c.acts, "float64")
    c.ref32 = restate(c.params, c.rows, c.w, c.acts, "float32")
    return c


def trainer_for(lib, c, max_seq=None, max_window=None):
    from nnnoiseless_amd.fit import Trainer
    t = Trainer(template_bytes(c.kind), max_seq=max_seq or c.S, max_window=max_window or c.T, lib=lib)
    t.set_params(c.params)
    return t


# ---- the rule -------------------------------------------------------------------------------------------------------------------------------
def rel_err(a, ref):
    a, ref = np.asarray(a, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    den = np.sqrt((ref ** 2).sum())
    num = np.sqrt(((a - ref) ** 2).sum())
    return num / den if den > 0 else num


def held(tag, got, ref64, ref32):
    """Prints both errors and returns whether `got` is inside the rule."""
    e, e32 = rel_err(got, ref64), rel_err(ref32, ref64)
    bound = max(FACTOR * e32, FLOOR)
    print(f"{tag}: error {e:.3g}, float32 restatement {e32:.3g}, bound {bound:.3g}, ratio to the restatement {e / e32 if e32 > 0 else float('inf'):.3g}")
    return e <= bound


def check_case(lib, S, T, kind="glorot"):
    """Forward outputs, loss terms (from loss and from grad: the same bits) and the fifteen gradient tensors against float64."""
    from nnnoiseless_amd.fit import LOSS_NAMES
    c = case(S, T, kind)
    tr = trainer_for(lib, c)
    if kind == "builtin":   # the activations come from the template's header bytes: the built-in model's are not the reference script's
        assert c.acts == (0, 2, 2, 2) != REF_ACTS
    bad = []
    gains, vad = tr.forward(c.rows)
    assert gains.shape == (T, S, NB) and vad.shape == (T, S)
    for name, got in (("gains", gains), ("vad", vad)):
        if not held(f"{S}x{T} {kind} {name}", got, c.ref64[name], c.ref32[name]):
            bad.append(name)
    l_val = tr.loss(c.rows, c.w)
    l_grad = tr.grad(c.rows, c.w)
    assert l_val == l_grad
    for i, name in enumerate(LOSS_NAMES):
        if not held(f"{S}x{T} {kind} loss.{name}", l_grad[name], c.ref64["losses"][i], c.ref32["losses"][i]):
            bad.append("loss." + name)
    g = tr.gradient()
    assert np.isfinite(g).all()
    for name, (off, shape) in tensors().items():
        n = int(np.prod(shape))
        if not held(f"{S}x{T} {kind} d {name}", g[off:off + n], c.ref64["grad"][off:off + n], c.ref32["grad"][off:off + n]):
            bad.append(name)
    tr.close()
    assert not bad, bad


def check_template_start(lib):
    """A template's weights / 256 are the starting parameters; NULL starts from zero with the reference's activations."""
    from nnnoiseless_amd.fit import Trainer
    for kind in ("builtin", "sh"):
        rnn = template_bytes(kind)
        t = Trainer(rnn, max_seq=2, max_window=2, lib=lib)
        assert np.array_equal(t.params(), params_of(rnn).astype(np.float32) / np.float32(256))
        assert header_of(t.export_rnn()) == header_of(rnn) and t.export_rnn() == rnn
        t.close()
    t = Trainer(None, max_seq=2, max_window=2, lib=lib)
    assert not t.params().any() and t.step_count() == 0
    assert [h[2] for h in header_of(t.export_rnn())] == [0, 0, 2, 0, 1, 1]
    assert t.settings() == {k: float(np.float32(v)) for k, v in (("lr", 1e-3), ("beta1", 0.9), ("beta2", 0.999), ("epsilon", 1e-7), ("reg", 1e-6), ("clip", 0.499))}
    t.close()


def _grad_state(tr):
    return [bits(tr.gradient()), tr.losses()]


def check_independence(lib):
    """Nothing depends on the allocation or on earlier calls; [T][S] and [S][T] addressing, a repeated call and w = NULL against ones
    give the same bits."""
    from nnnoiseless_amd import _ffi
    from nnnoiseless_amd.fit import TILE
    big, small = case(TILE + 1, 40), case(3, 5)
    used = trainer_for(lib, big)
    used.grad(big.rows, big.w)
    used.forward(big.rows)
    fresh = trainer_for(lib, small)

    def all_of(tr):
        gains, vad = tr.forward(small.rows)
        l = tr.loss(small.rows, small.w)
        tr.grad(small.rows, small.w)
        return [bits(gains), bits(vad), l] + _grad_state(tr)

    a, b = all_of(used), all_of(fresh)
    for x, y in zip(a, b):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y
    again = _grad_state(fresh)
    fresh.grad(small.rows, small.w)
    assert np.array_equal(_grad_state(fresh)[0], again[0]) and _grad_state(fresh)[1] == again[1]
    # the reference's [S][T][87] through the strides (device entry; the interpreter's device memory is the host's)
    st = np.ascontiguousarray(small.rows.transpose(1, 0, 2))
    wst = np.ascontiguousarray(small.w.T)
    rows_dev, w_dev = to_device(lib, st), to_device(lib, wst)
    fresh.grad_device(rows_dev[0], small.S, small.T, w_dev[0], frame_stride=87, seq_stride=small.T * 87, w_frame_stride=1, w_seq_stride=small.T)
    got = _grad_state(fresh)
    assert np.array_equal(got[0], again[0]) and got[1] == again[1]
    del rows_dev, w_dev
    # no weights = all-ones weights
    fresh.grad(small.rows, None)
    none = _grad_state(fresh)
    fresh.grad(small.rows, np.ones_like(small.w))
    ones = _grad_state(fresh)
    assert np.array_equal(none[0], ones[0]) and none[1] == ones[1] and not np.array_equal(none[0], again[0])
    used.close(), fresh.close()


def to_device(lib, a):
    """(pointer, keep-alive) of array `a` where the library's kernels can read it: the array itself under the interpreter, a torch
    tensor on the GPU."""
    if "hostsim" in os.path.basename(lib.path):
        a = np.ascontiguousarray(a)
        return a.ctypes.data, a
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t.data_ptr(), t


def check_optimizer(lib):
    """Three grad + step rounds from parameters just inside the clip with a gradient that pushes outward: parameters and both moments
    equal the NumPy float32 restatement (fed the gradient read back) bit for bit, the clip engages, and a second trainer continues
    from state() bit for bit."""
    c = case(3, 5)
    tr = trainer_for(lib, c)
    tr.grad(c.rows, c.w)
    g0 = tr.gradient()
    p = c.params.copy()
    push = np.flatnonzero(g0 != 0)[::3]
    p[push] = np.where(g0[push] < 0, np.float32(0.4985), np.float32(-0.4985))   # Adam moves against the gradient: outward
    tr.set_params(p)
    m, v = np.zeros(NP_, np.float32), np.zeros(NP_, np.float32)
    clipped = 0
    other = None
    for t in (1, 2, 3):
        tr.grad(c.rows, c.w)
        g = tr.gradient()
        tr.step()
        p_before = p
        p, m, v = adam_restated(p, m, v, g, t)
        unclipped = p_before - (np.float32(np.float64(np.float32(1e-3)) * np.sqrt(1.0 - np.float64(np.float32(0.999)) ** t) / (1.0 - np.float64(np.float32(0.9)) ** t)) * m) / (np.sqrt(v) + np.float32(1e-7))
        clipped += int((np.abs(unclipped) > np.float32(0.499)).sum())
        s = tr.state()
        assert s["step"] == t
        for name, want in (("params", p), ("m", m), ("v", v)):
            assert np.array_equal(bits(s[name]), bits(want)), (t, name, int((bits(s[name]) != bits(want)).sum()))
        if t == 2:
            other = trainer_for(lib, c)
            other.load_state(s)
    assert clipped > 0 and (np.abs(p) == np.float32(0.499)).any()
    other.grad(c.rows, c.w)
    other.step()
    so, st = other.state(), tr.state()
    assert so["step"] == st["step"] == 3
    for name in ("params", "m", "v"):
        assert np.array_equal(bits(so[name]), bits(st[name])), name
    tr.close(), other.close()


def check_export(lib):
    """export_rnn = the dump_rnn rule in NumPy, ties and both ends included; the file parses and keeps the template's activation bytes;
    set_params(q / 256) exports the same bytes; a NaN refuses."""
    import pytest
    import nnnoiseless_amd as nn
    from nnnoiseless_amd import _ffi
    from nnnoiseless_amd.fit import Trainer
    rng = np.random.default_rng(5)
    p = rng.uniform(-0.6, 0.6, NP_).astype(np.float32)
    planted = {0: (0.5 / 256, 0), 1: (1.5 / 256, 2), 2: (-2.5 / 256, -2), 3: (0.499, 127), 4: (-0.499, -128), 5: (-0.5 / 256, 0), 6: (126.5 / 256, 126)}
    for i, (x, _) in planted.items():
        p[i] = np.float32(x)
    for kind in ("sh", None):
        rnn = template_bytes(kind)
        tr = Trainer(rnn, max_seq=2, max_window=2, lib=lib)
        tr.set_params(p)
        out = tr.export_rnn()
        header = header_of(rnn) if rnn else [(42, 24, 0), (24, 24, 0), (90, 48, 2), (114, 96, 0), (96, 22, 1), (24, 1, 1)]
        assert len(out) == 87521 and out == dump_restated(p, header)
        q = params_of(out)
        for i, (_, want) in planted.items():
            assert q[i] == want, (i, q[i], want)
        assert q.min() == -128 and q.max() == 127
        model = nn.RnnModel.from_bytes(out, lib=lib)
        assert model is not None and model.shape()[6:] == [h[2] for h in header]
        tr.set_params(q.astype(np.float32) / np.float32(256))
        assert tr.export_rnn() == out
        bad = p.copy()
        bad[1000] = np.nan
        with pytest.raises(RuntimeError, match="not finite"):
            tr.set_params(bad)
        assert tr.export_rnn() == out
        tr.close()


def smooth_rows(seed, S, T):
    """Rows whose targets are a fixed smooth function of the features."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((T, S, 87), np.float32)
    x = rng.normal(0.0, 1.0, (T, S, NF))
    rows[..., :NF] = x
    mix = np.random.default_rng(99).normal(0, 0.4, (NF, NB))
    rows[..., NF:NF + NB] = 1 / (1 + np.exp(-(x @ mix)))
    rows[..., 86] = np.where(x[..., 0] > 0.5, 1.0, np.where(x[..., 0] < -0.5, 0.0, 0.5))
    return rows


def check_end_to_end(lib, rounds=30):
    """(8, 16): 30 grad + step rounds bring the loss below its start, for the library and for the float64 twin alike; the exported model
    loads into a BatchDenoiser, and the largest difference between `network`'s gains and the trainer's forward outputs on the
    quantised parameters -- the inference path's table activations -- is printed (a measurement, no bar)."""
    import torch
    import nnnoiseless_amd as nn
    S, T = 8, 16
    rows = smooth_rows(11, S, T)
    params, acts = make_params("glorot", seed=21)
    tr = trainer_for(lib, type("C", (), {"kind": "glorot", "params": params, "S": S, "T": T}))
    first = tr.loss(rows)["total"]
    for _ in range(rounds):
        tr.grad(rows)
        tr.step()
    last = tr.loss(rows)["total"]
    # the float64 twin: the same loop on the restatement, Adam in float64
    p = torch.tensor(params, dtype=torch.float64, requires_grad=True)
    r = torch.tensor(rows, dtype=torch.float64)
    w = torch.ones(T, S, dtype=torch.float64)
    m, v, twin = torch.zeros_like(p), torch.zeros_like(p), []
    for t in range(1, rounds + 2):
        g, pv = network(torch, p, r[..., :NF], acts)
        total = loss_terms(torch, p, g, pv, r, w, 1e-6)[0]
        twin.append(float(total.detach()))
        if t > rounds:
            break
        grad, = torch.autograd.grad(total, p)
        with torch.no_grad():
            m = 0.9 * m + 0.1 * grad
            v = 0.999 * v + 0.001 * grad * grad
            p -= 1e-3 * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t) * m / (torch.sqrt(v) + 1e-7)
            p.clamp_(-0.499, 0.499)
    print(f"end to end: loss {first:.6g} -> {last:.6g} after {rounds} rounds; float64 twin {twin[0]:.6g} -> {twin[-1]:.6g}")
    assert last < first and twin[-1] < twin[0]
    assert abs(first - twin[0]) <= 1e-5 * twin[0] and abs(last - twin[-1]) <= 1e-3 * twin[-1]
    rnn = tr.export_rnn()
    tr.set_params(params_of(rnn).astype(np.float32) / np.float32(256))
    gains, vad = tr.forward(rows)
    bd = nn.BatchDenoiser(S, model=nn.RnnModel.from_bytes(rnn, lib=lib), lib=lib)
    n_gains, n_vad = bd.network(rows[..., :NF])
    print(f"end to end: network against the trainer's forward pass on the quantised parameters: gains differ by at most {np.abs(n_gains - gains).max():.3g}, "
          f"vad by at most {np.abs(n_vad - vad).max():.3g} (the inference path's table activations)")
    assert np.isfinite(n_gains).all() and n_gains.shape == gains.shape
    tr.close()


def check_refusals(lib):
    import pytest
    from nnnoiseless_amd import _ffi
    from nnnoiseless_amd.fit import Trainer
    L = lib.L
    sh = bytearray(template_bytes("sh"))
    other = other_shape()   # (a file the model parser accepts: its sizes are consistent, they are just not the reference's)
    assert not L.nnn_fit_create(other, len(other), 2, 2, 0) and "shape" in lib.error()
    assert not L.nnn_fit_create(bytes(sh[:-1]), len(sh) - 1, 2, 2, 0) and "malformed" in lib.error()
    for at in HEADER_AT[4:]:
        bad = bytearray(sh)
        bad[at + 2] = 0
        assert not L.nnn_fit_create(bytes(bad), len(bad), 2, 2, 0) and "sigmoid" in lib.error()
    assert not L.nnn_fit_create(None, 0, 0, 2, 0) and not L.nnn_fit_create(None, 0, 2, 0, 0)
    L.nnn_fit_destroy(None)
    assert L.nnn_fit_step(None, None) != 0 and L.nnn_fit_get(None, 0, None) != 0
    tr = Trainer(None, max_seq=3, max_window=4, lib=lib)
    with pytest.raises(RuntimeError, match="no gradient yet"):
        tr.step()
    rows, w = make_rows(1, 3, 4)
    buf = np.zeros(NP_, np.float32)
    fr = lambda **kw: _ffi.FitRows(**{**dict(rows=rows.ctypes.data, frame_stride=3 * 87, seq_stride=87, w=None, w_frame_stride=3, w_seq_stride=1, n_seq=3, window=4), **kw})
    import ctypes as C
    for kw in ({"n_seq": 4}, {"n_seq": 0}, {"window": 5}, {"window": 0}, {"rows": None}):
        r = fr(**kw)
        assert L.nnn_fit_grad_device(tr._h, C.byref(r), None) != 0, kw
        assert L.nnn_fit_loss_device(tr._h, C.byref(r), None) != 0, kw
        assert L.nnn_fit_forward_device(tr._h, C.byref(r), buf.ctypes.data, buf.ctypes.data, None) != 0, kw
    assert "outside" in lib.error() or "null" in lib.error()
    assert L.nnn_fit_grad_device(tr._h, None, None) != 0
    assert L.nnn_fit_forward_device(tr._h, C.byref(fr()), None, buf.ctypes.data, None) != 0
    assert L.nnn_fit_grad_host(tr._h, None, None, 3, 4) != 0 and L.nnn_fit_grad_host(tr._h, rows.ctypes.data, None, 4, 4) != 0
    assert L.nnn_fit_loss_host(tr._h, rows.ctypes.data, None, 3, 5) != 0
    assert L.nnn_fit_get(tr._h, 0, None) != 0 and L.nnn_fit_get(tr._h, 4, buf.ctypes.data) != 0 and L.nnn_fit_set(tr._h, 0, None) != 0
    assert L.nnn_fit_set(tr._h, _ffi.FIT_SEL_GRAD, buf.ctypes.data) != 0 and "cannot be set" in lib.error()
    assert L.nnn_fit_losses(tr._h, None) != 0 and L.nnn_fit_export_rnn(tr._h, buf.ctypes.data, 87520) != 0
    assert L.nnn_fit_set_step(tr._h, -1) != 0
    for sel in (_ffi.FIT_SEL_PARAMS, _ffi.FIT_SEL_ADAM_M, _ffi.FIT_SEL_ADAM_V):
        for value in (np.nan, np.inf, -np.inf):
            bad = buf.copy()
            bad[-1] = value
            assert L.nnn_fit_set(tr._h, sel, bad.ctypes.data) != 0 and "not finite" in lib.error()
    with pytest.raises(RuntimeError, match="no gradient yet"):   # nothing above left one
        tr.step()
    assert not tr.params().any() and tr.step_count() == 0
    with pytest.raises(ValueError):
        tr.grad(rows[..., :86])
    with pytest.raises(ValueError):
        tr.grad(rows, w[:2])
    with pytest.raises(ValueError):
        tr.set_params(buf[:-1])
    tr.grad(rows, w)
    tr.step()
    assert tr.step_count() == 1
    tr.close()


def other_shape():
    """A well-formed .rnn file of another shape: noise GRU 90 -> 47 and denoise GRU 113 -> 96, zero weights."""
    out = bytearray()
    for kind, nin, n, act in (("d", 42, 24, 0), ("g", 24, 24, 0), ("g", 90, 47, 2), ("g", 113, 96, 0), ("d", 96, 22, 1), ("d", 24, 1, 1)):
        out += bytes([nin, n, act]) + bytes((nin * n + n) if kind == "d" else (3 * n * nin + 3 * n * n + 3 * n))
    return bytes(out)
