"""The network trainer (include/nnn_fit.h): the reference's train/rnn_train.py and train/dump_rnn.py on the
device.  Rows from nnnoiseless_amd.training go in, a .rnn model comes out.

Trainer mirrors the C object: forward pass, loss, back-propagation through time and Adam for the reference's 3-GRU network over
windows of consecutive rows.  What is policy rather than arithmetic stays on the host as plain Python without a device: the
initialiser (glorot_params), the sample weights (row_weights), the cut into windows (windows), the validation split and the batch
plan, and the loop over epochs (fit; `python -m nnnoiseless_amd.fit` is its front-end).
"""
import ctypes as C

import numpy as np

from . import _ffi, library

ROW_WIDTH = 87
NB_FEATURES, NB_BANDS = 42, 22
PARAMS = _ffi.FIT_PARAMS
TILE = _ffi.FIT_TILE
TENSORS = _ffi.FIT_TENSORS
CLIP = 0.499                      # train/rnn_train.py:62
LOSS_NAMES = ("total", "gain", "vad", "reg", "msse")


class Trainer:
    """The reference's network with f32 master parameters, their gradient and Adam's moments on the device.

    template: the bytes of a .rnn file -- it fixes the activations and its weights / 256 are the starting parameters (fine-tuning) --
    or None for the reference's training set-up (tanh, tanh, ReLU, tanh) with zero parameters, to be overwritten by set_params.
    Arrays are float32 [window, n_seq, ...] (the generator's layout); the *_device methods take raw pointers and strides."""

    def __init__(self, template=None, max_seq=32, max_window=2000, device=0, lib=None):
        self._lib = lib or library()
        if not hasattr(self._lib.L, "nnn_fit_create"):
            raise RuntimeError("nnnoiseless_amd: this build of the library has no trainer (nnn_fit_*)")
        self.max_seq, self.max_window = int(max_seq), int(max_window)
        t = None if template is None else bytes(template)
        self._h = self._lib.L.nnn_fit_create(t, 0 if t is None else len(t), self.max_seq, self.max_window, device)
        if not self._h:
            raise RuntimeError("nnnoiseless_amd: " + self._lib.error())

    # ---- parameters, moments, checkpoint ----
    def _get(self, which):
        a = np.empty(PARAMS, np.float32)
        self._lib.check(self._lib.L.nnn_fit_get(self._h, which, _ffi.ptr(a)))
        return a

    def _set(self, which, values):
        a = _ffi.as_f32(values).reshape(-1)
        if a.size != PARAMS:
            raise ValueError(f"need {PARAMS} values, got {a.size}")
        self._lib.check(self._lib.L.nnn_fit_set(self._h, which, _ffi.ptr(a)))

    def params(self):
        """The parameter vector, float32 [87503], in .rnn file order without the header bytes (fit.TENSORS has the fifteen tensors)."""
        return self._get(_ffi.FIT_SEL_PARAMS)

    def set_params(self, values):
        self._set(_ffi.FIT_SEL_PARAMS, values)

    def gradient(self):
        """The gradient the last grad call left."""
        return self._get(_ffi.FIT_SEL_GRAD)

    def step_count(self):
        n = C.c_int64(0)
        self._lib.check(self._lib.L.nnn_fit_get_step(self._h, C.byref(n)))
        return int(n.value)

    def state(self):
        """The checkpoint: parameters, Adam's two moments and its step count."""
        return {"params": self.params(), "m": self._get(_ffi.FIT_SEL_ADAM_M), "v": self._get(_ffi.FIT_SEL_ADAM_V), "step": self.step_count()}

    def load_state(self, state):
        self._set(_ffi.FIT_SEL_PARAMS, state["params"])
        self._set(_ffi.FIT_SEL_ADAM_M, state["m"])
        self._set(_ffi.FIT_SEL_ADAM_V, state["v"])
        self._lib.check(self._lib.L.nnn_fit_set_step(self._h, int(state["step"])))

    def settings(self):
        s = _ffi.FitSettings()
        self._lib.check(self._lib.L.nnn_fit_get_settings(self._h, C.byref(s)))
        return {k: float(getattr(s, k)) for k, _ in _ffi.FitSettings._fields_}

    def set_settings(self, **kw):
        """lr, beta1, beta2, epsilon (Adam as Keras runs it), reg (L2 of the GRU matrices), clip."""
        cur = self.settings()
        unknown = set(kw) - set(cur)
        if unknown:
            raise ValueError(f"unknown settings {sorted(unknown)}")
        cur.update(kw)
        self._lib.check(self._lib.L.nnn_fit_set_settings(self._h, C.byref(_ffi.FitSettings(**cur))))

    def export_rnn(self):
        """The .rnn file of the current parameters: clamp(rint(256 x), -128, 127) behind the template's headers (train/dump_rnn.py)."""
        out = np.zeros(_ffi.FIT_RNN_BYTES, np.uint8)
        self._lib.check(self._lib.L.nnn_fit_export_rnn(self._h, _ffi.ptr(out), out.size))
        return out.tobytes()

    # ---- calls on arrays ----
    def _rows(self, rows, w):
        r = _ffi.as_f32(rows)
        if r.ndim != 3 or r.shape[2] != ROW_WIDTH:
            raise ValueError(f"rows must have shape [window, n_seq, {ROW_WIDTH}]")
        T, S, _ = r.shape
        if w is not None:
            w = _ffi.as_f32(w)
            if w.shape != (T, S):
                raise ValueError("weights must have shape [window, n_seq]")
        return r, w, S, T

    def forward(self, rows):
        """Gains float32 [window, n_seq, 22] and VAD [window, n_seq] of rows [window, n_seq, 87] (only the 42 features are read)."""
        r, _, S, T = self._rows(rows, None)
        gains, vad = np.empty((T, S, NB_BANDS), np.float32), np.empty((T, S), np.float32)
        self._lib.check(self._lib.L.nnn_fit_forward_host(self._h, _ffi.ptr(r), S, T, _ffi.ptr(gains), _ffi.ptr(vad)))
        return gains, vad

    def loss(self, rows, w=None):
        """Forward pass and loss terms (a validation batch); returns losses()."""
        r, w, S, T = self._rows(rows, w)
        self._lib.check(self._lib.L.nnn_fit_loss_host(self._h, _ffi.ptr(r), _ffi.ptr(w), S, T))
        return self.losses()

    def grad(self, rows, w=None):
        """Forward pass, loss terms and the gradient into the object; returns losses()."""
        r, w, S, T = self._rows(rows, w)
        self._lib.check(self._lib.L.nnn_fit_grad_host(self._h, _ffi.ptr(r), _ffi.ptr(w), S, T))
        return self.losses()

    def step(self, hip_stream=0):
        """One Adam step from the held gradient, then the clip."""
        self._lib.check(self._lib.L.nnn_fit_step(self._h, hip_stream))

    def losses(self):
        """{total, gain (10 mean(w Lg)), vad (0.5 mean(w Lv)), reg, msse} of the last loss or grad call (waits for it)."""
        out = (C.c_float * 5)()
        self._lib.check(self._lib.L.nnn_fit_losses(self._h, out))
        return dict(zip(LOSS_NAMES, (float(x) for x in out)))

    # ---- calls on raw device pointers (asynchronous) ----
    @staticmethod
    def _rows_device(d_rows, n_seq, window, frame_stride, seq_stride, d_w, w_frame_stride, w_seq_stride):
        fs = n_seq * ROW_WIDTH if frame_stride is None else frame_stride
        ss = ROW_WIDTH if seq_stride is None else seq_stride
        wfs = n_seq if w_frame_stride is None else w_frame_stride
        wss = 1 if w_seq_stride is None else w_seq_stride
        return _ffi.FitRows(d_rows, fs, ss, d_w, wfs, wss, n_seq, window)

    def forward_device(self, d_rows, n_seq, window, d_gains, d_vad, frame_stride=None, seq_stride=None, hip_stream=0):
        """Strides in floats; the defaults are the generator's [window][n_seq][87]."""
        r = self._rows_device(d_rows, n_seq, window, frame_stride, seq_stride, None, None, None)
        self._lib.check(self._lib.L.nnn_fit_forward_device(self._h, C.byref(r), d_gains, d_vad, hip_stream))

    def loss_device(self, d_rows, n_seq, window, d_w=None, frame_stride=None, seq_stride=None, w_frame_stride=None, w_seq_stride=None, hip_stream=0):
        r = self._rows_device(d_rows, n_seq, window, frame_stride, seq_stride, d_w, w_frame_stride, w_seq_stride)
        self._lib.check(self._lib.L.nnn_fit_loss_device(self._h, C.byref(r), hip_stream))

    def grad_device(self, d_rows, n_seq, window, d_w=None, frame_stride=None, seq_stride=None, w_frame_stride=None, w_seq_stride=None, hip_stream=0):
        r = self._rows_device(d_rows, n_seq, window, frame_stride, seq_stride, d_w, w_frame_stride, w_seq_stride)
        self._lib.check(self._lib.L.nnn_fit_grad_device(self._h, C.byref(r), hip_stream))

    def debug_recurrence(self, layer, backward, n_seq, window, reps, hip_stream=0):
        """Measuring hook: one GRU's recurrence kernel alone."""
        self._lib.check(self._lib.L.nnn_fit_debug_recurrence(self._h, layer, int(backward), n_seq, window, reps, hip_stream))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.L.nnn_fit_destroy(self._h)
            self._h = None

    __del__ = close


# ---- policies: plain Python, no device ----------------------------------------------------------------------------------------------------
def glorot_params(rng, clip=CLIP):
    """Keras' default kernel initialiser for every matrix: uniform in +-sqrt(6 / (fan_in + fan_out)) of the matrix as stored (a GRU's is
    [inputs, 3 n]), capped at the clip; zero biases.  (Keras starts a GRU's recurrent matrix orthogonal; here it is Glorot like the
    others: a start, not a contract.)  float32 [87503]."""
    p = np.zeros(PARAMS, np.float32)
    for name, (off, shape) in TENSORS.items():
        if len(shape) == 2:
            limit = np.sqrt(6.0 / (shape[0] + shape[1]))
            v = rng.uniform(-limit, limit, size=shape)
            p[off:off + v.size] = np.clip(v, -clip, clip).astype(np.float32).reshape(-1)
    return p


def row_weights(rows):
    """train/rnn_train.py:111-117: a row's class is the mean of its targets that are not -1 -- below 1/3, above 2/3 or between -- and
    every class gets the same total weight, a third of the number of rows.  A row without a target weighs 0 (in the reference its mean
    is NaN, which belongs to no class).  One deliberate deviation: a class without a member contributes nothing, where the reference
    divides by zero and turns every weight into NaN.  rows [..., 87] -> float32 [...]."""
    y = np.asarray(rows)[..., NB_FEATURES:NB_FEATURES + NB_BANDS].astype(np.float64)
    have = y != -1
    n = have.sum(axis=-1)
    mean = np.where(n > 0, (y * have).sum(axis=-1) / np.maximum(n, 1), np.nan)
    hi, lo = mean > 2 / 3, mean < 1 / 3
    med = (mean >= 1 / 3) & (mean <= 2 / 3)
    total = mean.size
    w = np.zeros(mean.shape, np.float64)
    for cls in (hi, med, lo):
        if cls.any():
            w += cls * (total / cls.sum())
    return (w / 3).astype(np.float32)


def windows(rows, window):
    """[count, n_streams, 87] (the generator's output: consecutive rows of every stream) -> [n_streams * (count // window), window, 87]:
    each stream cut into windows of consecutive rows, stream by stream; the remainder of count / window is dropped."""
    r = np.asarray(rows)
    if r.ndim != 3 or r.shape[2] != ROW_WIDTH:
        raise ValueError(f"rows must have shape [count, n_streams, {ROW_WIDTH}]")
    count, S, _ = r.shape
    n = count // window
    return np.ascontiguousarray(r[:n * window].transpose(1, 0, 2).reshape(S * n, window, ROW_WIDTH))


def validation_split(n_sequences, validation):
    """Keras' validation_split: the LAST fraction of the sequences, before any shuffling.  Returns (n_train, n_validation)."""
    n_train = int(n_sequences * (1.0 - validation))
    return n_train, n_sequences - n_train


def batch_plan(n_train, batch, rng):
    """One epoch's batches: the training sequences in a new random order, `batch` at a time, the last one short."""
    order = rng.permutation(n_train)
    return [order[i:i + batch] for i in range(0, n_train, batch)]


def fit(trainer, rows, epochs=20, batch=32, window=2000, validation=0.1, seed=0, log=None):
    """train/rnn_train.py's model.fit on rows [count, n_streams, 87]: windows, sample weights, the last `validation` of the sequences
    held out, `epochs` passes over the shuffled rest in batches of `batch` sequences (one grad + step each).  Returns
    {"loss": [...], "val_loss": [...]}: per epoch the mean of `total` over the rows trained on and over the held-out rows (None
    without any)."""
    seqs = windows(rows, window)
    weights = row_weights(seqs)
    n_train, n_val = validation_split(len(seqs), validation)
    if n_train < 1:
        raise ValueError(f"{len(seqs)} windows of {window} rows leave nothing to train on")
    rng = np.random.default_rng(seed)
    history = {"loss": [], "val_loss": []}

    def batch_arrays(idx):   # [n, window, ...] -> the trainer's [window, n, ...]
        return np.ascontiguousarray(seqs[idx].transpose(1, 0, 2)), np.ascontiguousarray(weights[idx].T)

    for epoch in range(epochs):
        acc = 0.0
        for idx in batch_plan(n_train, batch, rng):
            r, w = batch_arrays(idx)
            acc += trainer.grad(r, w)["total"] * len(idx)
            trainer.step()
        history["loss"].append(acc / n_train)
        val = None
        if n_val:
            acc = 0.0
            for i in range(n_train, len(seqs), batch):
                idx = np.arange(i, min(i + batch, len(seqs)))
                r, w = batch_arrays(idx)
                acc += trainer.loss(r, w)["total"] * len(idx)
            val = acc / n_val
        history["val_loss"].append(val)
        if log:
            log(f"epoch {epoch + 1}/{epochs}: loss {history['loss'][-1]:.6g}" + ("" if val is None else f", val_loss {val:.6g}"))
    return history


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m nnnoiseless_amd.fit", description="Train a .rnn model from training rows (train/rnn_train.py and dump_rnn.py).")
    ap.add_argument("rows", help=".npy of float32 [count, n_streams, 87] as `python -m nnnoiseless_amd.training` writes it")
    ap.add_argument("-o", "--output", required=True, help="the .rnn file to write")
    ap.add_argument("--template", help="a .rnn file to fine-tune from (default: Glorot start, the reference's activations)")
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--window", type=int, default=2000)
    ap.add_argument("--validation", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    rows = np.load(a.rows, mmap_mode="r")
    if rows.ndim == 2:   # the reference's flat [count, 87]: one stream
        rows = rows[:, None, :]
    template = open(a.template, "rb").read() if a.template else None
    trainer = Trainer(template, max_seq=a.batch, max_window=a.window, device=a.device)
    if template is None:
        trainer.set_params(glorot_params(np.random.default_rng(a.seed)))
    fit(trainer, rows, epochs=a.epochs, batch=a.batch, window=a.window, validation=a.validation, seed=a.seed, log=print)
    with open(a.output, "wb") as f:
        f.write(trainer.export_rnn())
    trainer.close()


if __name__ == "__main__":
    main()
