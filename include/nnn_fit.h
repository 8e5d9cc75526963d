// SPDX-License-Identifier: BSD-3-Clause
/*
 * nnn_fit.h -- the network trainer of the reference's train/rnn_train.py on the device.
 *
 * nnn_sim.h and nnn_train.h turn raw PCM into 87-column training rows; this object turns rows into a model: forward pass, loss,
 * back-propagation through time and Adam over windows of consecutive rows, and the quantisation of train/dump_rnn.py into a .rnn file.
 *
 * The network has the reference's shape and no other: dense 42->24, GRU 24->24 (vad), GRU 90->48 (noise), GRU 114->96 (denoise),
 * dense 96->22 (gains), dense 24->1 (vad).  In training the activations are the true tanh / sigmoid / ReLU in f32 -- not the
 * inference path's tables and not its 1/256 scale.  Per GRU, with h = 0 at the first row of every window (Keras stateful=False):
 *     z  = sigmoid(x Wz + h Uz + bz)
 *     r  = sigmoid(x Wr + h Ur + br)
 *     c  = act(x Wc + (r * h) Uc + bc)
 *     h' = z * h + (1 - z) * c
 * noise GRU input = [dense | vad | features], denoise GRU input = [vad | noise | features] (src/rnn.rs:343-379).
 *
 * The loss (the contract; DESIGN.md section 22 has the reasons).  Per row: x = columns 0..41, y = columns 42..63 (-1: no target),
 * v = column 86, w = the row's weight (no weights: 1); g the 22 gain outputs, p the VAD output:
 *     lo = float32(1e-7), hi = float32(1) - float32(1e-7)
 *     yc = clamp(y, lo, hi), vc = clamp(v, lo, hi)
 *     c(a, o) = -(a log(o) + (1 - a) log(1 - o))          -- the PREDICTION is `a`: the reference passes it as the target
 *     m_b = min(y_b + 1, 1), e_b = sqrt(g_b) - sqrt(max(y_b, 0))
 *     Lg = 1/22 sum_b m_b (10 e_b^4 + e_b^2 + 0.01 c(g_b, yc_b)),  Lv = 2 |v - 0.5| c(p, vc),  msse = 1/22 sum_b m_b e_b^2
 *     total = 10 mean(w Lg) + 0.5 mean(w Lv) + reg sum(W^2, U^2 of the three GRUs)
 * mean: the plain mean over the n_seq x window rows of the call.
 *
 * Plain C ABI; all functions return 0 on success (nnn_last_error() of nnn_batch.h has the text); no CPU fallback.  Calls with a
 * stream are asynchronous on it.  The same call on the same data gives the same bits every time: no floating-point atomics, every sum
 * in a fixed order that depends on n_seq and window alone (not on max_seq, max_window or earlier calls).
 */
#ifndef NNN_FIT_H
#define NNN_FIT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nnn_fit nnn_fit;

#define NNN_FIT_PARAMS 87503      /* f32 values: the .rnn file without its 18 header bytes, in file order */
#define NNN_FIT_RNN_BYTES 87521
#define NNN_FIT_ROW 87            /* columns of a training row */
#define NNN_FIT_TILE 4            /* sequences one recurrence block owns */
#define NNN_FIT_ROW_BYTES 5752    /* saved activations and deltas per row: the object allocates max_seq x max_window of them
                                     (about 370 MB at 32 x 2000, 2.9 GB at 256 x 2000) */

/*
 * The fifteen tensors of the parameter vector.  A dense layer is W[in][n] then b[n]; a GRU is W[in][3n], U[n][3n], b[3n], columns
 * z | r | candidate.
 */
#define NNN_FIT_OFF_IN_W 0         /* input dense     [42][24] */
#define NNN_FIT_OFF_IN_B 1008      /*                 [24]     */
#define NNN_FIT_OFF_VAD_W 1032     /* vad GRU         [24][72] */
#define NNN_FIT_OFF_VAD_U 2760     /*                 [24][72] */
#define NNN_FIT_OFF_VAD_B 4488     /*                 [72]     */
#define NNN_FIT_OFF_NOISE_W 4560   /* noise GRU       [90][144] */
#define NNN_FIT_OFF_NOISE_U 17520  /*                 [48][144] */
#define NNN_FIT_OFF_NOISE_B 24432  /*                 [144]    */
#define NNN_FIT_OFF_DN_W 24576     /* denoise GRU     [114][288] */
#define NNN_FIT_OFF_DN_U 57408     /*                 [96][288] */
#define NNN_FIT_OFF_DN_B 85056     /*                 [288]    */
#define NNN_FIT_OFF_OUT_W 85344    /* denoise output  [96][22] */
#define NNN_FIT_OFF_OUT_B 87456    /*                 [22]     */
#define NNN_FIT_OFF_VOUT_W 87478   /* vad output      [24][1]  */
#define NNN_FIT_OFF_VOUT_B 87502   /*                 [1]      */

/* selectors of nnn_fit_get / nnn_fit_set */
#define NNN_FIT_SEL_PARAMS 0
#define NNN_FIT_SEL_GRAD 1         /* get only */
#define NNN_FIT_SEL_ADAM_M 2
#define NNN_FIT_SEL_ADAM_V 3

/* Adam as Keras runs it, the L2 factor of the GRU matrices and the clip of every parameter (train/rnn_train.py:61-62). */
typedef struct nnn_fit_settings {
    float lr, beta1, beta2, epsilon;   /* 1e-3, 0.9, 0.999, 1e-7 */
    float reg;                         /* 1e-6 */
    float clip;                        /* 0.499 */
} nnn_fit_settings;

/* The rows of one call.  Element `col` of row (t, s) is rows[t * frame_stride + s * seq_stride + col] (strides in floats): the
 * generator's [T][S][87] is frame_stride = n_seq * 87, seq_stride = 87; the reference's [S][T][87] is frame_stride = 87, seq_stride =
 * window * 87.  w: NULL (every row weighs 1) or weights[t * w_frame_stride + s * w_seq_stride]. */
typedef struct nnn_fit_rows {
    const float *rows;
    size_t frame_stride, seq_stride;
    const float *w;
    size_t w_frame_stride, w_seq_stride;
    int n_seq, window;                 /* 1 <= n_seq <= max_seq, 1 <= window <= max_window */
} nnn_fit_rows;

/*
 * rnn_bytes: a .rnn file as template -- it fixes the four hidden activations (each tanh, sigmoid or ReLU) and its weights / 256 are
 * the starting parameters.  Another layer size than the reference's, or an output layer that is not sigmoid (the loss takes the
 * square root of the output), is refused.  NULL: the reference's training set-up (tanh, tanh, ReLU, tanh) with zero parameters, to
 * be overwritten by nnn_fit_set.  Adam's moments and the step count start at zero.
 */
nnn_fit *nnn_fit_create(const uint8_t *rnn_bytes, size_t len, int max_seq, int max_window, int device);
void nnn_fit_destroy(nnn_fit *f);

/* NNN_FIT_PARAMS floats of host memory (synchronous).  set refuses non-finite values and the gradient selector. */
int nnn_fit_get(nnn_fit *f, int which, float *out);
int nnn_fit_set(nnn_fit *f, int which, const float *in);
/* Adam's step count t (the number of nnn_fit_step calls so far).  With the parameters and the two moments: the checkpoint. */
int nnn_fit_get_step(nnn_fit *f, int64_t *step);
int nnn_fit_set_step(nnn_fit *f, int64_t step);
int nnn_fit_get_settings(nnn_fit *f, nnn_fit_settings *s);
int nnn_fit_set_settings(nnn_fit *f, const nnn_fit_settings *s);

/* The 87 521-byte .rnn file: the template's headers and every parameter as clamp(rint(256 x), -128, 127), rint to even
 * (train/dump_rnn.py:9-13).  cap < NNN_FIT_RNN_BYTES or a non-finite parameter refuses. */
int nnn_fit_export_rnn(nnn_fit *f, uint8_t *out, size_t cap);

/* Forward pass alone: gains [window][n_seq][22] and vad [window][n_seq] (device memory; r->w is ignored). */
int nnn_fit_forward_device(nnn_fit *f, const nnn_fit_rows *r, float *d_gains, float *d_vad, void *hip_stream);
/* Forward pass and the loss terms (validation batches). */
int nnn_fit_loss_device(nnn_fit *f, const nnn_fit_rows *r, void *hip_stream);
/* Forward pass, loss terms and the gradient of `total` into the object (NNN_FIT_SEL_GRAD). */
int nnn_fit_grad_device(nnn_fit *f, const nnn_fit_rows *r, void *hip_stream);
/* One optimiser step from the held gradient; refused before the first nnn_fit_grad_*.  lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t) in
 * f64 on the host; per element in f32, one IEEE operation per statement (k_fit_adam):
 *     m = beta1 m + (1 - beta1) grad;  v = beta2 v + (1 - beta2) grad^2;  p = p - lr_t m / (sqrt(v) + epsilon);  p = min(max(p, -clip), clip) */
int nnn_fit_step(nnn_fit *f, void *hip_stream);
/* Waits for the last loss or grad call: {total, 10 mean(w Lg), 0.5 mean(w Lv), reg term, mean(w msse)}. */
int nnn_fit_losses(nnn_fit *f, float out[5]);

/* The same with host memory, synchronous: rows dense [window][n_seq][87], w NULL or [window][n_seq]. */
int nnn_fit_forward_host(nnn_fit *f, const float *rows, int n_seq, int window, float *gains, float *vad);
int nnn_fit_loss_host(nnn_fit *f, const float *rows, const float *w, int n_seq, int window);
int nnn_fit_grad_host(nnn_fit *f, const float *rows, const float *w, int n_seq, int window);

/* Measuring hook: the recurrence kernel of GRU `layer` (0 vad, 1 noise, 2 denoise) alone, forward or backward, `reps` launches over
 * whatever the object's buffers hold.  The gradient and the loss terms are not touched; the saved activations are. */
int nnn_fit_debug_recurrence(nnn_fit *f, int layer, int backward, int n_seq, int window, int reps, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* NNN_FIT_H */
