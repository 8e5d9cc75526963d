// SPDX-License-Identifier: BSD-3-Clause
/*
 * nnn_sim.h -- the noise simulator of the reference's training-data generator on the device.
 *
 * nnn_train.h is the per-frame body of the generator (src/training.rs:113-160).  This is what feeds it: n_streams
 * independent NoiseSimulator instances (src/training.rs:263-422) over two int16 arenas resident in device memory, one
 * of clean speech and one of noise, each a concatenation of 48 kHz mono 16-bit clips.  A call names, for every
 * (frame, triple), the element of each arena where that frame's 480 samples begin; one kernel (k_sim) turns them
 * into the three signals and the two labels, statement for statement as NoiseSimulator::next_frame does:
 *     n[i] = (float)noise16[i] * noise_gain                                                   (:322-328)
 *     x[i] = (float)sig16[i];  energy += x[i] * x[i] (f32, in sample order);  x[i] *= signal_gain   (:331-339)
 *     sig_filter.filter_in_place(x, signal_resp_mem);  noise_filter.filter_in_place(n, noise_resp_mem)
 *                                                 (src/util.rs:114-126: f64 arithmetic, both memories rounded to f32 every step)
 *     combined[i] = x[i] + n[i]                                                               (:402-404)
 *     vad_count: = 0 above 1e9, -5 above 1e8, +1 above 1e7, else +2; clamped to [0, 15];
 *     vad = 0.0 for vad_count >= 10, 0.5 for vad_count > 0, else 1.0                          (:368-386)
 *     band_gain_cutoff = (vad == 0 && noise_gain == 0) ? 0 : band_lp + 1                      (:409-413)
 * and the training-row path of nnn_train.h runs over them: only the offsets go in and only the rows come out.
 * The random policy (randomize, random_filter) and the file-reading policy (SignalReader) are host arithmetic: they
 * arrive as parameters and offsets (nnnoiseless_amd/training.py has both).
 *
 * Plain C ABI; all functions return 0 on success (nnn_last_error() of nnn_batch.h has the text); no CPU fallback.
 */
#ifndef NNN_SIM_H
#define NNN_SIM_H

#include <stddef.h>
#include <stdint.h>

#include "nnn_train.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nnn_sim nnn_sim;

#define NNN_SIM_ARENA_SIGNAL 0
#define NNN_SIM_ARENA_NOISE 1

/* One triple's parameters (44 bytes).  NoiseSimulator::new: gains 1, every coefficient 0, band_lp 21. */
typedef struct nnn_sim_params {
    float signal_gain, noise_gain;
    float sig_a[2], sig_b[2];     /* sig_filter: Biquad { a, b } (src/util.rs:81-86) */
    float noise_a[2], noise_b[2]; /* noise_filter */
    int32_t band_lp;              /* 0 .. 21 */
} nnn_sim_params;

/*
 * n_streams = that of `t`, which the simulator borrows: t must outlive it.  Allocates the staging of one frame
 * group of t on t's device: three f32 rows of max_group_frames x 480 per triple plus a cutoff and a VAD row, i.e.
 * 3 x 1920 B x group frames per triple -- about 2.3 GB at 16 384 triples x 24 frames.
 */
nnn_sim *nnn_sim_create(nnn_train *t);
void nnn_sim_destroy(nnn_sim *sim);

/* Arenas.  which: NNN_SIM_ARENA_SIGNAL or NNN_SIM_ARENA_NOISE.  load uploads a copy the simulator owns (synchronous;
 * may be repeated: the previous arena is released once the calls that read it are done); adopt_device borrows a
 * device buffer of the caller's (2-byte aligned; it must stay valid until replaced or the simulator is destroyed). */
int nnn_sim_load(nnn_sim *sim, int which, const int16_t *pcm, uint64_t elems);
int nnn_sim_adopt_device(nnn_sim *sim, int which, const int16_t *d_pcm, uint64_t elems);

/* Parameters of the listed triples (streams == NULL: triples 0 .. n - 1).  Configuration: a change takes effect from
 * the next call's first frame.  A record with a non-finite value or a band_lp outside [0, 21], or a stream index
 * out of range, refuses the whole call and nothing changes. */
int nnn_sim_set_params(nnn_sim *sim, const int *streams, int n, const nnn_sim_params *recs);
int nnn_sim_get_params(nnn_sim *sim, const int *streams, int n, nnn_sim_params *recs);

/* Zeroes the filter memories and the VAD counters; parameters and arenas stay.  Leaves `t` alone: pair it with
 * nnn_train_reset. */
int nnn_sim_reset(nnn_sim *sim);

/*
 * n_frames rows per triple.  d_sig_off / d_noise_off [f * n_streams + s]: the element of the arena where frame f of
 * triple s begins; any value with off + 480 <= elems, odd ones and frames shared between triples included.
 * d_rows [(f * n_streams + s) * 87 ...] as nnn_train_process_device writes them.  Any n_frames > 0; runs group by
 * group (k_sim into the staging, then nnn_train_process_device over it).  Asynchronous; hip_stream: a hipStream_t
 * (NULL = the training object's own stream).
 * A frame whose offset leaves its arena reads as 480 zeros -- nothing out of range is touched -- and sets the flag
 * nnn_sim_fault returns.
 */
int nnn_sim_process_device(nnn_sim *sim, const uint64_t *d_sig_off, const uint64_t *d_noise_off, float *d_rows, int n_frames,
                           void *hip_stream);
/* Same with host buffers, synchronous.  Every offset is checked first: one that leaves its arena refuses the whole
 * call before anything is enqueued. */
int nnn_sim_process_host(nnn_sim *sim, const uint64_t *sig_off, const uint64_t *noise_off, float *rows, int n_frames);

/*
 * The three signals and the two labels without the rows, in the layout nnn_train_process_* takes:
 *   sample i of frame f of triple s: d_signal / d_noise / d_combined [s * stream_stride + f * frame_stride + i]
 *   d_cutoff / d_vad [f * n_streams + s]
 * Bases and strides must be multiples of 16 bytes (strides are in floats: multiples of 4).  Advances the simulator's
 * state exactly as process does and leaves the feature states of `t` alone.  The host variant is dense
 * [n_streams][n_frames][480] and checks the offsets like nnn_sim_process_host.
 */
int nnn_sim_signals_device(nnn_sim *sim, const uint64_t *d_sig_off, const uint64_t *d_noise_off, float *d_signal, float *d_noise,
                           float *d_combined, int32_t *d_cutoff, float *d_vad, int n_frames, size_t stream_stride, size_t frame_stride,
                           void *hip_stream);
int nnn_sim_signals_host(nnn_sim *sim, const uint64_t *sig_off, const uint64_t *noise_off, float *signal, float *noise, float *combined,
                         int32_t *cutoff, float *vad, int n_frames);

/* 1 once a device entry point met a frame whose offset leaves its arena (sticky; waits for the calls enqueued so
 * far), 0 if none did, negative on error. */
int nnn_sim_fault(nnn_sim *sim);

/* Measuring hook: k_sim alone, `reps` launches of n_frames (<= max_group_frames) frames into the staging.  The
 * simulator's state advances; nothing else is written. */
int nnn_sim_debug_kernel(nnn_sim *sim, const uint64_t *d_sig_off, const uint64_t *d_noise_off, int n_frames, int reps, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* NNN_SIM_H */
