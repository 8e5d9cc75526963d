/* SPDX-License-Identifier: BSD-3-Clause */
/*
 * nnn_rate.h -- rate adapter: streams at another sample rate in and out of a 48 kHz batch.
 *
 * The reference CLI resamples any input that is not at 48 kHz before denoising it (src/nnnoiseless.rs:179-227): `Resample<RS>` around
 * dasp_interpolate 0.11's `Sinc<[f32; 16]>`, ratio = source_rate / 48000 (include/nnn_resample.h has the loop).  An adapter is that loop
 * in front of a batch, the batch's ordinary processing call over the whole frames the resampled samples make, and THE SAME loop run at the
 * inverse ratio, 48000 / source_rate, behind it, in one asynchronous call: source-rate samples in, source-rate samples out.
 *   - Up-leg: position sequence, credit and idx exactly as nnn_resampler_process_device has them; the 48 kHz samples go behind the
 *     partial frame the adapter carries from call to call, in device memory of its own.
 *   - The T whole frames now present (T may be 0) go through nnn_batch_process_device; what lies behind frame T is carried.
 *   - Down-leg: the T * 480 denoised samples through the same interpolator with a history, position and credit of its own.
 * The return leg is the reference CLI's interpolator run at the inverse ratio and invents nothing else: like the up-leg it is restated
 * from the published source of dasp_interpolate 0.11.0 and pinned by no reference test; it has NO anti-alias filter of its own (the
 * 16-tap Hann-windowed sinc is all there is), and at integer ratios (8, 12, 16, 24 kHz) its position is always 0, so it picks the
 * denoised sample at each source instant.
 * Any chunking of the input gives the same bits as one call.  All streams of the batch share one source rate (another rate: another
 * batch), mono, stream-major rows; the position is shared by all streams.
 *
 * Plain C ABI; 0 on success (nnn_last_error() of nnn_batch.h has the text); no CPU fallback.
 */
#ifndef NNN_RATE_H
#define NNN_RATE_H

#include <stddef.h>

#include "nnn_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nnn_rate nnn_rate;

/* Borrows b (b must outlive the adapter).  max_in = the largest n_in a call may pass: it sizes the device staging (whole frames of
 * 48 kHz samples per stream), the schedule tables and the page-locked memory they are uploaded from, all allocated here.
 * Refused (NULL): a NULL batch, source_rate <= 0 or == 48000 (use the batch), a rate so far from 48 kHz that 64 outputs of a leg span
 * more source samples than a workgroup's LDS holds (below 1 kHz or above 2.4 MHz), max_in < 1 or so large that a call's sample
 * counts leave 32 bits. */
nnn_rate *nnn_rate_create(nnn_batch *b, double source_rate, long max_in);
void nnn_rate_destroy(nnn_rate *a);
/* The adapter alone back to its fresh state: positions, histories, the carried partial frame.  The batch is not touched, and the
 * resident schedule tables stay (they are pure functions of their key). */
int nnn_rate_reset(nnn_rate *a);
/*
 * Per-stream reset and hold.  The position is shared, so a stream cannot keep a phase of its own; what a stream owns is its two 16-sample
 * histories and its carried partial-frame samples.  nnn_rate_reset_streams clears those for the listed streams (host memory; an index
 * outside [0, n_streams) is refused, repeats are harmless): from the next call on each listed stream's output is what it would have
 * been had all its earlier source samples been zero.  It takes effect at the head of the next processing call, in order with it.  The
 * caller resets the batch's slot with nnn_batch_reset_streams as before.
 * A stream the BATCH holds (nnn_batch_hold_streams) sits an adapter call out: its source row is not read, its output and VAD rows are
 * not written, and its adapter state is cleared as by nnn_rate_reset_streams -- a resumed call restarts its resampler legs from silence
 * while its denoiser state continues bit for bit.  The mask goes to the device only while the batch holds a stream or a reset is
 * waiting; otherwise the kernels run in the instantiations that have no mask.
 */
int nnn_rate_reset_streams(nnn_rate *a, const int *streams, int n);
/* Bounds for a call of n_in samples per stream, whatever the adapter's state: source-rate samples it can return, frames (VAD rows) it
 * can complete. */
long nnn_rate_max_output(const nnn_rate *a, long n_in);
int nnn_rate_max_frames(const nnn_rate *a, long n_in);
/* 48 kHz samples of the partial frame now held (0..479). */
long nnn_rate_carried(const nnn_rate *a);
/*
 * Feed n_in source samples per stream, d_in[s * in_stride + i], and collect what they complete:
 *   d_out[s * out_stride + m], m < *n_out      source-rate samples, the same count for every stream
 *   d_vad[t * n_streams + s], t < *n_frames    the VAD of the frames the call completed (NULL to skip)
 * format: NNN_PCM_F32 (floats in i16 range) or NNN_PCM_I16 (packed int16 in; out = round-half-away(clamp(x, -32768, 32767)) as the
 * CLI's writers do) for d_in and d_out alike; strides in elements of the format.  Other formats and interleaved channels are refused.
 * *n_out and *n_frames are known on return (the schedule is host arithmetic); the device work is asynchronous on hip_stream, NULL = the
 * batch's own stream, as in nnn_batch_process_device.  The call does not synchronise: schedule tables go up from page-locked memory of
 * the adapter's, and a table whose key -- the bits of the position, idx, credit, n_in -- was seen in one of the last few calls is
 * reused where it lies on the device, with no trigonometry and no upload (at 10 ms ticks of 16 kHz: every call from the third on;
 * at 44.1 kHz the position drifts in its last bits and every call builds its tables).
 * Refused, consuming nothing and changing nothing: cap_out below nnn_rate_max_output(a, n_in); cap_frames below
 * nnn_rate_max_frames(a, n_in); n_in above max_in or below 0; a NULL d_out, or a NULL d_in with n_in > 0; another format; frames
 * pending from an nnn_batch_analyze_*; a set nnn_batch_fault; a batch under nnn_batch_set_inputs_ready(b, 1) (the frames the batch
 * reads are produced on the call's stream by the call itself).
 */
int nnn_rate_process_device(nnn_rate *a, const void *d_in, long n_in, size_t in_stride, void *d_out, long cap_out, size_t out_stride,
                            long *n_out, float *d_vad, int cap_frames, int *n_frames, int format, void *hip_stream);
/* The same with dense host rows, in[s * n_in + i] -> out[s * cap_out + m], vad[t * n_streams + s]; synchronous.  With streams held
 * the caller's out and vad rows make the round trip, so that held rows come back as they were. */
int nnn_rate_process_host(nnn_rate *a, const void *in, long n_in, void *out, long cap_out, long *n_out, float *vad, int cap_frames,
                          int *n_frames, int format);
/* Test hook: schedule tables built so far (a call that finds its key resident builds none) and the host microseconds spent building
 * them; [0] the up-leg, [1] the down-leg.  Either pointer may be NULL. */
int nnn_rate_debug_tables(const nnn_rate *a, long tables[2], double host_us[2]);

#ifdef __cplusplus
}
#endif
#endif /* NNN_RATE_H */
