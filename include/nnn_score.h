// SPDX-License-Identifier: BSD-3-Clause
/*
 * nnn_score.h -- the scorer: per-stream sums between a reference signal and a test signal, carried across calls
 * on the device, from which SNR, SI-SDR and segmental SNR are host arithmetic (nnnoiseless_amd/score.py has the formulas).
 *
 * An object holds, for each of its n_streams streams: a delay in samples (0 <= delay <= max_delay, configuration, 0 at creation), the
 * last max_delay reference samples (the history: zeros at creation and after a reset), four f64 totals and a u64 count of the frames
 * that were counted.  With r[n] the stream's reference samples since its last reset (zeros before them) and y[n] its test samples,
 * a frame of 480 samples n = n0 .. n0 + 479 yields
 *     A = sum r[n - delay]^2    B = sum y[n]^2    C = sum r[n - delay] y[n]    E = sum (r[n - delay] - y[n])^2
 * and the stream's totals are its frames' sums added in frame order, each total starting at +0.0.
 *
 * THE ARITHMETIC (the contract: a restatement that follows it gives the same bits; tests/score_cases.py is one).  Per sample i of the
 * frame (0 <= i < 480), with rd = (double)r[n0 + i - delay] and yd = (double)y[n0 + i], every operation one IEEE binary64 operation,
 * round to nearest even, nothing contracted into a fused multiply-add:
 *     a_i = rd * rd     b_i = yd * yd     c_i = rd * yd     d = rd - yd,  e_i = d * d
 * (the three products of two f32 values are exact; d and e_i round once each).  The 480 terms of a sum are added in this order:
 *   1. 64 partial sums p_0 .. p_63.  p_L starts at +0.0 and takes the terms i = L, L + 64, L + 128, ... below 480 in ascending order:
 *          p_L = ((((0.0 + t_L) + t_(L+64)) + t_(L+128)) + ...)          -- eight terms for L < 32, seven for L >= 32
 *   2. six pairwise steps over the partial sums, for m = 32, 16, 8, 4, 2, 1 in this order:
 *          p_L <- p_L + p_(L xor m)      for all 64 L at once
 *      the frame's sum is p_0 after the sixth step:
 *          ((((p_0 + p_32) + (p_16 + p_48)) + ((p_8 + p_40) + (p_24 + p_56))) + ...) + ...
 * The order depends on the sample's index in the frame and on nothing else: not on n_streams, n_frames, the delay, the addresses or
 * their alignment.  So any cut of a stream's frames into calls gives the same bits, and so does any layout of them in memory.
 * Non-finite samples propagate as IEEE 754 says (inf - inf and 0 x inf are NaN); nothing is clamped or flagged.  Which NaN (sign and
 * payload) comes out is not part of the contract.  The device takes no logarithm.
 *
 * Plain C ABI; all functions return 0 on success (nnn_last_error() of nnn_batch.h has the text); no CPU fallback.  Calls with a stream
 * are asynchronous on it; calls of one object made on different streams are ordered by the object.
 */
#ifndef NNN_SCORE_H
#define NNN_SCORE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nnn_score nnn_score;

#define NNN_SCORE_FRAME 480
#define NNN_SCORE_MAX_DELAY 960     /* the largest max_delay an object takes: two frames */
#define NNN_SCORE_SUMS 4            /* A, B, C, E in this order */

/* 1 <= n_streams, 0 <= max_delay <= NNN_SCORE_MAX_DELAY.  Device memory: 8 x max_delay + 45 bytes per stream, and
 * 32 bytes per stream-frame of the longest call that handed in no d_frame_sums. */
nnn_score *nnn_score_create(int n_streams, int max_delay, int device);
void nnn_score_destroy(nnn_score *h);

/* The delays of the listed streams (idx == NULL: streams 0 .. n - 1).  set also zeroes those streams' history, totals and count: sums
 * taken under two delays do not add up to anything.  A delay outside [0, max_delay] or an index outside the object refuses the whole
 * call and nothing changes.  Both wait for the calls enqueued so far. */
int nnn_score_set_delay(nnn_score *h, const int *idx, int n, const int32_t *delays);
int nnn_score_get_delay(nnn_score *h, const int *idx, int n, int32_t *delays);

/* Zeroes history, totals and count of the listed streams (idx == NULL: of every stream, n is ignored).  The delays stay. */
int nnn_score_reset(nnn_score *h, const int *idx, int n);

/*
 * n_frames >= 1 frames of every stream.  Sample i of frame f of stream s: d_ref / d_test [s * stream_stride + f * frame_stride + i]
 * (strides in floats, the addressing of nnn_train_process_device: the batch's [T][S][480] is stream_stride = 480, frame_stride =
 * n_streams * 480; per-stream-contiguous audio is stream_stride = n_frames * 480, frame_stride = 480).  f32 at any scale; 4-byte
 * alignment is all the bases need, and any strides do: there is one code path, and it fetches 64 consecutive floats an instruction.
 * d_valid: NULL (every frame counts) or uint8 [n_frames][n_streams]; a frame marked 0 adds nothing to totals or count and its row of
 *   d_frame_sums is zeros, but its reference samples enter the history like any other's: time passes for it.
 * d_frame_sums: NULL or double [n_frames][n_streams][4], the frames' own A, B, C, E.
 * Both signals must stay valid until the call has run.  hip_stream: a hipStream_t (NULL = the object's own stream).
 */
int nnn_score_accumulate_device(nnn_score *h, const float *d_ref, const float *d_test, const uint8_t *d_valid, double *d_frame_sums,
                                int n_frames, size_t stream_stride, size_t frame_stride, void *hip_stream);
/* The same with host memory, synchronous: ref / test dense [n_streams][n_frames][480], valid NULL or [n_frames][n_streams],
 * frame_sums NULL or [n_frames][n_streams][4]. */
int nnn_score_accumulate_host(nnn_score *h, const float *ref, const float *test, const uint8_t *valid, double *frame_sums, int n_frames);

/* Totals double [n_streams][4] and counts uint64 [n_streams] (either may be NULL).  The host call waits for the calls enqueued so far;
 * the device call is an asynchronous copy into the caller's device memory, ordered behind them. */
int nnn_score_totals(nnn_score *h, double *out, uint64_t *counts);
int nnn_score_totals_device(nnn_score *h, double *d_out, uint64_t *d_counts, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* NNN_SCORE_H */
