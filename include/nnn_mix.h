// SPDX-License-Identifier: BSD-3-Clause
/*
 * nnn_mix.h -- the conference mixer: the step a voice server puts behind the VAD gate.  Every stream belongs to a
 * room; each live member of a room receives the sum of the room's other talkers, its own voice left out (mix-minus), on the device: the
 * denoised audio, the gate's d_open rows (who is talking) and the batch's held mask (who is absent) are there already.
 *
 * An object beside the batch, like the scorer and the gate: it changes no call and no kernel of the batch.  There is no node mirror: a
 * node's host makes one mixer per shard, next to the shard's batch and gate, and rooms do not span shards.
 *
 * An object holds, for each of its n_streams streams,
 *   configuration   room   int32 in -1 .. n_streams - 1: a label; -1 = alone, the same as a room of one     -1 at creation
 *                   gain   f32 in [0, NNN_MIX_MAX_GAIN]; NaN is refused                                       1
 *   state           prev   f32: the stream's effective gain in its last live frame                           0, and 0 after nnn_mix_reset
 * The members of a room are its streams in ascending stream index.  That order is the summation order; it does not depend on the
 * labels, the grid or the layout.  A stereo participant is two streams in two rooms (one room per channel).
 *
 * THE RULE (the contract: a restatement that follows it gives the same bits; tests/mix_cases.py is one).  A stream's frames are numbered
 * n = 0, 1, ... over its live frames since its last reset.  x_n[i] are the stream's 480 samples of frame n after the format's loader
 * ((float) of an int16, unit floats times 32768.0f, plain floats as they are); talk_n is its d_talk entry, or 1 where d_talk is NULL.
 *   1. h_n = talk_n ? gain : 0.0f,   h_(-1) = prev
 *   2. the gain    g_i = h_n                                       if h_(n-1) == h_n
 *                  g_i = h_(n-1) + (h_n - h_(n-1)) * RAMP[i]       otherwise, RAMP[i] = (float)(i + 1) / 480.0f
 *      every operation one IEEE binary32 operation, round to nearest even, nothing contracted into a fused multiply-add (step 6 of
 *      nnn_gate.h verbatim): mute, unmute and set_gains are click-free one-frame ramps
 *   3. the stream-frame is AUDIBLE iff h_(n-1) != 0 || h_n != 0.  The input of an inaudible stream-frame is not read: whatever bytes
 *      lie there, NaN included, cannot matter.
 *   4. the term    c[i] = (double)x_n[i] * (double)g_i             exact in binary64 (24 x 24 bits); +0.0 for an inaudible stream-frame
 *   5. the room's total  T[i] = (...((+0.0 + c_a) + c_b) + ...)    over the room's live audible members in ascending stream index,
 *      binary64, round to nearest even
 *   6. the output of every live member p, with A the number of live audible members of its room in this frame:
 *        p audible and A == 1:   y_p[i] = +0.0f                    (nobody else is audible; T - c_p is that for every finite sample)
 *        p audible and A == 2:   y_p[i] = (float)c_q[i]            q the other audible member: a two-party call hands each side the
 *                                                                  other's samples with one rounding, bit for bit at gain 1
 *        otherwise:              y_p[i] = (float)(T[i] - c_p[i])   (for an inaudible p that is (float)T[i])
 *      stored through the output format's writer: int16 rounds half away from zero and clamps, unit floats are / 32768.0f and clamped
 *      to [-1, 1], plain floats as they are
 *   7. heard_p = the number of live audible members of the room other than p (optional output): a DTX or "nobody is talking to you" flag
 *   8. after the call  prev = h_(the call's last frame)  for every live stream
 * A stream marked 0 in d_live sits the call out: for that call it is not a member of its room; its input, d_talk entries, output and
 * d_heard entries are neither read nor written and its prev does not move.  This is how the streams a batch holds pass (live = !held).
 *
 * What follows from the rule:
 *   - a lone audible talker receives +0.0; so does every member of a room in which nobody is audible, and a room of one reads nothing
 *   - with one steady audible talker at gain 1 every other member receives that talker's bits (-0.0 becomes +0.0; which NaN a NaN
 *     becomes is not part of the contract)
 *   - for integer-valued (int16) samples and steady gain 1 every sum is exact: the output is the correctly rounded integer sum of the
 *     others, whatever the order
 *   - in general T - c_p is within about A * 2^-52 * sum|c| of the exact sum of the others, before the one rounding to binary32; the
 *     restatement is the bit contract, not this bound
 *   - a non-finite audible sample makes that sample non-finite for the other members of its room
 *   - the output depends on the frame's number, the parameters and the masks alone: not on how the frames are cut into calls, on
 *     layout, alignment, room labels or n_streams
 *
 * Plain C ABI; all functions return 0 on success (nnn_last_error() of nnn_batch.h has the text); no CPU fallback.  Everything is
 * checked before anything changes: a refused call leaves the object as it was.  Calls with a stream are asynchronous on it; calls of one
 * object made on different streams are ordered by the object.
 */
#ifndef NNN_MIX_H
#define NNN_MIX_H

#include <stddef.h>
#include <stdint.h>

#include "nnn_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nnn_mix nnn_mix;

#define NNN_MIX_FRAME 480
#define NNN_MIX_MAX_GAIN 16
/* tuning, not contract: no output bit depends on either */
#define NNN_MIX_TILE 32          /* listeners a block of the sum kernel serves: a room's members are cut into runs of at most this many */
#define NNN_MIX_REG_TALKERS 8    /* audible terms of a room-frame the sum kernel keeps in registers; the terms beyond are recomputed */

/* 1 <= n_streams.  Every stream alone (room -1), gain 1, prev 0.  Device memory: about 30 bytes per stream. */
nnn_mix *nnn_mix_create(int n_streams, int device);
void nnn_mix_destroy(nnn_mix *m);

/* The rooms and gains of the listed streams (idx == NULL: streams 0 .. n - 1).  A value out of range or NaN, an index outside the
 * object or one listed twice refuses the whole call.  The setters wait for the calls enqueued so far, rebuild the member tables on the
 * host (page-locked) and upload them; a changed value is in force from the next call's first frame.  A changed gain reaches the audio
 * through the one-frame ramp of step 2.  set_rooms does not touch prev: a stream moved while audible clicks in the room it leaves (its
 * ramp down is never mixed there) and fades in nowhere -- the host mutes it (gain 0 or talk 0 for one frame) first.  The getters read
 * the host's copy and wait for nothing. */
int nnn_mix_set_rooms(nnn_mix *m, const int *idx, int n, const int32_t *room);
int nnn_mix_get_rooms(nnn_mix *m, const int *idx, int n, int32_t *room);
int nnn_mix_set_gains(nnn_mix *m, const int *idx, int n, const float *gain);
int nnn_mix_get_gains(nnn_mix *m, const int *idx, int n, float *gain);

/* prev = 0 for the listed streams (idx == NULL: every stream, n is ignored).  Rooms and gains stay. */
int nnn_mix_reset(nnn_mix *m, const int *idx, int n);

/*
 * n_frames >= 1 frames of every stream.  Sample i of frame t of stream s: d_in [s * in_stream_stride + t * in_frame_stride + i] and
 * d_out [s * out_stream_stride + t * out_frame_stride + i] (strides in floats, the addressing of nnn_batch_process_device on each side:
 * frame strides >= 480; 4-byte alignment is all the bases need).
 * d_out   must not overlap d_in: an output needs every member's input.  Equal bases are refused; any other overlap is the caller's error.
 * d_talk  NULL (everybody talks), or uint8 [n_frames][n_streams] in device memory: exactly the gate's d_open.
 * d_live  NULL, or uint8 [n_streams] in device memory (see above).
 * d_heard NULL, or int32 [n_frames][n_streams] in device memory: step 7.
 * hip_stream: a hipStream_t (NULL = the object's own stream).
 */
int nnn_mix_apply_device(nnn_mix *m, const float *d_in, float *d_out, const uint8_t *d_talk, const uint8_t *d_live, int32_t *d_heard,
                         int n_frames, size_t in_stream_stride, size_t in_frame_stride, size_t out_stream_stride, size_t out_frame_stride,
                         void *hip_stream);
/*
 * The same on the packed boundary of nnn_batch_process_pcm_device, a layout per side: NNN_PCM_F32, NNN_PCM_I16 and NNN_PCM_F32_UNIT
 * independently (int16 legs in and a float monitor out is a real case), channel-interleaved groups addressed in elements as there.
 * discard_first must be 0 and n_streams a multiple of each side's channels.  The bases are aligned to their elements.  A stereo
 * participant is two streams in two rooms.  The same aliasing rule.
 */
int nnn_mix_apply_pcm_device(nnn_mix *m, const void *d_in, void *d_out, const uint8_t *d_talk, const uint8_t *d_live, int32_t *d_heard,
                             int n_frames, const nnn_pcm_layout *in_layout, const nnn_pcm_layout *out_layout, void *hip_stream);
/* Host memory, synchronous: in / out dense f32 [n_streams][n_frames][480] (out must not be in), talk NULL or [n_frames][n_streams],
 * live NULL or [n_streams], heard NULL or [n_frames][n_streams]; what a stream marked 0 owns in out and heard is left as it was. */
int nnn_mix_apply_host(nnn_mix *m, const float *in, float *out, const uint8_t *talk, const uint8_t *live, int32_t *heard, int n_frames);

#ifdef __cplusplus
}
#endif
#endif /* NNN_MIX_H */
