// SPDX-License-Identifier: BSD-3-Clause
/*
 * nnn_pick.h -- the talker picker: the step a conference bridge puts between the VAD gate and the mixer.  Of every
 * room's open gates it forwards the k loudest, with hysteresis so that the set does not flap, a pin for moderators, and the room's
 * dominant speaker for the UI -- on the device, where the denoised audio, the gate's d_open rows and the batch's held mask are already.
 * What it writes, d_talk, is what nnn_mix_apply_* takes as d_talk.
 *
 * An object beside the batch, like the gate and the mixer: it changes no call and no kernel of theirs.  There is no node mirror: a node's
 * host makes one picker per shard, next to the shard's gate and mixer, and rooms do not span shards.
 *
 * An object holds, for each of its n_streams streams,
 *   configuration   room      int32 in -1 .. n_streams - 1: a label, the mixer's; -1 = alone, the same as a room of one      -1 at creation
 *                   pinned    uint8 0 or 1: a moderator or presenter                                                        0
 *   state           level     f64: the decayed peak of the stream's frame energies                                        +0.0, and after reset
 *                   selected  uint8: talk of the stream's last live frame                                                  0, and after reset
 * and for the whole object the policy
 *                   k         int in 1 .. NNN_PICK_MAX_K: talkers forwarded per room                                        3
 *                   decay     f32 in [0, 1], used as (double)decay: what a frame leaves of the level                        0.875
 *                   stick     f32 in [1, 16], used as (double)stick: by how much a challenger must exceed an incumbent      4
 * NaN policy values are refused.  The members of a room are its streams in ascending stream index.
 *
 * THE RULE (the contract: a restatement that follows it gives the same bits; tests/pick_cases.py is one).  A stream's frames are numbered
 * n = 0, 1, ... over its live frames since its last reset.  For frame n of a live stream s, open_n is its d_open entry (any non-zero byte
 * is 1), or 1 where d_open is NULL; x[i] are its 480 samples after the format's loader ((float) of an int16, unit floats times 32768.0f
 * in binary32, plain floats as they are).
 *   1. energy.   If open_n: e = sum of (double)x[i] * (double)x[i] (each product exact in binary64) in exactly the order nnn_score.h
 *      states -- 64 partial sums p_L from +0.0 over i = L, L + 64, ... in ascending order, then p_L <- p_L + p_(L xor m) for m = 32, 16,
 *      8, 4, 2, 1, the sum is p_0 --, every addition one IEEE binary64 operation, nothing contracted.  e_n = (e <= DBL_MAX) ? e : +0.0: a
 *      frame holding a NaN or inf sample measures as silent.  If !open_n: e_n = +0.0 and the stream-frame's input is not read: whatever
 *      bytes lie there, NaN included, cannot matter.
 *   2. level.    d = level_(n-1) * (double)decay;  level_n = (e_n > d) ? e_n : d.  One binary64 multiplication and one comparison:
 *      instant attack, geometric release.  level_(-1) is the state.
 *   3. ranking.  The candidates of a room in frame n are its live members with open_n == 1.  A candidate's score is
 *      level_n * (double)stick if selected_(n-1), else level_n (selected_(-1) is the state).  The candidates are ranked by
 *        - pinned, descending;
 *        - then score, descending, compared as the u64 bit pattern of the (non-negative) double: no float comparison is involved;
 *        - then stream index, ascending.
 *   4. selection.  talk_n = 1 for the first min(k, number of candidates) candidates in that order, 0 for every other live member;
 *      selected_n = talk_n.
 *   5. optional outputs per live stream-frame: dominant (int32) = the stream index of the room's first-ranked candidate, -1 when it has
 *      none; level (f64) = level_n.
 *   6. a stream marked 0 in d_live sits the call out: for that call it is no member of its room; nothing of it is read or written -- not
 *      its input, not its d_open entries, not its rows of the outputs -- and its state does not move.  This is how the streams a batch
 *      holds pass (live = !held).
 *
 * What follows from the rule (each has a test):
 *   - talk is a subset of open
 *   - at most k talkers per room-frame
 *   - a room-frame with at most k candidates has talk == open
 *   - a challenger displaces an incumbent only when its level exceeds stick x the incumbent's (or equals it to the bit and the
 *     challenger has the lower stream index)
 *   - equal scores go to the lower stream index
 *   - a pinned open stream is always selected while the room's pinned candidates number at most k
 *   - the bits depend on the frame's number, the parameters and the masks alone: not on how the frames are cut into calls, on layout,
 *     format (for samples the formats hold alike), alignment, room labels or n_streams
 *
 * Plain C ABI; all functions return 0 on success (nnn_last_error() of nnn_batch.h has the text); no CPU fallback.  Everything is
 * checked before anything changes: a refused call leaves the object as it was.  Calls with a stream are asynchronous on it; calls of one
 * object made on different streams are ordered by the object.
 */
#ifndef NNN_PICK_H
#define NNN_PICK_H

#include <stddef.h>
#include <stdint.h>

#include "nnn_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nnn_pick nnn_pick;

#define NNN_PICK_FRAME 480
#define NNN_PICK_MAX_K 8
#define NNN_PICK_MAX_STICK 16
/* tuning, not contract: no output bit depends on either.  How the ranking kernel seats a room: alone on a lane; up to SEG_ROOM members
 * on a run of SEG_ROOM lanes; up to WAVE_ROOM on a wave; beyond that on a block, its members strided over the threads. */
#define NNN_PICK_SEG_ROOM 8
#define NNN_PICK_WAVE_ROOM 64

/* 1 <= n_streams.  Every stream alone (room -1), unpinned, level +0.0, not selected; k 3, decay 0.875, stick 4.  Device memory: about
 * 40 bytes per stream, and 8 bytes per stream-frame of the longest call. */
nnn_pick *nnn_pick_create(int n_streams, int device);
void nnn_pick_destroy(nnn_pick *p);

/* The rooms and pins of the listed streams (idx == NULL: streams 0 .. n - 1).  A value out of range, an index outside the object or one
 * listed twice refuses the whole call.  The setters wait for the calls enqueued so far, rebuild the member tables on the host
 * (page-locked) and upload them; a changed value is in force from the next call's first frame.  Neither touches level or selected: a
 * stream moved while selected keeps its incumbent's bonus in the room it enters until it loses a ranking there.  The getters read the
 * host's copy and wait for nothing. */
int nnn_pick_set_rooms(nnn_pick *p, const int *idx, int n, const int32_t *room);
int nnn_pick_get_rooms(nnn_pick *p, const int *idx, int n, int32_t *room);
int nnn_pick_set_pinned(nnn_pick *p, const int *idx, int n, const uint8_t *pinned);
int nnn_pick_get_pinned(nnn_pick *p, const int *idx, int n, uint8_t *pinned);

/* The policy of the whole object; in force from the next call's first frame.  get: any of the three pointers may be NULL. */
int nnn_pick_set_policy(nnn_pick *p, int k, float decay, float stick);
int nnn_pick_get_policy(nnn_pick *p, int *k, float *decay, float *stick);

/* level = +0.0 and selected = 0 for the listed streams (idx == NULL: every stream, n is ignored).  Rooms, pins and policy stay. */
int nnn_pick_reset(nnn_pick *p, const int *idx, int n);

/*
 * n_frames >= 1 frames of every stream.  Sample i of frame t of stream s: d_in [s * stream_stride + t * frame_stride + i] (strides in
 * floats, the addressing of nnn_batch_process_device: frame_stride >= 480; 4-byte alignment is all the base needs).  The input is only
 * read.
 * d_open      NULL (every gate is open), or uint8 [n_frames][n_streams] in device memory: exactly the gate's d_open.
 * d_live      NULL, or uint8 [n_streams] in device memory (see above).
 * d_talk      uint8 [n_frames][n_streams] in device memory: exactly what nnn_mix_apply_* takes as d_talk.  It may be d_open itself (equal
 *             bases: every byte is read before it is written, by the thread that writes it); any other overlap is the caller's error.
 * d_dominant  NULL, or int32 [n_frames][n_streams] in device memory: step 5.
 * d_level     NULL, or double [n_frames][n_streams] in device memory, 8-byte aligned: step 5.
 * hip_stream: a hipStream_t (NULL = the object's own stream).
 */
int nnn_pick_select_device(nnn_pick *p, const float *d_in, const uint8_t *d_open, const uint8_t *d_live, uint8_t *d_talk, int32_t *d_dominant,
                           double *d_level, int n_frames, size_t stream_stride, size_t frame_stride, void *hip_stream);
/*
 * The same on the packed boundary of nnn_batch_process_pcm_device: NNN_PCM_F32, NNN_PCM_I16 and NNN_PCM_F32_UNIT, channel-interleaved
 * groups addressed in elements as there.  discard_first must be 0 and n_streams a multiple of channels.  The base is aligned to its
 * elements.  A stereo participant is two streams.
 */
int nnn_pick_select_pcm_device(nnn_pick *p, const void *d_in, const uint8_t *d_open, const uint8_t *d_live, uint8_t *d_talk, int32_t *d_dominant,
                               double *d_level, int n_frames, const nnn_pcm_layout *layout, void *hip_stream);
/* Host memory, synchronous: in dense f32 [n_streams][n_frames][480], open NULL or [n_frames][n_streams], live NULL or [n_streams], talk
 * [n_frames][n_streams], dominant and level NULL or [n_frames][n_streams]; what a stream marked 0 owns in the outputs is left as it was. */
int nnn_pick_select_host(nnn_pick *p, const float *in, const uint8_t *open, const uint8_t *live, uint8_t *talk, int32_t *dominant, double *level,
                         int n_frames);

#ifdef __cplusplus
}
#endif
#endif /* NNN_PICK_H */
