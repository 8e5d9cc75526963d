// SPDX-License-Identifier: BSD-3-Clause
/*
 * nnn_gate.h -- the VAD gate: the step a voice server puts behind the denoiser.  Per stream a threshold on the
 * speech probability the batch returns, a grace period that keeps the gate open after speech, a look-back that delays the audio a few
 * frames so that the onset which made the VAD fire is not cut, and a gain for the closed gate (0 = mute), all on the device: the audio
 * never crosses the bus for it and the per-frame counter is one small kernel instead of a scan in the host's framework.
 *
 * An object beside the batch, like the scorer: it changes no call and no kernel of the batch.  There is no node mirror: a node's host
 * makes one gate per shard, next to the shard's batch (nnn_node_batch).
 *
 * An object holds, for each of its n_streams streams,
 *   configuration   threshold  f32 in [0, 1]                           0 at creation: vad >= 0, so the gate never closes once it saw a frame
 *                                                                       (that first frame still fades in from `level`: see the rule's h_(-1))
 *                   grace      int32 G, 0 .. NNN_GATE_MAX_GRACE        0
 *                   lookback   int32 R, 0 .. max_lookback              0
 *                   level      f32 in [0, 1], the gain while closed    0 (mute)
 *   state           since      int32: frames since the last voiced frame; NNN_GATE_NEVER at creation and after a reset, where it saturates
 *                   was_open   the previous frame's decision           0
 *                   history    the last R input frames as floats ((float) of an int16 is exact), oldest first; zeros
 *
 * THE RULE (the contract: a restatement that follows it gives the same bits; tests/gate_cases.py is one).  The stream's frames are
 * numbered n = 0, 1, ... since its last reset; vad_n is its d_vad entry and in_n its 480 input samples of frame n.
 *   1. voiced_n = vad_n >= threshold                          (NaN is not voiced)
 *   2. since_n  = voiced_n ? 0 : min(since_(n-1) + 1, NNN_GATE_NEVER)
 *   3. open_n   = since_n <= G + R
 *      One counter covers both grace periods: the frame delivered at n is input frame n - R, and it is open exactly when some frame in
 *      [n - R - G, n] was voiced.
 *   4. h_n = open_n ? 1.0f : level,  h_(-1) = level
 *   5. the source  x[i] = in_(n-R)[i], zeros for n - R < 0
 *   6. the gain    g_i = h_n                                       if h_(n-1) == h_n
 *                  g_i = h_(n-1) + (h_n - h_(n-1)) * RAMP[i]       otherwise, RAMP[i] = (float)(i + 1) / 480.0f
 *      every operation one IEEE binary32 operation, round to nearest even, nothing contracted into a fused multiply-add
 *   7. the output  y[i] = x[i]          if g_i == 1.0f: bit for bit, NaN, inf and -0.0 included
 *                  y[i] = +0.0f         if g_i == 0.0f, whatever x[i] is: a muted stream emits exact zeros
 *                  y[i] = x[i] * g_i    otherwise (which NaN a NaN sample becomes here is not part of the contract)
 * Since h_(-1) = level and was_open = 0 after a reset, a stream's first frame after creation, reset, set_params is the ramp from `level` up to
 * 1 whenever that frame is open and level < 1: a host that wants frame 0 untouched sets level = 1 or feeds one frame first.
 * The output depends on the frame's number and the stream's parameters alone: not on how the frames are cut into calls, on layout,
 * alignment or n_streams.  The delivered audio is the input R frames late; to drain a stream's last R frames the host feeds it R more
 * frames with VAD below the threshold (any audio: it is never delivered).
 *
 * Plain C ABI; all functions return 0 on success (nnn_last_error() of nnn_batch.h has the text); no CPU fallback.  Everything is
 * checked before anything changes: a refused call leaves the object as it was.  Calls with a stream are asynchronous on it; calls of one
 * object made on different streams are ordered by the object.
 */
#ifndef NNN_GATE_H
#define NNN_GATE_H

#include <stddef.h>
#include <stdint.h>

#include "nnn_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nnn_gate nnn_gate;

#define NNN_GATE_FRAME 480
#define NNN_GATE_MAX_LOOKBACK 8     /* frames: 80 ms */
#define NNN_GATE_MAX_GRACE 6000     /* frames: one minute */
#define NNN_GATE_NEVER 0x7fffffff

typedef struct nnn_gate_params {
    float threshold;
    int32_t grace;
    int32_t lookback;
    float level;
} nnn_gate_params;

/*
 * A stream's record, NNN_GATE_STATE_BYTES bytes whatever the object's max_lookback, little-endian:
 *    0  uint32  NNN_GATE_STATE_MAGIC          4  uint32  NNN_GATE_STATE_VERSION       8  uint32  NNN_GATE_STATE_BYTES
 *   12  f32     threshold                    16  int32   grace                       20  int32   lookback R
 *   24  f32     level                        28  int32   since                       32  uint32  was_open (0 or 1)
 *   36  12 bytes, zero
 *   48  f32 [8][480]  the history: row r < R is input frame n - R + r (n = the next frame's number), rows r >= R are zeros
 */
#define NNN_GATE_STATE_MAGIC 0x3147564Eu   /* "NVG1" */
#define NNN_GATE_STATE_VERSION 1
#define NNN_GATE_STATE_BYTES (48 + NNN_GATE_MAX_LOOKBACK * NNN_GATE_FRAME * 4)

/* 1 <= n_streams, 0 <= max_lookback <= NNN_GATE_MAX_LOOKBACK.  Device memory: 1920 x max_lookback + 25 bytes per stream, and one byte
 * per stream-frame of the longest call. */
nnn_gate *nnn_gate_create(int n_streams, int max_lookback, int device);
void nnn_gate_destroy(nnn_gate *g);

/* The parameters of the listed streams (idx == NULL: streams 0 .. n - 1).  set also resets those streams (since, was_open, history): a
 * history taken under one look-back means nothing under another.  A parameter out of range or NaN, an index outside the object or one
 * listed twice refuses the whole call.  set waits for the calls enqueued so far; get reads the host's copy and waits for nothing. */
int nnn_gate_set_params(nnn_gate *g, const int *idx, int n, const nnn_gate_params *params);
int nnn_gate_get_params(nnn_gate *g, const int *idx, int n, nnn_gate_params *params);

/* since = NNN_GATE_NEVER, was_open = 0 and a history of zeros for the listed streams (idx == NULL: every stream, n is ignored).  The
 * parameters stay. */
int nnn_gate_reset(nnn_gate *g, const int *idx, int n);

/*
 * n_frames >= 1 frames of every stream.  Sample i of frame t of stream s: d_in / d_out [s * stream_stride + t * frame_stride + i]
 * (strides in floats, the addressing of nnn_batch_process_device: frame_stride >= 480; 4-byte alignment is all the bases need).
 * d_vad   [t * n_streams + s], as the batch writes it.
 * d_out   equals d_in (in place, the server's normal case; the strides are shared, so base equal is exactly equal) or does not overlap
 *         it.  Anything else is the caller's error.
 * d_live  NULL, or uint8 [n_streams] in device memory.  A stream marked 0 sits the call out: its input, VAD entries, output and d_open
 *         entries are neither read nor written and its state does not move.  This is how the streams a batch holds pass through
 *         (nnn_batch_held_mask gives the host copy; live = !held).
 * d_open  NULL, or uint8 [n_frames][n_streams]: open_n of each delivered frame -- the talking indicator or DTX flag.
 * hip_stream: a hipStream_t (NULL = the object's own stream).  Any n_frames >= 1; scratch is grow-only.
 */
int nnn_gate_apply_device(nnn_gate *g, const float *d_in, float *d_out, const float *d_vad, const uint8_t *d_live, uint8_t *d_open,
                          int n_frames, size_t stream_stride, size_t frame_stride, void *hip_stream);
/*
 * The same on the packed boundary of nnn_batch_process_pcm_device: NNN_PCM_F32, NNN_PCM_F32_UNIT (both: step 7 on the floats as they
 * are) and NNN_PCM_I16 (the sample is (float)x; y is rounded half away from zero and clamped to int16 as the batch's int16 writer does,
 * so an open gate returns the int16 unchanged), channels-interleaved groups addressed in elements as there.  discard_first must be 0
 * and n_streams a multiple of channels.  The bases are aligned to their elements.  The same aliasing rule.
 */
int nnn_gate_apply_pcm_device(nnn_gate *g, const void *d_in, void *d_out, const float *d_vad, const uint8_t *d_live, uint8_t *d_open,
                              int n_frames, const nnn_pcm_layout *layout, void *hip_stream);
/* Host memory, synchronous: in / out dense f32 [n_streams][n_frames][480] (out may be in), vad [n_frames][n_streams], live NULL or
 * [n_streams], open NULL or [n_frames][n_streams]; what a stream marked 0 owns in out and open is left as it was. */
int nnn_gate_apply_host(nnn_gate *g, const float *in, float *out, const float *vad, const uint8_t *live, uint8_t *open, int n_frames);

/* State transfer: host records (the layout above), synchronous.  A stream exported and imported into another object -- one with another
 * n_streams or max_lookback -- continues bit for bit.  import checks every record and index first: a wrong magic, version or size, a
 * parameter out of range, a lookback above the target's max_lookback, a repeated index refuse the whole call. */
size_t nnn_gate_state_bytes(const nnn_gate *g);
int nnn_gate_export_streams(nnn_gate *g, const int *idx, int n, void *records, size_t bytes);
int nnn_gate_import_streams(nnn_gate *g, const int *idx, int n, const void *records, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* NNN_GATE_H */
