/* SPDX-License-Identifier: BSD-3-Clause */
/*
 * nnn_pack.h -- file packer: files of unequal length through one batch, slots refilled.
 *
 * The reference CLI denoises one file per process (src/nnnoiseless.rs:301-331): read whole frames until a short read ends the loop,
 * process every frame, write every frame but the first.  A packer is that loop for a whole corpus on one batch: the files lie in one
 * input arena in device memory, their outputs go to one output arena, and the batch's slots -- `channels` consecutive streams each --
 * take file after file until none is left.
 * For file i with n_i sample frames of C interleaved channels:
 *   F_i = n_i / 480 whole frames are processed (the trailing partial frame is dropped);
 *   (F_i - 1) * 480 * C output elements are written at out_off (the first frame is processed and not written);
 *   F_i * C VAD values are written at vad_off, value of frame f of channel c at vad_off + f * C + c.
 * What a file gets is, bit for bit, what it gets alone: a fresh batch of C streams and nnn_batch_process_pcm_* with channels = C and
 * discard_first over its F_i frames -- for any number of slots, any step_frames, any order and any mix of lengths.  A file with
 * F_i == 0 takes no slot and writes nothing; one with F_i == 1 writes its C VAD values and no audio.  Outside the files' own output
 * ranges not a byte of either output arena is written.
 *
 * A run is a sequence of STEPS, each one ordinary processing call of the batch:
 *   - before a step, free slots take the next files in list order, lowest slot first, and are reset (nnn_batch_reset_streams);
 *   - the step has n_k = min(step_frames, the longest remaining run among the occupied slots) frames;
 *   - a file that ends inside a step leaves its slot fed with zeros for the rest of it; those frames' output and VAD are discarded,
 *     and the slot is free from the next step on;
 *   - slots with no file left are held (nnn_batch_hold_streams) for the rest of the run;
 *   - at the end every hold is released and every slot the run used is reset: the batch leaves a run with every stream in its
 *     freshly-created state and nothing held (its frame count has moved: discard_first of a later call of the caller's own sees a
 *     batch that has processed frames; nnn_batch_reset clears that too).
 * Gain floors and the channel link are the batch's configuration and apply as in any ordinary call.
 *
 * Plain C ABI; 0 on success (nnn_last_error() of nnn_batch.h has the text); no CPU fallback.
 */
#ifndef NNN_PACK_H
#define NNN_PACK_H

#include <stddef.h>
#include <stdint.h>

#include "nnn_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nnn_pack nnn_pack;

/* Input formats beside NNN_PCM_F32 and NNN_PCM_I16 (same numeric values as in nnn_batch.h), converted to the i16-range floats
 * process_frame takes exactly as the CLI's readers do (src/nnnoiseless.rs:189-227):
 *   NNN_PACK_I24      packed little-endian 24-bit integers, 3 bytes an element: (float)(s >> 8) of the sign-extended sample
 *   NNN_PACK_I32      32-bit integers: (float)(s >> 16)
 *   NNN_PACK_F32_WAV  WAV floats in [-1, 1]: s * 32767.0f, one rounding
 * Output formats: NNN_PCM_F32 (the floats as process_frame leaves them) and NNN_PCM_I16 (clamp and round half away, the CLI's writers). */
enum nnn_pack_format { NNN_PACK_I24 = 16, NNN_PACK_I32 = 17, NNN_PACK_F32_WAV = 18 };

/* One file: where it lies in the input arena, how long it is, where its audio and its VAD values go.  Offsets in ELEMENTS of the
 * respective arena's format (a 24-bit element is 3 bytes; VAD values are floats) and arbitrary: an int16 span may start on an odd
 * element, a 24-bit span on any byte.  n_frames_samples = sample frames, i.e. samples per channel. */
typedef struct nnn_pack_file {
    uint64_t in_off, n_frames_samples, out_off, vad_off;
} nnn_pack_file;

/* Borrows b (b must outlive the packer).  A slot is `channels` consecutive streams: n_streams / channels slots.  step_frames = the
 * longest step, 0 = nnn_batch_max_group_frames(b); it sizes the staging rows (step_frames * 480 floats per stream), allocated here with
 * the descriptor tables and the page-locked memory they go up from.  Also makes the batch's empty first hold (nnn_batch_hold_streams(b,
 * NULL, 0)), so that no run stalls on it.
 * Refused (NULL): a NULL batch, channels < 1 or not dividing n_streams, step_frames outside [0, nnn_batch_max_group_frames(b)], a batch
 * with more than one model group (a file may land in any slot). */
nnn_pack *nnn_pack_create(nnn_batch *b, int channels, int step_frames);
void nnn_pack_destroy(nnn_pack *p);

/*
 * The plan of a run, pure host arithmetic (no batch, no device): the rule above applied to file_frames[i] = F_i WHOLE frames.
 *   slot_of_file[i]        the slot file i runs in, -1 for a file with F_i == 0
 *   first_step_of_file[i]  the step its frame 0 is the first frame of, -1 likewise
 * (either may be NULL).  summary, in SLOT units (a plan knows no channel count; a slot-frame is `channels` stream-frames):
 *   [0] steps                 [1] useful slot-frames = sum of F_i        [2] padded slot-frames (zeros behind a file's end)
 *   [3] held slot-steps       [4] slot-frames launched = n_slots * sum of n_k
 *   [5] held slot-frames (the held share of [4]: [1] + [2] + [5] == [4])
 *   [6] files that took a slot                                            [7] the largest padding of any one file (<= step_frames - 1)
 * Refused: n_slots < 1, step_frames < 1, n_files < 0, a NULL list with n_files > 0, a NULL summary, a file of 2^31 frames or more.
 * This is the function nnn_pack_run_* walk.
 */
int nnn_pack_plan(int n_slots, int step_frames, const uint64_t *file_frames, int n_files, int32_t *slot_of_file, int32_t *first_step_of_file,
                  int64_t summary[8]);

/*
 * One run: n_files files of the input arena d_in (in_elems elements of in_format) into the output arena d_out (out_elems elements of
 * out_format) and, unless d_vad is NULL, the VAD arena d_vad (vad_elems floats).  `files` is host memory and is read before the call
 * returns.  Asynchronous on hip_stream (NULL = the batch's own stream, as in nnn_batch_process_device): every step's descriptor table
 * goes up from a small ring of page-locked tables guarded by events, then k_pack_in, the batch's ordinary call and k_pack_out are
 * enqueued; the host waits only where it is about to overwrite a table whose copy, four steps back, is not done yet (and where
 * nnn_batch_reset_streams / nnn_batch_hold_streams wait for their own list buffer).
 * Everything is checked before anything is enqueued, and a refusal changes nothing.  Refused: a NULL packer, arena (d_in, d_out) or
 * file list; n_files < 0; an unknown format; a file whose input span (n_frames_samples * channels elements), output span or VAD span
 * leaves its arena; any stream held on entry; frames pending from an nnn_batch_analyze_*; a set nnn_batch_fault; a batch under
 * nnn_batch_set_inputs_ready(b, 1).  Output ranges of different files must not overlap (not checked).
 */
int nnn_pack_run_device(nnn_pack *p, const void *d_in, uint64_t in_elems, int in_format, void *d_out, uint64_t out_elems, int out_format,
                        float *d_vad, uint64_t vad_elems, const nnn_pack_file *files, int n_files, void *hip_stream);
/* The same with host arenas, staged in one piece (the output arenas make the round trip, so that bytes outside the files' ranges come
 * back as they were); synchronous. */
int nnn_pack_run_host(nnn_pack *p, const void *in, uint64_t in_elems, int in_format, void *out, uint64_t out_elems, int out_format,
                      float *vad, uint64_t vad_elems, const nnn_pack_file *files, int n_files);
/* The summary of the most recent run, as nnn_pack_plan reports it but in STREAM units: [1], [2], [4] and [5] are stream-frames and [3]
 * stream-steps (the plan's figures times `channels`).  All zero before the first run. */
int nnn_pack_last_summary(const nnn_pack *p, int64_t summary[8]);
/* Measuring hook: one of the two kernels alone, `reps` launches of a full step of n_frames (<= step_frames) frames on every slot, with
 * nothing skipped and no batch call in between.  which = 0: k_pack_in from a dense arena d_in (slot g's span at element g * n_frames * 480 *
 * channels, in_format) into the staging; which = 1: k_pack_out from the staging into a dense arena d_out laid out the same way
 * (out_format).  The arena of the other direction is not used and may be NULL.  Waits for hip_stream before it fills its table and
 * returns with the launches enqueued; the batch is not touched. */
int nnn_pack_debug_kernels(nnn_pack *p, int which, const void *d_in, int in_format, void *d_out, int out_format, int n_frames, int reps,
                           void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* NNN_PACK_H */
