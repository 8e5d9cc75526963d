// SPDX-License-Identifier: BSD-3-Clause
/*
 * nnn_batch.h -- batched entry points of the MI355X process_frame backend.
 *
 * The reference has no batched API: its only "N independent states in lock-step" call sites are
 * the per-channel loops `for ch { states[ch].process_frame(out[ch], in[ch]) }` at
 * src/signal.rs:102-104 and src/nnnoiseless.rs:318-320.  nnn_batch_process_* replaces exactly
 * that loop: n_streams independent DenoiseState's (src/denoise.rs:37-42) advanced by n_frames
 * calls of DenoiseState::process_frame (src/denoise.rs:95-116) each.
 *
 * Plain C ABI: pointers and sizes only.  All functions return 0 on success, non-zero on error
 * (nnn_last_error() has the text); nothing falls back to a CPU path.
 */
#ifndef NNN_BATCH_H
#define NNN_BATCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nnn_batch nnn_batch;
#ifndef RNNOISE_H
typedef struct RNNModel RNNModel;
#endif

#define NNN_FRAME_SIZE 480 /* DenoiseState::FRAME_SIZE, src/denoise.rs:46 */

/* RnnModel::from_bytes (src/rnn.rs:75-77, validation :116-232): NULL where the reference returns None. */
RNNModel *nnn_model_from_bytes(const uint8_t *bytes, size_t len);
/* RnnModel::default (src/rnn.rs:235-240): the built-in weights.rnn. */
RNNModel *nnn_model_default(void);
/* RNNoise / rnnoise-nu TEXT model ("rnnoise-nu model file version 1" + whitespace-separated integers) -> the binary
 * .rnn format: what the reference's train/convert_rnnoise.py:18-29 does (drop the header line, every integer modulo
 * 256 as one byte).  nnn_convert_rnnoise_text writes the bytes to out (cap bytes of room) and returns their count, or
 * -1 on a wrong header / a token that is not an integer / too little room (pass out = NULL to get the count only).
 * nnn_model_from_rnnoise_text = convert + nnn_model_from_bytes. */
long nnn_convert_rnnoise_text(const char *text, size_t len, uint8_t *out, size_t cap);
RNNModel *nnn_model_from_rnnoise_text(const char *text, size_t len);
void nnn_model_free(RNNModel *m);
/* RnnModel is Clone (#[derive(Clone)], src/rnn.rs:54): an independent copy of the parameters, freed with nnn_model_free.
 * NULL on a NULL model. */
RNNModel *nnn_model_clone(const RNNModel *m);
/* shape[0..5] = input_dense in/out, vad/noise/denoise GRU neurons, gains out; shape[6..11] = activations */
void nnn_model_shape(const RNNModel *m, int32_t shape[12]);

/* n_streams x DenoiseState::with_model(model) (src/denoise.rs:72-74); model NULL = DenoiseState::new().
 * The model is copied to the device; it need not outlive the batch.  device = HIP device ordinal. */
nnn_batch *nnn_batch_create(const RNNModel *model, int n_streams, int device);
/* Several models resident at once (e.g. the rnnoise-nu model zoo, one model per audience): streams
 * [0, group_streams[0]) run models[0], the next group_streams[1] run models[1], ...  Every group but the last must be
 * a multiple of 64 streams (the kernels' tile).  models == NULL or models[i] == NULL selects the built-in model.
 * Everything except the RNN kernel is model-independent; the RNN runs as one launch per group. */
nnn_batch *nnn_batch_create_grouped(const RNNModel *const *models, const int *group_streams, int n_groups, int device);
/* The same with options (NULL = defaults; zero-initialise the struct).
 * max_group_frames: the kernels work on groups of consecutive frames -- up to 24 by default, which sizes the per-stream scratch
 * and history rings for it (360 KB per stream).  A host whose calls are short says so here and gets a batch sized for groups of
 * that many frames: a real-time host that ticks ONE 10 ms frame per call passes 1 and pays 33 KB per stream (the reference's
 * DenoiseState is 10.3 KB, src/features.rs:18-46), i.e. 8.7 million live streams' worth of HBM instead of 800 thousand.  Longer
 * calls still work on such a batch, cut into groups of at most this many frames (slower, same results).  0 = default;
 * values above 24 (the kernels' longest group) are rejected.  How many groups a batch keeps in flight (1, or 2 under
 * NNN_LANES >= 2 / NNN_SCHED=stages) is fixed when it is created -- nnn_batch_set_schedule on an existing batch works with
 * the scratch sets and ring slots that are there -- and is part of what a state snapshot must match. */
typedef struct nnn_batch_opts {
    int max_group_frames;
    int reserved[7];                     /* must be zero */
} nnn_batch_opts;
nnn_batch *nnn_batch_create_opts(const RNNModel *const *models, const int *group_streams, int n_groups, int device,
                                 const nnn_batch_opts *opts);
int nnn_batch_max_group_frames(const nnn_batch *b);
/* Device memory the batch holds (state, scratch, tables, weights), bytes. */
size_t nnn_batch_device_bytes(const nnn_batch *b);
void nnn_batch_destroy(nnn_batch *b);
int nnn_batch_num_streams(const nnn_batch *b);
/* Back to freshly-created state (all zeros, src/features.rs:58-74). */
int nnn_batch_reset(nnn_batch *b);

/* DenoiseState is Clone (src/denoise.rs:36): a second batch with the same models and a copy of every stream's state as of
 * the calls made so far (device-to-device copy; waits for them).  NULL on failure.  The two continue independently and, fed
 * the same input, bit-identically. */
nnn_batch *nnn_batch_clone(nnn_batch *b);
/* The same state as host bytes: nnn_batch_state_bytes() of them.  A snapshot only loads into a batch of the same stream
 * count and models made by the same build of the library (it is a raw image of the state slab, not an interchange
 * format). */
size_t nnn_batch_state_bytes(const nnn_batch *b);
int nnn_batch_save_state(nnn_batch *b, void *host_dst, size_t dst_bytes);
int nnn_batch_load_state(nnn_batch *b, const void *host_src, size_t src_bytes);

/*
 * Per-stream state records: ONE stream's DenoiseState (src/denoise.rs:37-42) in the reference's own terms, independent of the batch
 * it came from (no ring slots, tiles, frame counts or group sizes): a record exported from any slot of any batch imports into any
 * slot of any other batch -- another max_group_frames, stream count, frame count, device, or a lone DenoiseState -- whose stream
 * runs a model of the same GRU sizes, and both continue bit-identically.  Fixed size, 16-byte multiple, little-endian, 32-bit words
 * (f32 unless marked).  Byte offsets:
 */
#define NNN_STREAM_STATE_BYTES 11232
#define NNN_STREAM_STATE_VERSION 1
#define NNN_STREAM_STATE_MAGIC 0x3153534Eu        /* "NSS1" */
#define NNN_STREAM_STATE_OFF_MAGIC 0              /* u32 NNN_STREAM_STATE_MAGIC                                                   */
#define NNN_STREAM_STATE_OFF_VERSION 4            /* u32 NNN_STREAM_STATE_VERSION                                                 */
#define NNN_STREAM_STATE_OFF_SIZE 8               /* u32 NNN_STREAM_STATE_BYTES                                                   */
#define NNN_STREAM_STATE_OFF_GRU_SIZES 12         /* i32 [3] vad / noise / denoise GRU neurons of the model (src/rnn.rs:65-70)    */
#define NNN_STREAM_STATE_OFF_MEM_ID 24            /* i32 cepstral ring position (src/features.rs:26)                             */
#define NNN_STREAM_STATE_OFF_LAST_PERIOD 28       /* i32 PitchFinder::last_period (src/pitch.rs:5)                               */
#define NNN_STREAM_STATE_OFF_LAST_GAIN 32         /* f32 PitchFinder::last_gain                                                  */
#define NNN_STREAM_STATE_OFF_MEM_HP_X 36          /* f32 [2] high-pass biquad state (src/features.rs:27)                         */
                                                  /* 44 .. 63 reserved, zero                                                      */
#define NNN_STREAM_STATE_OFF_INPUT_MEM 64         /* f32 [1728] high-passed input history, oldest first (src/features.rs:97-104)  */
#define NNN_STREAM_STATE_OFF_SYNTHESIS_MEM 6976   /* f32 [480] overlap memory (src/features.rs:263-275)                          */
#define NNN_STREAM_STATE_OFF_CEPSTRAL_MEM 8896    /* f32 [8][22] cepstral history, [ring slot][band] (src/features.rs:167-194)   */
#define NNN_STREAM_STATE_OFF_LASTG 9600           /* f32 [22] last applied gains (src/denoise.rs:106-109), then 2 zero words     */
#define NNN_STREAM_STATE_OFF_VAD_GRU 9696         /* f32 [128] the first nv used, the rest zero (src/rnn.rs:330-341)             */
#define NNN_STREAM_STATE_OFF_NOISE_GRU 10208      /* f32 [128] the first nn used                                                  */
#define NNN_STREAM_STATE_OFF_DENOISE_GRU 10720    /* f32 [128] the first ndn used                                                 */
/*
 * streams[i] (host memory) names the stream of record i.  Work is enqueued in call order with the processing calls -- after every call
 * made before, before every call made after, pipelined calls under nnn_batch_set_inputs_ready included -- on the batch's own stream
 * (host variants; they wait for it) or on hip_stream (device variants, NULL = the batch's own stream; they return once the work is
 * enqueued).  Every call checks everything it can before it writes anything and refuses, changing nothing, on: an index outside
 * [0, n_streams); a repeated index (import, reset); a record whose magic, version, size or GRU sizes do not match the target stream's
 * model (activations may differ: they are not state); a NULL pointer or a short buffer; an export from a batch whose nnn_batch_fault is
 * set.  Reset and import leave that sticky fault as it is.  The device import checks the records on the device: a list with a bad record
 * is dropped whole (nothing written) and the refusal is reported by the next nnn_batch_synchronize.
 */
/* streams back to freshly-created state (DenoiseState::new, src/features.rs:58-74): the import of an all-zero record */
int nnn_batch_reset_streams(nnn_batch *b, const int *streams, int n);
int nnn_batch_export_streams(nnn_batch *b, const int *streams, int n, void *host_dst, size_t dst_bytes);
int nnn_batch_import_streams(nnn_batch *b, const int *streams, int n, const void *host_src, size_t src_bytes);
/* records in device memory of the batch's device: n * NNN_STREAM_STATE_BYTES bytes at d_dst / d_src, 4-byte aligned */
int nnn_batch_export_streams_device(nnn_batch *b, const int *streams, int n, void *d_dst, void *hip_stream);
int nnn_batch_import_streams_device(nnn_batch *b, const int *streams, int n, const void *d_src, void *hip_stream);

/*
 * Hold and resume.  A batch advances all its streams in lock-step; a server's calls join, leave, mute and go on hold at different times.
 * nnn_batch_hold_streams: from the next processing call on, the listed streams do not take part.  nnn_batch_resume_streams: from the next
 * processing call on they take part again, exactly as if the calls in between had not happened for them -- a stream produces the output
 * and VAD the reference's DenoiseState produces when process_frame is called only on the frames the stream was live for (a state nobody
 * calls does not change, src/denoise.rs:95-116).  The server pattern: reset a slot when a call joins (nnn_batch_reset_streams), hold it
 * when the call goes quiet or on hold, resume it, export it to move it to another batch.
 * While a stream is held, every processing call (process_device / process_host / process_pcm_device / process_pcm_host, every format,
 * interleave and discard_first)
 *   - does not use the stream's input samples: the caller's buffer may hold anything there, NaN included (a host-buffer call may still
 *     copy those bytes to the device; nothing is computed from them);
 *   - writes neither the stream's output samples nor its d_vad entries: those bytes of the caller's buffers are left as they were
 *     (in interleaved PCM: the held channel's samples inside a frame that live channels write);
 *   - leaves the stream's rows of the frame log (nnn_batch_set_frame_log) and its taps (nnn_batch_read_tap) UNSPECIFIED;
 *   - changes nothing for the live streams: their bits are those of the same call with nothing held.
 * Work whose streams are all held is not done: the blocks of a kernel that would serve only held streams return at once (tiles of 64
 * streams in the high-pass and LPC kernels, runs of 16 in the pitch and RNN kernels, of 4 in the transforms and the synthesis), so a host
 * that wants idle slots to be free keeps them together.  A held stream beside live ones in such a run costs what a live one costs.
 * The state of a held stream is its record (the format above), parked in device memory of the batch: NNN_STREAM_STATE_BYTES per stream
 * of the batch, allocated at the first hold and counted in nnn_batch_device_bytes from then on.  That FIRST hold of a batch is not
 * asynchronous: it waits for the batch's work, allocates and synchronises the device (a stall for every batch on it); a real-time host
 * makes an empty hold, nnn_batch_hold_streams(b, NULL, 0), right after creating the batch, which allocates and holds nothing.  From then on both calls are asynchronous and ordered
 * on the batch's own stream like import and reset (after every call made before, before every call made after); both validate first and
 * refuse, changing nothing, on: an index outside [0, n_streams), a repeated index, a NULL list, a stream that is already held (hold) or
 * is not held (resume), and -- hold only, like export -- a batch whose nnn_batch_fault is set.  With no stream held every call behaves,
 * bit for bit, as it does in a batch that never held one.
 * How the other calls meet a held stream:
 *   nnn_batch_export_streams[_device]                  return the parked record (a copy)
 *   nnn_batch_import_streams[_device], reset_streams   replace the parked record; the stream stays held
 *   nnn_batch_reset                                    releases every hold
 *   nnn_batch_clone                                    the clone has the same held set and parked records
 *   nnn_batch_save_state / nnn_batch_load_state        refused while any stream is held (the raw image has no place for parked records)
 *   processing calls with EVERY stream held            succeed, advance the frame counter, launch nothing
 *   host-buffer processing calls                       with any stream held they run in one piece, not in overlapped chunks
 */
int nnn_batch_hold_streams(nnn_batch *b, const int *streams, int n);     /* already held: refused */
int nnn_batch_resume_streams(nnn_batch *b, const int *streams, int n);   /* not held: refused     */
int nnn_batch_num_held(const nnn_batch *b);
int nnn_batch_held_mask(const nnn_batch *b, uint8_t *held, size_t n);    /* held[s] = 0 / 1 for s < n_streams; n >= n_streams */

/*
 * Gain floors: an attenuation limit inside the ordinary call ("never take a band down by more than 18 dB" is a floor of 10^(-18/20)).
 * Every stream has 22 floors F[s][band] in [0, 1], all 0 -- off -- by default.  In every processing call (process_device / process_host /
 * process_pcm_device / process_pcm_host, every format, interleave, discard_first, schedule and back end) the raw network gain of a
 * non-silent frame becomes
 *     g_raw = fmaxf(rnn output, F[s][band])
 * before anything consumes it: the pitch filter (src/features.rs:223-257) sees the floored value, and so do the smoothing
 * g = max(g_raw, 0.6 lastg) and lastg (src/denoise.rs:106-109).
 *   - Silent frames are untouched: the reference applies no gains there and lastg stays.
 *   - VAD and the three GRU states do not depend on gains: they are the unfloored run's, bit for bit.
 *   - By definition an ordinary call under floors F equals nnn_batch_analyze_* -> nnn_batch_network_* -> max(gains, F) ->
 *     nnn_batch_synthesize_*, bit for bit, in audio, VAD and every field of every exported record.
 *   - NNN_TAP_G_RAW and NNN_TAP_G show the floored values.
 * Not affected: nnn_batch_network_* keeps returning the raw, unfloored network output; nnn_batch_synthesize_* applies the caller's gains
 * as given; nnn_batch_vad_*, nnn_batch_analyze_*, the training rows and the rnnoise_* surface are unchanged.
 * Floors are configuration, not state.  They are not in the stream record (NNN_STREAM_STATE_VERSION stays 1) and not in the raw snapshot
 * image (its size is unchanged, old snapshots still load).  How the other calls meet them:
 *   nnn_batch_reset_streams, nnn_batch_import_streams[_device]   the floors stay
 *   nnn_batch_hold_streams / nnn_batch_resume_streams             the floors stay; a held stream's floors may be set, and apply from its
 *                                                                first frame after resume
 *   nnn_batch_reset, nnn_batch_load_state                         the floors stay
 *   nnn_batch_clone                                               the clone has the same floors
 *   nnn_batch_export_streams[_device]                             the record of a floored stream imports anywhere: its lastg is simply >=
 *                                                                the floor
 * nnn_batch_set_gain_floor: floors[i * bands + k] for stream streams[i], bands = 1 (one value for all 22 bands of the stream) or 22; list
 * and values in host memory.  Asynchronous, and ordered exactly as nnn_batch_import_streams is: on the batch's own stream, after every call
 * made before and before every call made after (pipelined calls under nnn_batch_set_inputs_ready included); floors are constant for the
 * whole of a processing call.  The FIRST set of a batch allocates the floor rows (88 bytes per stream, counted in nnn_batch_device_bytes
 * from then on) and may stall the way the first hold does; a real-time host makes an empty set, nnn_batch_set_gain_floor(b, NULL, 0, NULL,
 * 1), right after creating the batch, which allocates the rows and sets nothing.  nnn_batch_get_gain_floor waits for the batch's work and
 * returns 22 values per listed stream (a set with bands = 1 reads back as 22 equal values; a batch that never set a floor: zeros; its list
 * may repeat).  nnn_batch_num_floored: streams with any floor above 0.  A batch that never set a floor, or whose floors are all back to 0,
 * runs exactly the kernels and instructions of a batch without floors.
 * Both calls check everything first and refuse, changing nothing, on: a NULL batch; a NULL list or NULL values with n > 0; n < 0; an
 * index outside [0, n_streams); a repeated index (set); bands other than 1 or 22; a floor that is NaN, below 0 or above 1.
 */
int nnn_batch_set_gain_floor(nnn_batch *b, const int *streams, int n, const float *floors, int bands);
int nnn_batch_get_gain_floor(nnn_batch *b, const int *streams, int n, float *floors /* n * 22 */);
int nnn_batch_num_floored(const nnn_batch *b);

/*
 * Channel link: one gain per band for the channels of a stereo (or four-channel) group, inside the ordinary call.  Streams are interleaved
 * channel groups at the PCM boundary -- stream s is channel s % channels of group s / channels -- and the reference denoises each channel
 * on its own (src/signal.rs:102-104, src/nnnoiseless.rs:318-320), so left and right are attenuated differently from frame to frame and
 * the stereo image wanders.  Linking is the standard cure: compute the gains per channel, apply one common gain per band to all of them.
 * Linking is batch-wide: the streams of link group s / channels are linked, channels = 2 or 4; channels = 1 or NNN_LINK_OFF means off, the
 * default.  For every frame t, link group G and band k, let A be the streams of G that are live (not held) and whose frame t is not
 * silent.  For s in A the raw network gain becomes
 *     g_raw[s][k] = fmaxf( OP over u in A of rnn output[u][k],  F[s][k] )
 * with OP = max for NNN_LINK_MAX (speech-preserving: a band is kept if any channel's network keeps it), min for NNN_LINK_MIN, and F the
 * stream's gain floor (0 without): link first, then each stream's own floor.  The result is formed before anything consumes it: the pitch
 * filter, the smoothing g = max(g_raw, 0.6 lastg), lastg, NNN_TAP_G_RAW / NNN_TAP_G and the frame log all see the linked value.
 *   - A silent frame contributes nothing and receives nothing: no gains are applied there and lastg stays, as in the reference.
 *   - A held stream contributes nothing and receives nothing.
 *   - A group with one member in A is unlinked for that frame.
 *   - VAD and the three GRU states do not depend on gains: they are the unlinked run's, bit for bit.
 *   - By definition an ordinary call under link (channels, mode) and floors F equals nnn_batch_analyze_* -> nnn_batch_network_* -> the
 *     formula above applied to the returned gains with the returned silence flags -> nnn_batch_synthesize_*, bit for bit, in audio, VAD and
 *     every field of every exported record, in every processing call, format, interleave, discard_first, schedule, back end and host
 *     route.  Max and min of finite floats are exact and order-independent: no tolerance enters anywhere.
 * Not affected: nnn_batch_network_* keeps returning the raw, unlinked network output; nnn_batch_synthesize_* applies the caller's gains as
 * given; nnn_batch_vad_*, nnn_batch_analyze_*, the training rows and the rnnoise_* surface are unchanged.
 * The link is configuration, not state: not in the stream record (NNN_STREAM_STATE_VERSION stays 1), not in the snapshot image; it
 * survives nnn_batch_reset, nnn_batch_reset_streams, nnn_batch_import_streams[_device], hold / resume and nnn_batch_load_state, and
 * nnn_batch_clone copies it.  A record exported from a linked batch imports anywhere.  The set call returns at once and is ordered exactly
 * as nnn_batch_set_gain_floor is: after every call made before and before every call made after; the setting is constant for the whole of
 * a processing call.  It allocates nothing.  A batch that never links, or whose link is off again, runs exactly the kernels and
 * instructions of a batch without a link.  A mean is deliberately left out: with silent members its divisor varies, and a sum brings
 * rounding order into a contract that is otherwise exact.
 * nnn_batch_set_channel_link refuses, changing nothing, on: a NULL batch; channels other than 1, 2 or 4; a mode outside the enum;
 * n_streams % channels != 0; frames pending from an nnn_batch_analyze_*; a set nnn_batch_fault.  nnn_batch_get_channel_link (either
 * pointer may be NULL) returns what the next processing call runs under: (1, NNN_LINK_OFF) while off, however it was switched off.
 */
enum nnn_link_mode { NNN_LINK_OFF = 0, NNN_LINK_MAX = 1, NNN_LINK_MIN = 2 };
int nnn_batch_set_channel_link(nnn_batch *b, int channels, int mode);
int nnn_batch_get_channel_link(const nnn_batch *b, int *channels, int *mode);

/*
 * n_frames x process_frame for every stream, buffers resident in device memory.
 *   sample i of frame t of stream s:  d_in [s * stream_stride + t * frame_stride + i]   (floats)
 *                                     d_out[s * stream_stride + t * frame_stride + i]   (may alias d_in)
 *   VAD probability (return value of process_frame): d_vad[t * n_streams + s]           (NULL to skip)
 * hip_stream: a hipStream_t to enqueue on.  NULL does NOT mean HIP's null stream: it means the batch's OWN non-blocking stream, which
 * is not ordered with anything the caller enqueued elsewhere -- a caller that produces d_in on a stream of its own passes that
 * stream (recommended) or synchronises it first.  Asynchronous: the call returns when the work is enqueued.
 */
int nnn_batch_process_device(nnn_batch *b, const float *d_in, float *d_out, float *d_vad, int n_frames,
                             size_t stream_stride, size_t frame_stride, void *hip_stream);
/* Same with host buffers (copies over PCIe, synchronous).  This is the shape of the reference's own interface -- process_frame
 * takes host slices (src/denoise.rs:95) -- and its rate is the bus's, not the kernels': a call of many gap-free frames
 * (frame_stride == 480 * channels) is cut into about sixteen chunks of 1 to 16 frames, chunk i + 1 going up and chunk i - 1 coming back
 * while chunk i is processed (same bits as one piece).  Buffers from nnn_host_alloc (page-locked) are transferred by DMA, both directions at once;
 * any other host memory works through the runtime's staging copies at a fraction of that rate. */
int nnn_batch_process_host(nnn_batch *b, const float *in, float *out, float *vad, int n_frames,
                           size_t stream_stride, size_t frame_stride);
/* Page-locked host memory for the *_host entry points (hipHostMalloc / hipHostFree underneath).  NULL on failure. */
void *nnn_host_alloc(size_t bytes);
void nnn_host_free(void *p);

/*
 * The same with the sample formats and channel interleave of the reference's callers fused into the first and last
 * kernels, so a CLI / DenoiseSignal style per-channel loop is ONE batched call on packed PCM:
 *   NNN_PCM_F32       floats in i16 range, what process_frame itself takes (src/denoise.rs:86-90)
 *   NNN_PCM_I16       int16 in; out = round-half-away(clamp(x, -32768, 32767)) as the CLI's frame writers do
 *                     (src/nnnoiseless.rs:147-177)
 *   NNN_PCM_F32_UNIT  floats in [-1, 1]: in * 32768, out = clamp(x / 32768, -1, 1)  (DenoiseSignal,
 *                     src/signal.rs:95-100 and :123-127)
 * Streams are `channels`-interleaved groups: stream s is channel s % channels of group s / channels, and
 *   sample i of frame t of stream s = buf[(s / channels) * group_stride + t * frame_stride + i * channels + s % channels]
 * in ELEMENTS of the format (a C-channel 16-bit file is one group with frame_stride = 480 * C).  n_streams must be a
 * multiple of channels.  discard_first != 0 reproduces the callers' dropped first frame (src/nnnoiseless.rs:322-330,
 * src/signal.rs:83-87): if the batch has processed no frame since create/reset, frame 0 produces no audio and the
 * call writes n_frames - 1 frames starting at frame position 0 of d_out.  VAD values are written for every frame.
 */
enum nnn_pcm_format { NNN_PCM_F32 = 0, NNN_PCM_I16 = 1, NNN_PCM_F32_UNIT = 2 };
typedef struct nnn_pcm_layout {
    int format;          /* enum nnn_pcm_format */
    int channels;
    int discard_first;
    int reserved;        /* 0 */
    size_t group_stride; /* elements */
    size_t frame_stride; /* elements, >= 480 * channels */
} nnn_pcm_layout;
int nnn_batch_process_pcm_device(nnn_batch *b, const void *d_in, void *d_out, float *d_vad, int n_frames,
                                 const nnn_pcm_layout *layout, void *hip_stream);
int nnn_batch_process_pcm_host(nnn_batch *b, const void *in, void *out, float *vad, int n_frames,
                               const nnn_pcm_layout *layout);
/*
 * Split calls: bring your own network.  The reference exports the two halves of process_frame on their own -- DenoiseFeatures
 * (src/lib.rs:30, src/features.rs:18-275: shift_and_filter_input, compute_frame_features, features(), pitch_filter, the synthesis) and
 * RnnState::compute (src/rnn.rs:343) -- and process_frame (src/denoise.rs:95-116) is the dozen lines that glue them.  These two calls are
 * that seam for a batch: ANALYZE runs everything up to the 42 features for up to nnn_batch_max_group_frames(b) consecutive frames of every
 * stream and hands the rows out; the caller's own network (any size, any framework -- rows are dense f32, a torch model sees [T, S, 42] and
 * returns [T, S, 22]) turns them into 22 band gains per frame; SYNTHESIZE takes those in place of rnn.compute's and runs the rest.
 *   d_features[(t * n_streams + s) * 42 + k]       the RNN input of frame t of stream s (all zero on a silent frame)
 *   d_silence [ t * n_streams + s]                 0 / 1: the frame is digital silence (src/features.rs:160-166)
 *   d_gains   [(t * n_streams + s) * 22 + band]    used as given: no clamp, a NaN goes where it would in the reference
 *   d_vad     [ t * n_streams + s]                 optional (NULL reads as 0): the network's VAD, kept only for NNN_TAP_VAD
 * `layout` describes d_in (analyze) and d_out (synthesize) -- format, channels and strides as nnn_batch_process_pcm_device reads them;
 * discard_first must be 0 for analyze, synthesize honours it.  Rows are 4-byte aligned.
 * Analyze = shift_and_filter_input + compute_frame_features: high-pass, LPC, pitch, both transforms with their band energies, the feature
 * stage.  It advances the input history and biquad state, last_period / last_gain, the cepstral ring and mem_id.  Synthesize, per stream,
 * frame and band on frames that are not silent: pitch_filter on the caller's gains, g = max(g, 0.6 * lastg), lastg = g, the gains
 * interpolated and applied; then frame_synthesis.  On silent frames the caller's gains are ignored, lastg stays, VAD is 0 and the synthesis
 * runs on the unfiltered spectrum, as in the reference.  It advances synthesis_mem and lastg, and the batch's frame count moves here, once
 * per pair.  Neither call touches the three GRU states: a stream may alternate between split calls and ordinary processing calls, and its
 * GRU state is what the last ordinary call left.
 * Protocol: an analyze is followed by a synthesize of the same n_frames before anything else that reads or moves per-stream state.  While
 * frames are pending (nnn_batch_pending_frames != 0) every processing call, a second analyze, hold / resume, export / import /
 * reset_streams, clone and save / load_state refuse -- the error text says that frames are pending -- and change nothing;
 * nnn_batch_reset drops the pending frames; synchronize, fault, the tap reads and destroy work as always.  Refused too, before anything
 * is enqueued: a synthesize with nothing pending or with another n_frames than was analysed, n_frames outside
 * [1, nnn_batch_max_group_frames(b)], a NULL required pointer, a bad layout.
 * The device calls are asynchronous and ordered like processing calls (hip_stream as there: NULL = the batch's own stream); the host
 * variants stage their buffers in one piece and wait.  Held streams (nnn_batch_hold_streams): analyze does not read their input and
 * writes neither their feature rows nor their silence entries, synthesize ignores their gains and writes none of their output; live
 * streams' bits are those of the same calls with nothing held; a pair with every stream held launches nothing and moves the frame count.
 * With taps on, every tap of the pair's last frame reads after the synthesize as after a processing call; NNN_TAP_G_RAW / NNN_TAP_VAD hold
 * the caller's values, NNN_TAP_G the smoothed ones.
 */
int nnn_batch_analyze_device(nnn_batch *b, const void *d_in, float *d_features, int32_t *d_silence, int n_frames,
                             const nnn_pcm_layout *layout, void *hip_stream);
int nnn_batch_synthesize_device(nnn_batch *b, const float *d_gains, const float *d_vad, void *d_out, int n_frames,
                                const nnn_pcm_layout *layout, void *hip_stream);
int nnn_batch_analyze_host(nnn_batch *b, const void *in, float *features, int32_t *silence, int n_frames, const nnn_pcm_layout *layout);
int nnn_batch_synthesize_host(nnn_batch *b, const float *gains, const float *vad, void *out, int n_frames, const nnn_pcm_layout *layout);
int nnn_batch_pending_frames(const nnn_batch *b);   /* frames analysed and not yet synthesised (0 = none) */
/*
 * VAD-only calls: process_frame's second return value without its first.  For hosts that use the voice-activity probability alone --
 * active-speaker detection, endpointing, gating a recorder, picking the conference legs to mix -- the call runs the front of the frame and
 * the network's VAD branch (input_dense, vad_gru, vad_output: src/rnn.rs:353-359) for up to nnn_batch_max_group_frames(b) consecutive
 * frames of every stream, and nothing of the denoiser behind them: no noise or denoise GRU (src/rnn.rs:361-378, about 95 % of the
 * network's multiply-adds), no pitch filter, no gain interpolation, no inverse transform, and neither spectrum through device memory.
 *   d_vad[t * n_streams + s]     the value process_frame returns for frame t of stream s; exactly 0.0f on a silent frame
 * `layout` describes d_in as nnn_batch_process_pcm_device reads it -- all three formats, channels, strides; discard_first must be 0 (there
 * is no audio to drop).  Rows are 4-byte aligned.  A host with more than nnn_batch_max_group_frames(b) frames loops.
 * State.  A VAD call = shift_and_filter_input + compute_frame_features + the VAD branch of RnnState::compute.  It advances the input
 * history and biquad state, last_period / last_gain, the cepstral ring and mem_id, the VAD GRU state (which stays put on silent frames, as
 * in the ordinary path) and the batch's frame count, by n_frames.  It neither reads nor writes synthesis_mem, lastg, or the noise and
 * denoise GRU states: of a stream's record every field is what ordinary processing calls on the same input would leave, except
 * NNN_STREAM_STATE_SYNTHESIS_MEM, _LASTG, _NOISE_GRU and _DENOISE_GRU, which keep their bytes.  Hence:
 *   - a stream may alternate freely between VAD calls and ordinary calls, and its VAD sequence is the all-ordinary run's bit for bit
 *     whatever the mix;
 *   - the AUDIO of the first ordinary frames after VAD-only frames overlap-adds a stale synthesis_mem and runs the two big GRUs from
 *     stale state: that audio is the caller's to discard or fade.
 * Ordering and protocol are a split call's: one frame group, in order on the caller's stream (hip_stream NULL = the batch's own), never
 * pipelined, the device call asynchronous; the host variant stages its input in one piece and waits.  Refused, changing nothing and
 * before anything is enqueued: frames pending from an analyze (the usual text), a NULL d_in, d_vad or layout, a bad layout or
 * discard_first != 0, n_frames outside [1, nnn_batch_max_group_frames(b)], a set nnn_batch_fault.
 * Held streams (nnn_batch_hold_streams): no kernel reads their input (the host variant still copies the caller's whole span to the
 * device, their samples with it), their d_vad entries are left as they were, their parked record does not change; live streams' bits
 * are those of the same call with nothing held; a call with every stream held launches nothing and moves the
 * frame count.  Grouped batches run every model's own VAD branch.  The frame log (nnn_batch_set_frame_log) is not written and its
 * position does not move.  With taps on, NNN_TAP_VAD, _FEATURES, _SILENCE, _PITCH and the pitch chain's taps read as after a processing
 * call; NNN_TAP_X, _P, _G, _G_RAW and _BRANCH are unspecified.
 * The batch is the denoiser's: a VAD-only host still pays its scratch (nnn_batch_device_bytes); nnn_batch_opts.max_group_frames sizes it.
 */
int nnn_batch_vad_device(nnn_batch *b, const void *d_in, float *d_vad, int n_frames, const nnn_pcm_layout *layout, void *hip_stream);
int nnn_batch_vad_host(nnn_batch *b, const void *in, float *vad, int n_frames, const nnn_pcm_layout *layout);
/*
 * Network-only calls: RnnState::compute (src/rnn.rs:343-379) on the caller's feature rows -- the piece of process_frame between
 * nnn_batch_analyze_* and nnn_batch_synthesize_*, on every stream's own resident model.  For hosts that want the built-in (or a converted)
 * network's gains in hand before the synthesis -- an attenuation limit, a per-band floor, a wet/dry blend --, for a bring-your-own-network
 * host that still wants the VAD, and for scoring a model over stored feature rows.  n_frames x compute for every stream:
 *   d_features[(t * n_streams + s) * 42 + k]   dense f32, as nnn_batch_analyze_* writes them
 *   d_silence[t * n_streams + s]               0 / 1 as nnn_batch_analyze_* writes it; NULL = no frame is silent
 *   d_gains[(t * n_streams + s) * 22 + band]   out: the RAW gains, rnn.compute's output (the value of NNN_TAP_G_RAW) -- no lastg smoothing,
 *                                              which is the synthesize half's
 *   d_vad[t * n_streams + s]                   out: the value process_frame returns; NULL = not wanted
 * Rows are 4-byte aligned; the output rows must not overlap the input rows.  On a silent frame process_frame does not call the network
 * (src/denoise.rs:100): the stream's three GRU states stay put, its gains row reads 22 x +0.0f and its VAD +0.0f.
 * State.  The call reads and writes the VAD, noise and denoise GRU states and nothing else: not the input history, synthesis_mem, lastg,
 * the cepstral ring, the pitch state, the frame log, a scratch set or a tap.  The frame count does not move (a fresh batch is still fresh
 * for discard_first afterwards).  analyze -> network -> synthesize with the gains and VAD as they come is an ordinary processing call bit
 * for bit, audio and state.
 * Protocol.  Allowed with frames pending (nnn_batch_pending_frames is unchanged by it) and with none.  It uses no scratch set, so n_frames
 * is any value >= 1, not bounded by nnn_batch_max_group_frames.  Ordering is a state call's: after every call made before it, before every
 * call made after it, on the caller's stream (hip_stream NULL = the batch's own); never pipelined, the device call asynchronous.  The
 * host variant stages its rows in one piece, waits, and copies rows back around held streams.
 * Refused, changing nothing and before anything is enqueued: a NULL batch, d_features or d_gains, n_frames < 1, a misaligned row pointer,
 * a set nnn_batch_fault.
 * Held streams (nnn_batch_hold_streams): their feature and silence entries are not read (they may hold NaN), their gains and VAD entries
 * are left as they were, their parked record does not change; live streams' bits are those of the same call with nothing held; a call with
 * every stream held launches nothing.  Grouped batches run every model on its own streams.
 */
int nnn_batch_network_device(nnn_batch *b, const float *d_features, const int32_t *d_silence, float *d_gains, float *d_vad, int n_frames,
                             void *hip_stream);
int nnn_batch_network_host(nnn_batch *b, const float *features, const int32_t *silence, float *gains, float *vad, int n_frames);
int nnn_batch_synchronize(nnn_batch *b);
/* 1 if a pitch workgroup of an earlier call ran out of patience waiting for the previous frame's result (the frames of a group
 * run side by side below 16 384 streams and hand the last pitch from workgroup to workgroup): the state of the affected streams
 * is invalid from that frame on.  Work items are handed out in the order workgroups start, so the wait cannot deadlock whatever
 * order the hardware dispatches them in; the condition exists as a safety net, and what trips it is wall time (10 s without the
 * predecessor's flag), not a spin count: a predecessor slowed by a shared GPU is waited for.  It is sticky: every later process call and
 * nnn_batch_synchronize fail with it until nnn_batch_reset or nnn_batch_load_state.  Cheap (a read of page-locked host memory the
 * device writes into): callers that synchronise their own stream instead of calling nnn_batch_synchronize can poll it. */
int nnn_batch_fault(const nnn_batch *b);
/* Test hook for the above: withhold the hand-off flag of the frame `frames_ahead` frames from now (negative: off). */
int nnn_batch_debug_withhold_flag(nnn_batch *b, int frames_ahead);
/* Test hook: how a call of n_frames on the batch's own stream would be enqueued as the batch stands now -- its kernel launches in
 * order, the stream of each, the events it waits for and records.  Plans only: launches nothing, changes nothing.  Writes
 * 8 + 17 * nodes integers (an error if `cap` is smaller):
 *   out[0] nodes, [1] frame groups, [2] 1 = spread over the internal streams, [3] schedule (0 seq, 1 lanes, 2 stages), [4] lanes,
 *   [5] where the parameter table is filled: 0 = no launch of its own (the first high-pass launch does it; none in a call with every
 *       stream held), 1 = the caller's stream ahead of everything, 2 = internal stream 0,
 *   [6] 1 = that fill waits for the end of the call two calls back (the table's previous user),
 *   [7] the group whose synthesis event the caller's stream waits for at the end of the call, -1 = none (it ran on that stream);
 *   then per node, in enqueue order: stage (0 hp, 1 pitch, 2 fft_xp, 3 rnn, 4 synth), group, frames of the group, its first frame
 *   within the call, stream (-1 = the caller's, 0..4 = internal), 1 = the stream's first use in the call (it waits for everything
 *   enqueued on the caller's stream before the call), 1 = records its event, number of waits, 3 x (origin, stage, group) -- origin
 *   0 = this call, 1 = the previous call, 2 = the end of the call two calls back (no stage or group); unused entries are -1.
 * A node's event is slot (stage, group mod 16) of a ring the call owns; the previous call has a ring of its own. */
int nnn_batch_debug_schedule(nnn_batch *b, int n_frames, int32_t *out, size_t cap);
/* Test hook: the route nnn_batch_process_pcm_host would take for n_frames of `layout` as the batch stands now (has_vad: a VAD buffer is
 * passed).  Plans only: allocates nothing, copies nothing, changes nothing.
 *   out[0] route: 0 = zero-copy (the kernels work on mapped page-locked host memory), 1 = staged in one piece, 2 = staged in chunks over
 *          two copy streams,
 *   [1] frames per chunk and [2] chunks (n_frames and 1 unless the route is 2), [3] bytes of the layout's bounding span (what is
 *   shipped), [4] bytes of the VAD rows (0 without), [5] offset of the VAD rows behind the span in a host image of both,
 *   [6] 1 = the first frame is dropped (discard_first on a fresh batch), [7] 1 = a one-piece call would copy the VAD rows back around
 *   held streams. */
int nnn_batch_debug_host_plan(nnn_batch *b, int n_frames, const nnn_pcm_layout *layout, int has_vad, int64_t out[8]);

/* Parity taps: intermediate quantities of the most recent frame, copied to the host as
 * [n_streams][len] (float32 or int32, see nnn_tap_info).  Test/diagnostic interface.  Everything inside the pitch kernel
 * (XLP, XCORR1, BEST1, XCORR2C, PITCH_SEARCH), X, P and FEATURES are quantities the kernels keep on
 * chip: they are stored to device memory only after nnn_batch_set_taps(batch, 1) (which also allocates their arrays), and
 * reading them without it is an error.  With taps at 1 the coarse pitch search computes all 147 cross-correlations exactly (the full
 * search, so that XCORR1 is complete); nnn_batch_set_taps(batch, 2) stores the same taps from the certified search production runs take --
 * XCORR1 then holds NaN at every lag the search ruled out and the exact sum at the lags it kept (ref: src/pitch.rs:83-84, 372-405). */
enum nnn_tap {
    NNN_TAP_FILTERED = 0, /* [480] f32  high-passed input (features.rs:97-104)           */
    NNN_TAP_XLP,          /* [864] f32  pitch_buf after pitch_downsample (pitch.rs:448)   */
    NNN_TAP_AC,           /* [5]   f32  windowed autocorrelation                          */
    NNN_TAP_LPC2,         /* [5]   f32  FIR taps                                          */
    NNN_TAP_XCORR1,       /* [147] f32  coarse cross-correlation                          */
    NNN_TAP_BEST1,        /* [2]   i32  best / second best coarse lag                     */
    NNN_TAP_XCORR2C,      /* [10]  f32  fine cross-correlation at 2*best-2..+2, 2*second-2..+2 */
    NNN_TAP_PITCH_SEARCH, /* [1]   i32                                                    */
    NNN_TAP_PITCH,        /* [1]   i32  pitch period after remove_doubling                */
    NNN_TAP_PITCH_GAIN,   /* [1]   f32                                                    */
    NNN_TAP_X,            /* [962] f32  (re,im) x 481, signal spectrum before filtering   */
    NNN_TAP_P,            /* [962] f32  pitch-lagged spectrum                             */
    NNN_TAP_EX, NNN_TAP_EP, NNN_TAP_EXP, /* [22] f32                                      */
    NNN_TAP_FEATURES,     /* [42]  f32                                                    */
    NNN_TAP_SILENCE,      /* [1]   i32                                                    */
    NNN_TAP_G_RAW,        /* [22]  f32  RNN gains                                         */
    NNN_TAP_G,            /* [22]  f32  smoothed gains                                    */
    NNN_TAP_VAD,          /* [1]   f32                                                    */
    NNN_TAP_BRANCH,       /* [1]   i32  bit i < 22: pitch_filter took `exp > g` in band i (src/features.rs:227); bit 22: silent frame */
    NNN_TAP_COUNT
};
int nnn_tap_info(int tap, int *len, int *is_int);
int nnn_batch_set_taps(nnn_batch *b, int on);
int nnn_batch_read_tap(nnn_batch *b, int tap, void *host_dst, size_t dst_bytes);

/* Parity-test record of whole calls (the taps above hold the most recent frame only): from this call on, every processed frame
 * t = 0, 1, ... writes d_log[(t * n_streams + s) * NNN_FRAME_LOG_WORDS + i] for stream s -- word 0: pitch index (int32), word 1: the
 * BRANCH tap (int32), words 2..23: the 22 smoothed band gains (float32; zero on silent frames) -- until `frames` frames have
 * been recorded.  d_log is device memory owned by the caller; NULL or 0 frames switches the record off. */
#define NNN_FRAME_LOG_WORDS 24
int nnn_batch_set_frame_log(nnn_batch *b, void *d_log, size_t frames);

/* Per-kernel timing with HIP events on the launch stream (off by default: it adds two event
 * records per launch).  Times accumulate until read; reading resets them. */
int nnn_batch_set_profiling(nnn_batch *b, int on);
int nnn_batch_num_kernels(void);
const char *nnn_batch_kernel_name(int k);
int nnn_batch_read_kernel_times(nnn_batch *b, double *total_ms, int64_t *launches, int n);

/* Developer instrumentation: 64 shader-clock stamps of block 0 (zeros unless the library was built with
 * -DNNN_STAMPS). */
int nnn_batch_read_stamps(nnn_batch *b, long long *dst64);

/* Retained from the round-1 ABI, no effect: a frame group is five kernel launches now and they are always eager. */
int nnn_batch_set_graph(nnn_batch *b, int on);
/* 1 = calls of 32 frames or more spread their frame groups over the batch's internal HIP streams so that independent stages
 * overlap (default), 0 = every call runs its groups back to back on the caller's stream.  Results are bit-identical. */
int nnn_batch_set_pipeline(nnn_batch *b, int on);
/* The caller's promise about INPUT buffers of the device-pointer entry points: 1 = a call's input is final when the call is
 * made (uploaded and synchronised, or produced by work that has completed) -- not produced by work the caller enqueued on
 * the call's stream after the previous call.  Consecutive pipelined calls on one stream may then overlap at the boundary:
 * the next call's high-pass chain (the only stage that reads the input) starts while the previous call is still draining.
 * Outputs stay ordered on the caller's stream exactly as without it; results are bit-identical.  0 (default): a call's
 * input is read only after everything enqueued on its stream before the call. */
int nnn_batch_set_inputs_ready(nnn_batch *b, int on);
/* Which kernels run the part of a frame behind the pitch analysis.  0: transforms (k_fft_xp) -> RNN (k_rnn / k_rnn_wf) -> synthesis
 * (k_synth), the spectra crossing device memory in between.  1: groups of ONE frame -- the real-time host ticking 10 ms per call, the
 * reference's primary use (src/capi.rs:75-85, src/signal.rs:102-104) -- take the fused back end instead (k_back: one launch, both
 * spectra in registers from their transforms to the inverse transform); 2: every group does.  3 / 4: the fused kernel's RNN stretch
 * alone (16 waves, one layer at a time) replaces the RNN kernels for one-frame / all groups.  -1 (default): by batch size, as
 * measured -- one-frame groups take the fused kernel up to 8192 streams and the RNN stretch alone above that or while other batches
 * tick beside this one ON THE SAME DEVICE; longer groups stay with the layer-pipelined RNN between k_fft_xp and k_synth.
 * Every choice gives the same bits: a stream may change back end from call to call. */
int nnn_batch_set_back_end(nnn_batch *b, int mode);
/* How a pipelined call uses the internal streams: mode 0 = not at all (as set_pipeline(0)); 1 = "lanes": the high-pass
 * chain on its own stream, the other four stages of group k on lane k mod `lanes` (1..4; default 2; lane 0 is the caller's stream);
 * 2 = "stages": one stream per stage, every stream a chain of groups.  Environment: NNN_SCHED=seq|lanes|stages,
 * NNN_LANES=n.  Nobody choosing, the library does: calls of 32 frames or more are pipelined with one lane on batches of up to
 * 16 384 streams (from 8192 streams the high-pass chain of a group waits for the previous group's pitch kernel); bigger batches keep two
 * groups in flight (650 instead of 360 KB of device memory per stream) and run such calls with one stream per stage when they are two groups
 * long, on two lanes when longer (+2-3 % over one stream in order: every kernel of a big batch ends in a tail of half-empty compute
 * units, which another stage's blocks fill).  Shorter calls run in order on the caller's stream. */
int nnn_batch_set_schedule(nnn_batch *b, int mode, int lanes);
/*
 * Environment.  The library reads exactly these variables (the first eight when a batch is created, NNN_NODE_THREADS when a node is,
 * NNN_DEVICE when rnnoise_create / rnnoise_init make their batch of one), every setting gives the same bits, and each is exercised by
 * a test (named on the right).  It sets none: in particular GPU_MAX_HW_QUEUES (real-time hosts ticking several batches side by side
 * want 8) is the host's to export before its first HIP call -- the library only LOOKS whether it is set, to print
 * one note on stderr per process when batches are driven side by side on a device without it (they largely serialise on 4 queues).
 *   NNN_SCHED=seq|lanes|stages   how a call of 32 frames or more uses the batch's internal streams (nnn_batch_set_schedule)   test_hostsim_knobs
 *   NNN_LANES=1..4               lanes of the "lanes" schedule                                                                  test_hostsim_knobs
 *   NNN_HOST_CHUNK=n             host-buffer calls staged, n frames per chunk, 0 = one piece (unset: small calls zero-copy)   test_gpu_parity / test_hostsim_pcm
 *   NNN_RNN_ROWS=16|32           stream rows per RNN workgroup (default by model and batch size)                              test_gpu_parity / test_hostsim_parity
 *   NNN_RNN_WF_MIN_G=n           shortest frame group the layer-pipelined RNN kernel takes                                    test_gpu_parity / test_hostsim_parity
 *   NNN_HP_SPLIT=0|1             the high-pass on one wave per 64 streams or two (default: two for launches of <= 256 tiles)  test_gpu_back_end / test_hostsim_parity
 *   NNN_LPC_HEAD=0|1             one-frame calls: the old part of the LPC sums in the high-pass launch                        test_gpu_back_end / test_hostsim_parity
 *   NNN_PITCH_CHAIN=0|1|2        frames of a group side by side in k_pitch with a flag hand-off, or looped (default by size)  test_gpu_parity / test_hostsim_parity
 *   NNN_NODE_THREADS=0           a node's shards one after the other on the caller's thread                                   test_hostsim_node
 *   NNN_DEVICE=n                 HIP device of the rnnoise_* single-stream surface (default 0)                                 test_gpu_node
 * Earlier rounds' A/B probe knobs are gone but for four that let the tests force a path: NNN_HP_TPB, NNN_X_RIDES, NNN_LPC_WIDE and
 * NNN_LPC_FC.  They exist only in builds with -DNNN_DEV_KNOBS (the tests' interpreter build, scripts/build_variant*.sh); the product
 * does not read them.
 */

/* Diagnostic: the device's activation functions on their own, y[i] = act(x[i]) for n host floats; act 0 = tansig_approx,
 * 1 = sigmoid_approx, 2 = relu (src/util.rs:29-53). */
int nnn_debug_activations(int device, int act, const float *x, float *y, int n);

/* The CPUs local to a HIP device's PCI function in the kernel's cpulist syntax ("0-63,128-191"; /sys/bus/pci/devices/<id>/local_cpulist):
 * where a host thread that feeds that device should run (the node object pins its workers there).  0 and the text, or non-zero. */
int nnn_device_local_cpulist(int device, char *buf, size_t cap);

const char *nnn_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* NNN_BATCH_H */
