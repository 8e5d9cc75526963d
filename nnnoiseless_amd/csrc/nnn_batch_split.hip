// nnn_batch_split.hip -- the split calls (include/nnn_batch.h): one process_frame cut in two at the network.
// nnn_batch_analyze_* runs the front of a frame group and hands the 42 features of every frame to the caller; nnn_batch_synthesize_* takes
// the caller's 22 band gains per frame and runs the rest.  The plan (plan_split), the two enqueue bodies, the device and host entry points.
// Needs nnn_batch_core.hip (refuse_pending, SplitIo, grow), call_begin / call_end of nnn_batch_streams.hip, plan_group / launch_stage /
// check_layout / drain_profile of nnn_batch_launch.hip and plan_host_call / host_frames_back of nnn_batch_host.hip.
#pragma once

// A split call is ONE group of up to gmax frames, its launches in order on the caller's stream: never pipelined, never spread over
// lanes.  Decided before anything is enqueued, like a processing call (plan_call / plan_schedule); reads the batch only, and gives the
// same answer for the analyze and the synthesize of a pair (nothing it reads can change while frames are pending).
struct SplitPlan {
    int g;          // frames
    int set0;       // first scratch set: block (group_count mod depth), which the pair shares -- the group counter moves with the synthesize
    int slot;       // history ring slot of the first frame (frame_count mod nslot: the frame counter moves with the synthesize too)
    bool idle;      // every stream is held: the pair launches nothing and moves the counters
};
// `p`: the front as plan_group picks it (high-pass split, LPC inside k_pitch or behind the high-pass, chained k_pitch, the held forms)
// with the unfused back end and no rider blocks: the spectra must reach device memory, and k_synth must be the kernel that reads them.
static SplitPlan plan_split(const nnn_batch *h, int n_frames, GroupPlan &p)
{
    plan_group(h, n_frames, p);
    p.back = BACK_UNFUSED;
    p.riders = false;
    SplitPlan s;
    s.g = n_frames;
    s.set0 = (int)(h->group_count % h->depth) * h->gmax;
    s.slot = (int)(h->frame_count % h->nslot);
    s.idle = h->n_held == h->S;
    return s;
}

// what both halves check before anything else: the handle, the protocol state, the frame count, the layout
static int split_check(const nnn_batch *h, const char *what, bool analyze, int n_frames, const nnn_pcm_layout *L)
{
    if (!h) return fail("null batch");
    if (analyze) {
        if (int rc = refuse_pending(h, what)) return rc;
    } else {
        if (!h->pending) return fail("%s refused: no frames are pending (nnn_batch_analyze_* comes first)", what);
    }
    if (n_frames < 1 || n_frames > h->gmax)
        return fail("%s: n_frames (%d) outside [1, %d] (nnn_batch_max_group_frames: a split call is one frame group)", what, n_frames, h->gmax);
    if (!analyze && n_frames != h->pending)
        return fail("%s refused: %d frames are pending (analysed and not yet synthesised), the call brings gains for %d", what, h->pending, n_frames);
    if (int rc = check_layout(h, L)) return rc;
    if (analyze && L->discard_first) return fail("%s: discard_first belongs to the synthesize half (the analysis of a dropped frame is still needed)", what);
    return 0;
}

// The common frame of both halves: ordering (call_begin / call_end, the pipelined-call link cleared as a state call does), this call's
// parameter table filled for the frames' ring slots, the launches, the end-of-call event.  `v0`: the call's parameters but for the slot.
// `enqueued`: the call got as far as its launches (from then on the caller's bookkeeping follows the device, whatever is reported).
template <class Launches> static int split_enqueue(nnn_batch *h, const SplitPlan &sp, StepParams v0, void *hip_stream, bool &enqueued, Launches launches)
{
    enqueued = false;
    if ((size_t)sp.g > h->sp_tab.cap) {
        const size_t cap = 64;   // (a group is at most 24 frames)
        if (int rc = grow(h, true, h->sp_tab, 2 * cap * sizeof(StepParams), cap)) return rc;
    }
    hipError_t e;
    hipStream_t st = call_begin(h, hip_stream, e);
    if (e != hipSuccess) return fail("could not order the call after the batch's earlier work: %s", hipGetErrorString(hipGetLastError()));
    enqueued = true;
    v0.slot = sp.slot;
    v0.n_streams = h->S;
    h->call_count += 1;
    const int par = (int)(h->call_count & 1);
    StepParams *const tab = h->sp_tab.p + (size_t)par * h->sp_tab.cap;
    if (!sp.idle) {
        hipLaunchKernelGGL(k_fill_params, dim3(1), dim3(64), 0, st, tab, v0, sp.g, h->nslot);
        launches(st, (const StepParams *)tab);
    }
    bool ok = hipEventRecord(h->ev_done[par], st) == hipSuccess;
    h->have_done[par] = true;
    ok &= call_end(h, st) == hipSuccess;
    h->prev_pipe = false;
    if (!ok) return fail("stream/event call failed while enqueueing a split call: %s", hipGetErrorString(hipGetLastError()));
    HIPCHK(hipGetLastError());
    if (h->profiling) {
        HIPCHK(hipStreamSynchronize(st));
        return drain_profile(h);
    }
    return 0;
}

extern "C" int nnn_batch_pending_frames(const nnn_batch *h) { return h ? h->pending : 0; }

// shift_and_filter_input + compute_frame_features (src/features.rs:97-219) for n_frames frames of every stream: high-pass, LPC, pitch,
// both transforms with their band energies, the feature stage; the rows out.  Leaves X, P, ex, ep, exp, silence and pitch in the group's
// scratch sets for the synthesize.
extern "C" int nnn_batch_analyze_device(nnn_batch *h, const void *d_in, float *d_features, int32_t *d_silence, int n_frames,
                                        const nnn_pcm_layout *L, void *hip_stream)
{
    if (int rc = split_check(h, "nnn_batch_analyze_device", true, n_frames, L)) return rc;
    if (!d_in || !d_features || !d_silence) return fail("null buffer");
    if (((uintptr_t)d_features & 3) || ((uintptr_t)d_silence & 3)) return fail("feature or silence rows not 4-byte aligned");
    HIPCHK(hipSetDevice(h->device));
    if (int rc = report_fault(h)) return rc;
    const SplitPlan sp = plan_split(h, n_frames, h->plan);
    const long long eb = pcm_elem_bytes(L->format);
    StepParams v0 = {};
    v0.in = (const char *)d_in;
    v0.group_stride = (long long)L->group_stride * eb;
    v0.frame_stride = (long long)L->frame_stride * eb;
    v0.fmt = L->format;
    v0.channels = L->channels;
    SplitIo io;
    io.features = d_features;
    io.silence = (int *)d_silence;
    bool enqueued;
    const int rc = split_enqueue(h, sp, v0, hip_stream, enqueued, [&](hipStream_t st, const StepParams *tab) {
        for (int s : {(int)ST_HP, (int)ST_PITCH, (int)ST_FFT, (int)ST_FEAT})
            launch_stage(h, s, sp.set0, h->plan, tab, st, h->profiling, false, nullptr, 0, &io);
    });
    if (!enqueued) return rc;
    h->pending = sp.g;
    h->pending_set0 = sp.set0;
    h->pending_slot = sp.slot;
    return rc;
}

// The rest of process_frame (src/denoise.rs:103-114) with the caller's gains in place of rnn.compute: pitch_filter on the raw gains, the
// lastg smoothing, gain interpolation, frame_synthesis.  Moves the frame counter, once per pair.
extern "C" int nnn_batch_synthesize_device(nnn_batch *h, const float *d_gains, const float *d_vad, void *d_out, int n_frames,
                                           const nnn_pcm_layout *L, void *hip_stream)
{
    if (int rc = split_check(h, "nnn_batch_synthesize_device", false, n_frames, L)) return rc;
    if (!d_gains || !d_out) return fail("null buffer");
    if (((uintptr_t)d_gains & 3) || ((uintptr_t)d_vad & 3)) return fail("gain or VAD rows not 4-byte aligned");
    HIPCHK(hipSetDevice(h->device));
    if (int rc = report_fault(h)) return rc;
    const SplitPlan sp = plan_split(h, n_frames, h->plan);
    if (sp.set0 != h->pending_set0 || sp.slot != h->pending_slot) return fail("internal: the pending frames' scratch sets or ring slot moved");
    const long long eb = pcm_elem_bytes(L->format);
    const bool plain_out = L->format == NNN_PCM_F32 && L->channels == 1;
    StepParams v0 = {};
    v0.out = (char *)d_out;
    v0.group_stride = (long long)L->group_stride * eb;
    v0.frame_stride = (long long)L->frame_stride * eb;
    v0.fmt = L->format;
    v0.channels = L->channels;
    v0.discard = (L->discard_first && h->frame_count == 0) ? 1 : 0;
    v0.log = h->frame_log_left ? h->frame_log : nullptr;
    v0.log_frames = (int)(h->frame_log_left < (size_t)n_frames ? h->frame_log_left : (size_t)n_frames);
    if (v0.log) {
        h->frame_log += (size_t)v0.log_frames * h->S * FRAME_LOG_WORDS;
        h->frame_log_left -= (size_t)v0.log_frames;
    }
    SplitIo io;
    io.gains = d_gains;
    io.vad = d_vad;
    bool enqueued;
    const int rc = split_enqueue(h, sp, v0, hip_stream, enqueued, [&](hipStream_t st, const StepParams *tab) {
        launch_stage(h, ST_GAINS, sp.set0, h->plan, tab, st, h->profiling, plain_out, nullptr, 0, &io);
        launch_stage(h, ST_SYN, sp.set0, h->plan, tab, st, h->profiling, plain_out);
    });
    if (!enqueued) return rc;
    h->pending = 0;
    h->group_count += 1;
    h->frame_count += sp.g;
    h->last_set = sp.set0 + sp.g - 1;
    return rc;
}

// ---- host buffers: staged in one piece, synchronous ------------------------------------------------------------------------------
// rows of `w` 32-bit words per (frame, stream) back into the caller's buffer, a held stream's left as they were
static void split_rows_back(const nnn_batch *h, void *dst, const void *src, int n_frames, size_t w)
{
    const size_t S = (size_t)h->S;
    if (!h->n_held) { memcpy(dst, src, (size_t)n_frames * S * w * 4); return; }
    for (size_t r = 0; r < (size_t)n_frames * S; r++)
        if (!h->held[r % S]) memcpy((char *)dst + r * w * 4, (const char *)src + r * w * 4, w * 4);
}
// the device staging of a host call: the audio span in h->stage, `words` 32-bit words per (frame, stream) of rows in h->split_stage
static int split_host_stage(nnn_batch *h, size_t span, int n_frames)
{
    if (span > h->stage.cap || (size_t)n_frames > h->split_stage.cap) {
        NNN_RT_LOCK;
        if (int rc = quiesce(h)) return rc;
        if (span > h->stage.cap && grow(h, false, h->stage, span + span / 2, span + span / 2)) return 1;
        const size_t cap = (size_t)h->gmax;   // (rows: whatever a group can be, once)
        if ((size_t)n_frames > h->split_stage.cap && grow(h, false, h->split_stage, cap * h->S * (NFEAT + 1) * sizeof(float), cap)) return 1;
    }
    return 0;
}

extern "C" int nnn_batch_analyze_host(nnn_batch *h, const void *in, float *features, int32_t *silence, int n_frames, const nnn_pcm_layout *L)
{
    if (int rc = split_check(h, "nnn_batch_analyze_host", true, n_frames, L)) return rc;
    if (!in || !features || !silence) return fail("null buffer");
    HIPCHK(hipSetDevice(h->device));
    const HostPlan p = plan_host_call(h, n_frames, *L, false);
    if (int rc = split_host_stage(h, p.span, n_frames)) return rc;
    const size_t rows = (size_t)n_frames * h->S;
    float *d_feat = h->split_stage.p;
    int32_t *d_sil = (int32_t *)(d_feat + rows * NFEAT);
    if (hipMemcpyAsync(h->stage.p, in, p.span, hipMemcpyHostToDevice, h->stream) != hipSuccess) return fail("host staging failed: %s", hipGetErrorString(hipGetLastError()));
    int rc = nnn_batch_analyze_device(h, h->stage.p, d_feat, d_sil, n_frames, L, h->stream);
    std::vector<char> &tmp = h->stage_host;
    if (tmp.size() < rows * (NFEAT + 1) * 4) tmp.resize(rows * (NFEAT + 1) * 4);
    if (!rc && hipMemcpyAsync(tmp.data(), d_feat, rows * (NFEAT + 1) * 4, hipMemcpyDeviceToHost, h->stream) != hipSuccess)
        rc = fail("copy back failed: %s", hipGetErrorString(hipGetLastError()));
    if (!rc) rc = nnn_batch_synchronize(h);   // (also reports a frame hand-off that never arrived)
    else hipStreamSynchronize(h->stream);
    if (!rc && h->n_held < h->S) {
        split_rows_back(h, features, tmp.data(), n_frames, NFEAT);
        split_rows_back(h, silence, tmp.data() + rows * NFEAT * 4, n_frames, 1);
    }
    return rc;
}

extern "C" int nnn_batch_synthesize_host(nnn_batch *h, const float *gains, const float *vad, void *out, int n_frames, const nnn_pcm_layout *L)
{
    if (int rc = split_check(h, "nnn_batch_synthesize_host", false, n_frames, L)) return rc;
    if (!gains || !out) return fail("null buffer");
    HIPCHK(hipSetDevice(h->device));
    const HostPlan p = plan_host_call(h, n_frames, *L, false);
    if (int rc = split_host_stage(h, p.span, n_frames)) return rc;
    const size_t rows = (size_t)n_frames * h->S;
    float *d_gains = h->split_stage.p, *d_vad = vad ? d_gains + rows * NB : nullptr;
    hipError_t err = hipMemcpyAsync(d_gains, gains, rows * NB * 4, hipMemcpyHostToDevice, h->stream);
    if (err == hipSuccess && vad) err = hipMemcpyAsync(d_vad, vad, rows * 4, hipMemcpyHostToDevice, h->stream);
    if (err != hipSuccess) return fail("host staging failed: %s", hipGetErrorString(err));
    const bool idle = h->n_held == h->S;
    int rc = nnn_batch_synthesize_device(h, d_gains, d_vad, h->stage.p, n_frames, L, h->stream);
    std::vector<char> &tmp = h->stage_host;
    if (tmp.size() < p.span) tmp.resize(p.span);
    // `out` may be strided: bring the span back and copy only the frames the call wrote, around held streams (host_frames_back)
    if (!rc && !idle && hipMemcpyAsync(tmp.data(), h->stage.p, p.span, hipMemcpyDeviceToHost, h->stream) != hipSuccess)
        rc = fail("copy back failed: %s", hipGetErrorString(hipGetLastError()));
    if (!rc) rc = nnn_batch_synchronize(h);
    else hipStreamSynchronize(h->stream);
    if (!rc && !idle) host_frames_back(h, (char *)out, tmp.data(), L, n_frames - p.drop);
    return rc;
}
