// nnn_batch_vad.hip -- the VAD-only calls (include/nnn_batch.h): process_frame's second return value without its
// first.  nnn_batch_vad_* runs the front of a frame group and the network up to the one-neuron VAD output, and nothing of the denoiser
// behind it: no noise or denoise GRU, no pitch filter, no inverse transform, no spectra through device memory.  The plan (plan_vad), the
// device and host entry points.
// Needs nnn_batch_core.hip (refuse_pending, grow), plan_group / launch_stage / check_layout of nnn_batch_launch.hip, plan_split /
// split_enqueue of nnn_batch_split.hip and plan_host_call / host_vad_back of nnn_batch_host.hip.
#pragma once

// A VAD call is one frame group in order on the caller's stream, like a split call, and is planned like one: the front as plan_group picks
// it, the back end forced unfused with no rider blocks (plan_split) -- here because there is no back end at all.  What it launches:
//   high-pass (+ k_lpc unless k_pitch does the analysis) | k_pitch | k_fft_feat | k_features | k_vad per resident model
// The counters move with the call itself: there is no second half.
struct VadPlan {
    SplitPlan sp;
    static constexpr int n_stages = 4;
    int stages[n_stages];
};
static VadPlan plan_vad(const nnn_batch *h, int n_frames, GroupPlan &p)
{
    VadPlan v;
    v.sp = plan_split(h, n_frames, p);
    const int st[VadPlan::n_stages] = {ST_HP, ST_PITCH, ST_FFT_FEAT, ST_VAD};
    for (int i = 0; i < VadPlan::n_stages; i++) v.stages[i] = st[i];
    return v;
}

static int vad_check(const nnn_batch *h, const char *what, const void *in, const float *vad, int n_frames, const nnn_pcm_layout *L)
{
    if (!h) return fail("null batch");
    if (int rc = refuse_pending(h, what)) return rc;
    if (n_frames < 1 || n_frames > h->gmax)
        return fail("%s: n_frames (%d) outside [1, %d] (nnn_batch_max_group_frames: a VAD call is one frame group)", what, n_frames, h->gmax);
    if (int rc = check_layout(h, L)) return rc;
    if (L->discard_first) return fail("%s: discard_first must be 0 (a VAD call produces no audio to drop)", what);
    if (!in || !vad) return fail("null buffer");
    for (const nnn_batch::ModelGroup &G : h->groups)
        if (!G.vad_rows) return fail("%s: a resident model's VAD branch does not fit k_vad's LDS operand matrices", what);
    return 0;
}

// shift_and_filter_input + compute_frame_features (src/features.rs:97-219) + the VAD branch of RnnState::compute (src/rnn.rs:353-359) for
// n_frames frames of every stream.  Advances what those advance -- input history and biquad, last_period / last_gain, the cepstral ring and
// mem_id, the VAD GRU -- and the frame count; synthesis_mem, lastg and the two big GRUs are neither read nor written.
extern "C" int nnn_batch_vad_device(nnn_batch *h, const void *d_in, float *d_vad, int n_frames, const nnn_pcm_layout *L, void *hip_stream)
{
    if (int rc = vad_check(h, "nnn_batch_vad_device", d_in, d_vad, n_frames, L)) return rc;
    if ((uintptr_t)d_vad & 3) return fail("VAD rows not 4-byte aligned");
    HIPCHK(hipSetDevice(h->device));
    if (int rc = report_fault(h)) return rc;
    const VadPlan vp = plan_vad(h, n_frames, h->plan);
    const long long eb = pcm_elem_bytes(L->format);
    StepParams v0 = {};
    v0.in = (const char *)d_in;
    v0.vad = d_vad;
    v0.group_stride = (long long)L->group_stride * eb;
    v0.frame_stride = (long long)L->frame_stride * eb;
    v0.fmt = L->format;
    v0.channels = L->channels;   // (no frame log: v0.log stays null and the log's position where it was)
    bool enqueued;
    const int rc = split_enqueue(h, vp.sp, v0, hip_stream, enqueued, [&](hipStream_t st, const StepParams *tab) {
        for (int s : vp.stages) launch_stage(h, s, vp.sp.set0, h->plan, tab, st, h->profiling, false);
    });
    if (!enqueued) return rc;
    h->group_count += 1;
    h->frame_count += vp.sp.g;
    h->last_set = vp.sp.set0 + vp.sp.g - 1;
    return rc;
}

// host buffers: the input staged in one piece (the whole span crosses the bus, held streams' samples with it: it is the kernels that do
// not read them), the VAD rows back around held streams, synchronous
extern "C" int nnn_batch_vad_host(nnn_batch *h, const void *in, float *vad, int n_frames, const nnn_pcm_layout *L)
{
    if (int rc = vad_check(h, "nnn_batch_vad_host", in, vad, n_frames, L)) return rc;
    HIPCHK(hipSetDevice(h->device));
    if (int rc = report_fault(h)) return rc;
    const HostPlan p = plan_host_call(h, n_frames, *L, true);
    if (p.span > h->stage.cap || p.vbytes > h->stage_vad.cap) {
        NNN_RT_LOCK;
        if (int rc = quiesce(h)) return rc;
        if (p.span > h->stage.cap && grow(h, false, h->stage, p.span + p.span / 2, p.span + p.span / 2)) return 1;
        if (p.vbytes > h->stage_vad.cap && grow(h, false, h->stage_vad, 2 * p.vbytes, 2 * p.vbytes)) return 1;
    }
    if (hipMemcpyAsync(h->stage.p, in, p.span, hipMemcpyHostToDevice, h->stream) != hipSuccess) return fail("host staging failed: %s", hipGetErrorString(hipGetLastError()));
    const bool idle = h->n_held == h->S;
    int rc = nnn_batch_vad_device(h, h->stage.p, h->stage_vad.p, n_frames, L, h->stream);
    std::vector<char> &tmp = h->stage_host;
    if (tmp.size() < p.vbytes) tmp.resize(p.vbytes);
    if (!rc && !idle && hipMemcpyAsync(tmp.data(), h->stage_vad.p, p.vbytes, hipMemcpyDeviceToHost, h->stream) != hipSuccess)
        rc = fail("copy back failed: %s", hipGetErrorString(hipGetLastError()));
    if (!rc) rc = nnn_batch_synchronize(h);   // (also reports a frame hand-off that never arrived)
    else hipStreamSynchronize(h->stream);
    if (!rc && !idle) host_vad_back(h, vad, (const float *)tmp.data(), n_frames);
    return rc;
}
