// nnn_batch_debug.hip -- parity taps, stamps, the activation known-answer sweep, per-kernel timing, and the set_* / debug_* switches.
// Needs nnn_batch_core.hip, make_tables and NNN_ALLOC_SETS of nnn_batch_create.hip, plan_call / plan_schedule / check_layout of
// nnn_batch_launch.hip and plan_host_call of nnn_batch_host.hip.
#pragma once

// ---- taps ---------------------------------------------------------------------------------------
struct TapDesc { int len; int is_int; int layout; /* 0 TI, 2 / 4 SM spectrum rows of FSTR (X / P order), 3 hist ring */ int sub_ofs; int sub_len; int needs_taps; };
static int last_slot(const nnn_batch *h) { return h ? (int)((h->frame_count + h->nslot - 1) % h->nslot) : 0; }   // ring slot of the most recent frame
static bool tap_desc(const nnn_batch *h, int tap, TapDesc &d, const void **ptr)
{
    const Buffers *b = h ? &h->b[h->last_set] : nullptr;   // scratch set of the most recent frame
#define TP(field) (b ? (const void *)b->field : nullptr)
    switch (tap) {
    case NNN_TAP_FILTERED: d = {FRAME, 0, 3, 0, FRAME, 0}; *ptr = TP(hist); return true;
    case NNN_TAP_XLP: d = {XLP, 0, 0, 0, XLP, 1}; *ptr = TP(xlp_ti); return true;
    case NNN_TAP_AC: d = {5, 0, 0, last_slot(h) * 10, (h ? h->nslot : 0) * 10, 0}; *ptr = TP(lpc); return true;
    case NNN_TAP_LPC2: d = {5, 0, 0, last_slot(h) * 10 + 5, (h ? h->nslot : 0) * 10, 0}; *ptr = TP(lpc); return true;
    case NNN_TAP_XCORR1: d = {NLAG1, 0, 0, 0, NLAG1, 1}; *ptr = TP(xc1); return true;
    case NNN_TAP_BEST1: d = {2, 1, 0, 0, 2, 1}; *ptr = TP(best1); return true;
    case NNN_TAP_XCORR2C: d = {10, 0, 0, 0, 10, 1}; *ptr = TP(xc2); return true;
    case NNN_TAP_PITCH_SEARCH: d = {1, 1, 0, 0, 1, 1}; *ptr = TP(psearch); return true;
    case NNN_TAP_PITCH: d = {1, 1, 0, 0, 1, 0}; *ptr = TP(pitch); return true;
    case NNN_TAP_PITCH_GAIN: d = {1, 0, 0, 0, 1, 0}; *ptr = TP(pgain); return true;
    case NNN_TAP_X: d = {2 * FREQ, 0, 2, 0, 2 * FREQ, 1}; *ptr = TP(X); return true;   // (the fused back end keeps both spectra in registers)
    case NNN_TAP_P: d = {2 * FREQ, 0, 4, 0, 2 * FREQ, 1}; *ptr = TP(P); return true;   // (layout 4: spectrum_index_p)
    case NNN_TAP_EX: d = {NB, 0, 0, 0, NB, 0}; *ptr = TP(ex); return true;
    case NNN_TAP_EP: d = {NB, 0, 0, 0, NB, 0}; *ptr = TP(ep); return true;
    case NNN_TAP_EXP: d = {NB, 0, 0, 0, NB, 0}; *ptr = TP(exp_); return true;
    case NNN_TAP_FEATURES: d = {NFEAT, 0, 0, 0, NFEAT, 1}; *ptr = TP(feat); return true;
    case NNN_TAP_SILENCE: d = {1, 1, 0, 0, 1, 0}; *ptr = TP(silence); return true;
    case NNN_TAP_G_RAW: d = {NB, 0, 0, 0, NB, 0}; *ptr = TP(g_raw); return true;
    case NNN_TAP_G: d = {NB, 0, 0, 0, NB, 0}; *ptr = TP(g); return true;
    case NNN_TAP_VAD: d = {1, 0, 0, 0, 1, 0}; *ptr = TP(vad); return true;
    case NNN_TAP_BRANCH: d = {1, 1, 0, 0, 1, 0}; *ptr = TP(branch); return true;
    default: return false;
    }
#undef TP
}

extern "C" int nnn_tap_info(int tap, int *len, int *is_int)
{
    TapDesc d;
    const void *p;
    if (!tap_desc(nullptr, tap, d, &p)) return fail("unknown tap %d", tap);
    if (len) *len = d.len;
    if (is_int) *is_int = d.is_int;
    return 0;
}

extern "C" int nnn_batch_set_taps(nnn_batch *h, int on)
{
    if (!h) return fail("null batch");
    if (on && !h->taps_alloc) {   // first use: the tap-only arrays, nset sets like every scratch array
        NNN_RT_LOCK;
        if (int rc = quiesce(h)) return rc;
        NNN_ALLOC_SETS(NNN_TAP_FIELDS);
        h->taps_alloc = true;
        // (dalloc clears the arrays with hipMemset on the null stream, which the batch's own streams do not wait for: at 65 536 streams the
        // clearing of these gigabytes ran into the first frame's tap stores -- found by round 6's certified-search test)
        HIPCHK(hipDeviceSynchronize());
    }
    // (1: every tap, the coarse pitch search as the full search so that all 147 cross-correlations exist; 2: the same taps from the certified
    // search -- NNN_TAP_XCORR1 then holds NaN at the lags it ruled out)
    for (int set = 0; set < h->nset; set++) h->b[set].taps = on == 2 ? 2 : (on != 0);
    return 0;
}

extern "C" int nnn_batch_read_tap(nnn_batch *h, int tap, void *host_dst, size_t dst_bytes)
{
    NNN_RT_LOCK;
    if (!h) return fail("null batch");
    TapDesc d;
    const void *p;
    if (!tap_desc(h, tap, d, &p)) return fail("unknown tap %d", tap);
    if (d.needs_taps && !h->b[0].taps) return fail("tap %d is only stored after nnn_batch_set_taps(batch, 1)", tap);
    if (dst_bytes < (size_t)h->S * d.len * 4) return fail("tap buffer too small");
    if (int rc = quiesce(h)) return rc;
    HIPCHK(hipDeviceSynchronize());
    uint32_t *dst = (uint32_t *)host_dst;
    const size_t Sp = (size_t)h->S_pad;
    if (d.layout == 0) {
        std::vector<uint32_t> tmp(Sp * d.sub_len);
        HIPCHK(hipMemcpy(tmp.data(), p, tmp.size() * 4, hipMemcpyDeviceToHost));
        for (int s = 0; s < h->S; s++)
            for (int i = 0; i < d.len; i++)
                dst[(size_t)s * d.len + i] = tmp[((size_t)(s / TILE) * d.sub_len + d.sub_ofs + i) * TILE + s % TILE];
    } else if (d.layout == 2 || d.layout == 4) {
        std::vector<uint32_t> tmp(Sp * 2 * FSTR);
        HIPCHK(hipMemcpy(tmp.data(), p, tmp.size() * 4, hipMemcpyDeviceToHost));
        // (a spectrum's row holds (bin k, bin 480 - k) pairs in the transforms' lane order: spectrum_index)
        for (int s = 0; s < h->S; s++)
            for (int k = 0; k < FREQ; k++) {
                const size_t at = (size_t)s * 2 * FSTR + 2 * (size_t)(d.layout == 4 ? spectrum_index_p(k) : spectrum_index(k));
                dst[(size_t)s * d.len + 2 * k] = tmp[at];
                dst[(size_t)s * d.len + 2 * k + 1] = tmp[at + 1];
            }
    } else {  // newest frame in the history ring
        const size_t hstr = (size_t)hist_stride(h->nslot);
        std::vector<uint32_t> tmp(Sp * hstr);
        HIPCHK(hipMemcpy(tmp.data(), p, tmp.size() * 4, hipMemcpyDeviceToHost));
        int slot = last_slot(h);  // slot of the most recent frame
        for (int s = 0; s < h->S; s++) memcpy(dst + (size_t)s * FRAME, tmp.data() + (size_t)s * hstr + slot * FRAME, FRAME * 4);
    }
    return 0;
}

extern "C" int nnn_batch_read_stamps(nnn_batch *h, long long *dst64)
{
    NNN_RT_LOCK;
    if (!h) return fail("null batch");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(dst64, h->b[0].stamps, 64 * sizeof(long long), hipMemcpyDeviceToHost));
    return 0;
}

// The device's activation functions on their own: y[i] = act(x[i]) with act 0 = tansig_approx, 1 = sigmoid_approx,
// 2 = relu (ref: src/util.rs:29-53) -- a direct known-answer check for the parity tests.
extern "C" int nnn_debug_activations(int device, int act, const float *x, float *y, int n)
{
    NNN_RT_LOCK;
    if (!x || !y || n < 0 || act < 0 || act > 2) return fail("bad argument");
    HIPCHK(hipSetDevice(device));
    std::vector<float> window, dct, tansig, bin_frac;
    std::vector<float2> tw;
    std::vector<int> bin_band;
    float wnorm;
    make_tables(window, dct, tw, tansig, bin_frac, bin_band, wnorm);
    float *d = nullptr;
    HIPCHK(hipMalloc((void **)&d, (size_t)(2 * n + 256) * sizeof(float)));
    float *dx = d + 256, *dy = dx + n;
    hipError_t e = hipMemcpy(d, tansig.data(), 201 * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dx, x, (size_t)n * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess && n) {
        hipLaunchKernelGGL(k_activation_kat, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t) nullptr, (const float *)d, (const float *)dx, dy, act, n);
        e = hipDeviceSynchronize();
    }
    if (e == hipSuccess) e = hipMemcpy(y, dy, (size_t)n * sizeof(float), hipMemcpyDeviceToHost);
    hipFree(d);
    if (e != hipSuccess) return fail("activation sweep failed: %s", hipGetErrorString(e));
    return 0;
}

// ---- profiling / scheduling switches -------------------------------------------------------------
extern "C" int nnn_batch_set_profiling(nnn_batch *h, int on)
{
    if (!h) return fail("null batch");
    h->profiling = on != 0;
    return 0;
}
extern "C" int nnn_batch_num_kernels(void) { return K_COUNT; }
extern "C" const char *nnn_batch_kernel_name(int k) { return (k >= 0 && k < K_COUNT) ? kKernelNames[k] : ""; }
extern "C" int nnn_batch_read_kernel_times(nnn_batch *h, double *total_ms, int64_t *launches, int n)
{
    if (!h) return fail("null batch");
    for (int k = 0; k < n && k < K_COUNT; k++) {
        total_ms[k] = h->k_ms[k];
        launches[k] = h->k_launches[k];
        h->k_ms[k] = 0;
        h->k_launches[k] = 0;
    }
    return 0;
}
extern "C" int nnn_batch_set_graph(nnn_batch *h, int on)
{
    (void)on;
    if (!h) return fail("null batch");
    return 0;   // kept for callers of the round-1 ABI: a group is six launches now and they are always eager
}
extern "C" int nnn_batch_set_inputs_ready(nnn_batch *h, int on)
{
    if (!h) return fail("null batch");
    h->paths.inputs_ready = on != 0;
    return 0;
}
// Parity-test record of every frame processed from now on (include/nnn_batch.h): device memory for `frames` frames.
extern "C" int nnn_batch_set_frame_log(nnn_batch *h, void *d_log, size_t frames)
{
    if (!h) return fail("null batch");
    h->frame_log = (unsigned *)d_log;
    h->frame_log_left = d_log ? frames : 0;
    return 0;
}
// Test hook: the hand-off flag of the frame `frames_ahead` frames from now (0 = the next one) is never published, so the workgroups
// waiting for it run into their timeout and raise the fault.  A negative value switches the hook off.
extern "C" int nnn_batch_debug_withhold_flag(nnn_batch *h, int frames_ahead)
{
    if (!h) return fail("null batch");
    const int seq = frames_ahead < 0 ? 0 : (int)((h->frame_count + (uint64_t)frames_ahead) & 0x3fffffffu) + 1;
    for (int set = 0; set < h->nset; set++) {
        h->b[set].dbg_withhold = seq;
        h->b[set].handoff_ticks = seq ? 20000000ll : HANDOFF_TICKS;   // the withheld flag is given up on after 0.2 s
    }
    return 0;
}
// Test hook: the schedule a call of n_frames on the batch's own stream would get now, as integers (include/nnn_batch.h).  Plans only.
extern "C" int nnn_batch_debug_schedule(nnn_batch *h, int n_frames, int32_t *out, size_t cap)
{
    if (!h || !out) return fail("null argument");
    if (n_frames < 1) return fail("n_frames must be at least 1");
    CallPlan cp = plan_call(h, n_frames, h->stream);
    if ((size_t)n_frames > h->sp_tab.cap) cp.early_hp = false;   // (the call would first grow its parameter table, which drains the batch: prev_pipe off)
    const Schedule sc = plan_schedule(h, cp);
    constexpr size_t HEAD = 8, PER_NODE = 8 + 3 * MAX_WAITS;
    if (cap < HEAD + PER_NODE * sc.nodes.size()) return fail("schedule buffer too small: %zu entries needed", HEAD + PER_NODE * sc.nodes.size());
    const int32_t head[HEAD] = {(int32_t)sc.nodes.size(), (int32_t)cp.sizes.size(), cp.pipe, cp.sched, cp.lanes, sc.fill, sc.fill_after_done, sc.last_syn};
    memcpy(out, head, sizeof(head));
    out += HEAD;
    for (const Node &n : sc.nodes) {
        const int32_t v[8] = {n.stage, n.group, n.frames, n.first, n.stream, n.first_use, n.record, n.n_waits};
        memcpy(out, v, sizeof(v));
        for (int w = 0; w < MAX_WAITS; w++) {
            const Wait x = w < n.n_waits ? n.waits[w] : Wait{-1, -1, -1};
            out[8 + 3 * w] = x.origin, out[9 + 3 * w] = x.stage, out[10 + 3 * w] = x.group;
        }
        out += PER_NODE;
    }
    return 0;
}
// Test hook: the route a host-buffer call of n_frames would take now (include/nnn_batch.h).  Plans only.
extern "C" int nnn_batch_debug_host_plan(nnn_batch *h, int n_frames, const nnn_pcm_layout *L, int has_vad, int64_t out[8])
{
    if (!h || !out || n_frames < 1) return fail("null argument or no frames");
    if (int rc = check_layout(h, L)) return rc;
    const HostPlan p = plan_host_call(h, n_frames, *L, has_vad != 0);
    const int64_t v[8] = {p.route, p.chunk, p.n_chunks, (int64_t)p.span, (int64_t)p.vbytes, (int64_t)p.vofs, p.drop, p.vad_masked};
    memcpy(out, v, sizeof(v));
    return 0;
}
extern "C" int nnn_batch_set_back_end(nnn_batch *h, int mode)
{
    if (!h) return fail("null batch");
    if (mode < -1 || mode > 4) return fail("unknown back-end mode %d", mode);
    h->paths.back_mode = mode;
    return 0;
}
extern "C" int nnn_batch_set_pipeline(nnn_batch *h, int on)
{
    if (!h) return fail("null batch");
    h->paths.use_pipeline = on != 0;
    return 0;
}
extern "C" int nnn_batch_set_schedule(nnn_batch *h, int mode, int lanes)
{
    if (!h) return fail("null batch");
    if (mode < SCHED_SEQ || mode > SCHED_STAGES) return fail("unknown schedule %d", mode);
    h->paths.sched = mode;
    if (lanes >= 1 && lanes <= NSTREAMS - 1) h->paths.n_lanes = lanes;
    h->paths.sched_auto = false;
    return 0;
}
