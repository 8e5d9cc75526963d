// nnn_train.hip -- training-feature rows (include/nnn_train.h): three batches' worth of feature state behind one handle.
// Needs nnn_batch_core.hip (GrowBuf, grow), lpc_launch / pitch_chained of nnn_batch_launch.hip and pump_chunks / plan_train_chunk of
// nnn_batch_host.hip.
#pragma once

// ---- training-feature rows (include/nnn_train.h) ---------------------------------------------------------------------
struct nnn_train {
    nnn_batch *comb = nullptr, *clean = nullptr, *noise = nullptr;   // three sets of DenoiseFeatures state
    GrowBuf<float> stage;            // device staging of the host entry point: [signal | noise | combined | vad | rows], capacity in frames
    GrowBuf<int32_t> stage_cut;
};

extern "C" void nnn_train_destroy(nnn_train *t)
{
    if (!t) return;
    t->stage.release();
    t->stage_cut.release();
    nnn_batch_destroy(t->comb);
    nnn_batch_destroy(t->clean);
    nnn_batch_destroy(t->noise);
    delete t;
}

extern "C" nnn_train *nnn_train_create(int n_streams, int device)
{
    nnn_train *t = new nnn_train();
    t->comb = nnn_batch_create(nullptr, n_streams, device);
    t->clean = t->comb ? nnn_batch_create(nullptr, n_streams, device) : nullptr;
    t->noise = t->clean ? nnn_batch_create(nullptr, n_streams, device) : nullptr;
    if (!t->noise) {
        std::string keep = g_err;
        nnn_train_destroy(t);
        g_err = keep;
        return nullptr;
    }
    return t;
}

extern "C" int nnn_train_reset(nnn_train *t)
{
    if (!t) return fail("null handle");
    if (int rc = nnn_batch_reset(t->comb)) return rc;
    if (int rc = nnn_batch_reset(t->clean)) return rc;
    return nnn_batch_reset(t->noise);
}

// shift_and_filter_input + the part of compute_frame_features the row needs: everything up to the 42 features for the
// mix, only the band energies of X for the clean and noise states (src/training.rs:129-131 computes their full
// features and says itself that only the transform and band energies are needed; nothing else of them is read).
static void enqueue_feature_group(nnn_batch *h, hipStream_t st, const float *in, size_t stream_stride, size_t frame_stride, int g, bool full)
{
    // `g` consecutive frames (<= GROUP) in scratch sets 0 .. g - 1, the same launches as the denoiser's front: the stateful
    // kernels cover the group in one launch, the per-frame feature stage once per frame
    const Buffers &b = h->b[0];
    const unsigned NT = (unsigned)h->NT, Sp = (unsigned)h->S_pad, ug = (unsigned)g;
    StepParams *sp = h->sp_tab.p;
    StepParams v;
    v.in = (const char *)in;
    v.out = nullptr;
    v.vad = nullptr;
    v.group_stride = (long long)stream_stride * 4;
    v.frame_stride = (long long)frame_stride * 4;
    v.fmt = PCM_F32;
    v.channels = 1;
    v.discard = 0;
    v.slot = (int)(h->frame_count % h->nslot);
    v.n_streams = h->S;
    v.log = nullptr;
    v.log_frames = 0;
    hipLaunchKernelGGL(k_fill_params, dim3(1), dim3(64), 0, st, sp, v, g, h->nslot);
    hipLaunchKernelGGL(k_hp<false>, dim3(NT), dim3(64), 0, st, b, (const StepParams *)sp, g, StepParams{}, 0);
    if (full) {
        const int fc = lpc_launch(h, g);
        if (!fc) hipLaunchKernelGGL(k_lpc_wide, dim3(NT * ug), dim3(320), 0, st, b, (const StepParams *)sp, g);
        else hipLaunchKernelGGL(k_lpc, dim3(NT * ((ug + fc - 1) / fc)), dim3(64), 0, st, b, (const StepParams *)sp, g, fc);
        const int chain = pitch_chained(h, g) ? 1 : 0, seq0 = (int)(h->frame_count & 0x3fffffffu) + 1;
        const unsigned grid = Sp / PK_SPB * (chain ? ug : 1u);
        hipLaunchKernelGGL(k_pitch<false>, dim3(grid), dim3(PK_T), 0, st, b, (const StepParams *)sp, g, chain, seq0, h->tickets, 0, 0);
        if (chain) h->tickets += grid;
        hipLaunchKernelGGL(k_fft_xp, dim3(Sp * ug / FFT_SPB), dim3(64 * FFT_SPB), 0, st, b, (const StepParams *)sp, g);
        hipLaunchKernelGGL(k_features, dim3(NT), dim3(64 * FEAT_WAVES), 0, st, b, g);
    } else {
        hipLaunchKernelGGL(k_fft_x, dim3(Sp * ug / FFT_SPB), dim3(64 * FFT_SPB), 0, st, b, (const StepParams *)sp, g);
    }
    h->frame_count += g;
}

extern "C" int nnn_train_process_device(nnn_train *t, const float *d_signal, const float *d_noise, const float *d_combined,
                                        const int32_t *d_cutoff, const float *d_vad, float *d_rows, int n_frames,
                                        size_t stream_stride, size_t frame_stride, void *hip_stream)
{
    if (!t) return fail("null handle");
    if (n_frames <= 0) return 0;
    if (!d_signal || !d_noise || !d_combined || !d_cutoff || !d_vad || !d_rows) return fail("null buffer");
    nnn_batch *h = t->comb;
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : h->stream;
    const size_t S = (size_t)h->S;
    const int gmax = t->comb->gmax;
    for (int f0 = 0; f0 < n_frames; f0 += gmax) {
        const int g = n_frames - f0 < gmax ? n_frames - f0 : gmax;
        const size_t off = (size_t)f0 * frame_stride;
        enqueue_feature_group(t->comb, st, d_combined + off, stream_stride, frame_stride, g, true);
        enqueue_feature_group(t->clean, st, d_signal + off, stream_stride, frame_stride, g, false);
        enqueue_feature_group(t->noise, st, d_noise + off, stream_stride, frame_stride, g, false);
        hipLaunchKernelGGL(k_train_rows, dim3((unsigned)(h->NT * g)), dim3(64), 0, st, t->comb->b[0], t->clean->b[0], t->noise->b[0],
                           (const int *)d_cutoff + (size_t)f0 * S, d_vad + (size_t)f0 * S, d_rows + (size_t)f0 * S * TRAIN_COLS);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int nnn_train_process_host(nnn_train *t, const float *signal, const float *noise, const float *combined,
                                      const int32_t *cutoff, const float *vad, float *rows, int n_frames)
{
    if (!t) return fail("null handle");
    if (n_frames <= 0) return 0;
    if (!signal || !noise || !combined || !cutoff || !vad || !rows) return fail("null buffer");
    nnn_batch *h = t->comb;
    HIPCHK(hipSetDevice(h->device));
    const size_t S = (size_t)h->S, na = S * n_frames * FRAME, nl = S * n_frames;
    if ((size_t)n_frames > t->stage.cap && grow(h, true, t->stage, (3 * na + nl + nl * TRAIN_COLS) * sizeof(float), (size_t)n_frames, &t->stage_cut, nl * sizeof(int32_t))) return 1;
    float *d = t->stage.p, *dv = d + 3 * na, *dr = dv + nl;
    int32_t *dc = t->stage_cut.p;
    // In chunks like the denoiser's host calls.  Audio is [stream][frame][480] (a chunk: 2-D copies, one row per stream), labels and rows
    // are frame-major (a chunk: one run each).
    const size_t pitch = (size_t)n_frames * FRAME * 4;
    const float *src[3] = {signal, noise, combined};
    return pump_chunks(h, n_frames, plan_train_chunk(h, n_frames),
        [&](int t0, int n) {
            const size_t off = (size_t)t0 * FRAME, lo = (size_t)t0 * S;
            hipError_t e = hipSuccess;
            for (int k = 0; k < 3 && e == hipSuccess; k++)
                e = hipMemcpy2DAsync(d + k * na + off, pitch, src[k] + off, pitch, (size_t)n * FRAME * 4, S, hipMemcpyHostToDevice, h->copy_in);
            if (e == hipSuccess) e = hipMemcpyAsync(dv + lo, vad + lo, n * S * 4, hipMemcpyHostToDevice, h->copy_in);
            if (e == hipSuccess) e = hipMemcpyAsync(dc + lo, cutoff + lo, n * S * 4, hipMemcpyHostToDevice, h->copy_in);
            return e;
        },
        [&](int t0, int n) {
            const size_t off = (size_t)t0 * FRAME, lo = (size_t)t0 * S;
            return nnn_train_process_device(t, d + off, d + na + off, d + 2 * na + off, dc + lo, dv + lo, dr + lo * TRAIN_COLS, n,
                                            (size_t)n_frames * FRAME, FRAME, h->stream);
        },
        [&](int t0, int n) {
            return hipMemcpyAsync(rows + t0 * S * TRAIN_COLS, dr + t0 * S * TRAIN_COLS, n * S * TRAIN_COLS * 4, hipMemcpyDeviceToHost, h->copy_out);
        });
}
