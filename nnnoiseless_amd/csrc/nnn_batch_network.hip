// nnn_batch_network.hip -- the network-only calls (include/nnn_batch.h "Network-only calls"): RnnState::compute on
// the caller's feature rows with the stream's own resident model, raw gains and VAD out, and nothing else of the frame.  The piece between
// nnn_batch_analyze_* and nnn_batch_synthesize_*; also usable on its own.  The check, the device and host entry points.
// Needs nnn_batch_core.hip (grow, quiesce, report_fault), call_begin / call_end of nnn_batch_streams.hip, kNetKernel of
// nnn_batch_launch.hip and split_rows_back / host_vad_back of nnn_batch_split.hip / nnn_batch_host.hip.
#pragma once

// A network call has no scratch set, no parameter-table entry and no counter to move: the rows' pointers go to k_net as they are
// (NetIo), so it may be of any length, and it is allowed while frames are pending -- that is its place.  Hence no refuse_pending, no
// plan_split, no split_enqueue: a state call's ordering (call_begin / call_end) around one launch per resident model.
static int network_check(const nnn_batch *h, const char *what, const float *features, const int32_t *silence, const float *gains, const float *vad,
                         int n_frames)
{
    if (!h) return fail("null batch");
    if (!features || !gains) return fail("null buffer");
    if (n_frames < 1) return fail("%s: n_frames (%d) must be at least 1", what, n_frames);
    if (((uintptr_t)features & 3) || ((uintptr_t)silence & 3) || ((uintptr_t)gains & 3) || ((uintptr_t)vad & 3))
        return fail("%s: feature, silence, gain or VAD rows not 4-byte aligned", what);
    return 0;
}

// n_frames x RnnState::compute (src/rnn.rs:343-379) for every stream; a silent frame (src/denoise.rs:100) leaves the stream's states alone
// and reads gains and VAD of +0.  Reads and writes the three GRU states and nothing else of the batch.
extern "C" int nnn_batch_network_device(nnn_batch *h, const float *d_features, const int32_t *d_silence, float *d_gains, float *d_vad, int n_frames,
                                        void *hip_stream)
{
    if (int rc = network_check(h, "nnn_batch_network_device", d_features, d_silence, d_gains, d_vad, n_frames)) return rc;
    HIPCHK(hipSetDevice(h->device));
    if (int rc = report_fault(h)) return rc;
    hipError_t e;
    hipStream_t st = call_begin(h, hip_stream, e);
    if (e != hipSuccess) return fail("could not order the call after the batch's earlier work: %s", hipGetErrorString(hipGetLastError()));
    if (h->n_held < h->S) {   // (every stream held: nothing to launch)
        const NetIo io{d_features, (const int *)d_silence, d_gains, d_vad};
        for (const nnn_batch::ModelGroup &G : h->groups)   // one launch per resident model, as the RNN's
            hipLaunchKernelGGL(kNetKernel, dim3((unsigned)(G.ntiles * (TILE / G.net_rows))), dim3(64 * RNN_WAVES), G.net_lds, st, h->b[0], io, G.plan, G.wq,
                               G.fpar, G.tile0, G.net_rows, n_frames);
    }
    const bool ok = call_end(h, st) == hipSuccess;
    h->prev_pipe = false;
    if (!ok) return fail("stream/event call failed while enqueueing a network call: %s", hipGetErrorString(hipGetLastError()));
    HIPCHK(hipGetLastError());
    return 0;
}

// host buffers: the rows staged in one piece (features | silence in h->stage, gains | vad in h->stage_vad), synchronous; the rows come back
// around held streams
extern "C" int nnn_batch_network_host(nnn_batch *h, const float *features, const int32_t *silence, float *gains, float *vad, int n_frames)
{
    if (int rc = network_check(h, "nnn_batch_network_host", features, silence, gains, vad, n_frames)) return rc;
    const size_t S = (size_t)h->S;
    // (the largest count formed below is the 2 * out_bytes of a grown stage_vad, 184 bytes per row, against the 172 this bounds: with
    // int n_frames and int S neither wraps 64 bits; the check is for a 32-bit size_t)
    if ((size_t)n_frames > SIZE_MAX / (S * (NFEAT + 1) * sizeof(float)))
        return fail("nnn_batch_network_host: %d frames of %d streams: the rows' byte count overflows", n_frames, h->S);
    HIPCHK(hipSetDevice(h->device));
    if (int rc = report_fault(h)) return rc;
    const size_t rows = (size_t)n_frames * S;
    const size_t fbytes = rows * NFEAT * 4, in_bytes = fbytes + (silence ? rows * 4 : 0), gbytes = rows * NB * 4, out_bytes = gbytes + rows * 4;
    if (in_bytes > h->stage.cap || out_bytes > h->stage_vad.cap) {
        NNN_RT_LOCK;
        if (int rc = quiesce(h)) return rc;
        if (in_bytes > h->stage.cap && grow(h, false, h->stage, in_bytes + in_bytes / 2, in_bytes + in_bytes / 2)) return 1;
        if (out_bytes > h->stage_vad.cap && grow(h, false, h->stage_vad, 2 * out_bytes, 2 * out_bytes)) return 1;
    }
    const float *d_feat = (const float *)h->stage.p;
    const int32_t *d_sil = silence ? (const int32_t *)(h->stage.p + fbytes) : nullptr;
    float *d_gains = h->stage_vad.p, *d_vad = vad ? d_gains + rows * NB : nullptr;
    hipError_t err = hipMemcpyAsync(h->stage.p, features, fbytes, hipMemcpyHostToDevice, h->stream);
    if (err == hipSuccess && silence) err = hipMemcpyAsync(h->stage.p + fbytes, silence, rows * 4, hipMemcpyHostToDevice, h->stream);
    if (err != hipSuccess) return fail("host staging failed: %s", hipGetErrorString(err));
    const bool idle = h->n_held == h->S;
    int rc = nnn_batch_network_device(h, d_feat, d_sil, d_gains, d_vad, n_frames, h->stream);
    std::vector<char> &tmp = h->stage_host;
    const size_t back = vad ? out_bytes : gbytes;
    if (tmp.size() < back) tmp.resize(back);
    if (!rc && !idle && hipMemcpyAsync(tmp.data(), d_gains, back, hipMemcpyDeviceToHost, h->stream) != hipSuccess)
        rc = fail("copy back failed: %s", hipGetErrorString(hipGetLastError()));
    if (!rc) rc = nnn_batch_synchronize(h);
    else hipStreamSynchronize(h->stream);
    if (!rc && !idle) {
        split_rows_back(h, gains, tmp.data(), n_frames, NB);
        if (vad) host_vad_back(h, vad, (const float *)(tmp.data() + gbytes), n_frames);
    }
    return rc;
}
