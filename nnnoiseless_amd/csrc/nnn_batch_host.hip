// nnn_batch_host.hip -- host-buffer calls: the route plan (plan_host_call, plan_train_chunk), the chunk pump and the three routes,
// the copies back that leave held streams alone, and the two *_host entry points.
// Needs nnn_batch_core.hip (grow, quiesce) and check_layout of nnn_batch_launch.hip; the routes run through the public *_device calls.
#pragma once

constexpr size_t ZC_MAX = (size_t)1 << 20;                 // host-buffer calls up to this many bytes run on mapped host memory (plan_host_call)
constexpr size_t HOST_CHUNK_MIN_BYTES = (size_t)1 << 20;   // a chunk of a host-buffer call is at least this long

// How a host-buffer call crosses the bus (plan_host_call, which reads the batch only; process_host_span runs it,
// nnn_batch_debug_host_plan shows it to the tests)
enum HostRoute { HOST_ZERO_COPY = 0, HOST_ONE_PIECE = 1, HOST_CHUNKED = 2 };
struct HostPlan {
    int route;
    int chunk, n_chunks;   // frames per chunk and chunks (one chunk of n_frames unless HOST_CHUNKED)
    size_t span;           // bytes of the bounding span of the (possibly strided) layout: what is shipped
    size_t vbytes;         // bytes of the VAD rows, 0 = not asked for
    size_t vofs;           // where the VAD rows sit behind the span in a host image of both (zero-copy; one piece with vad_masked)
    int drop;              // 1 = the first frame produces no audio (discard_first on a fresh batch)
    bool vad_masked;       // one piece: the VAD rows come back through the host image too, a held stream's entries are not copied
};
static HostPlan plan_host_call(const nnn_batch *h, int n_frames, const nnn_pcm_layout &L, bool has_vad)
{
    const size_t e = (size_t)pcm_elem_bytes(L.format), groups = (size_t)(h->S / L.channels), fr = (size_t)FRAME * L.channels * e;
    HostPlan p;
    p.route = HOST_ZERO_COPY, p.chunk = n_frames, p.n_chunks = 1;   // (until the rules below say otherwise)
    p.span = (groups - 1) * L.group_stride * e + (size_t)(n_frames - 1) * L.frame_stride * e + fr;
    p.vbytes = has_vad ? (size_t)n_frames * h->S * sizeof(float) : 0;
    p.vofs = (p.span + 15) / 16 * 16;
    p.drop = (L.discard_first && h->frame_count == 0) ? 1 : 0;
    p.vad_masked = has_vad && h->n_held > 0;
    // Small calls -- the RNNoise C ABI's state is a batch of one, a frame per call -- have nothing to overlap and pay for every runtime call they
    // make: two or three staged copies of a few kilobytes cost more than the three kernels between them.  Up to ZC_MAX bytes the kernels work on
    // page-locked host memory directly (the input read over the link by the first kernel, audio and VAD written over it by the last): one
    // memcpy in, one wait, one memcpy out.  Same kernels, same bits.  An explicit NNN_HOST_CHUNK always takes the staged routes.
    if (h->paths.host_chunk < 0 && p.span + p.vbytes + 16 <= ZC_MAX) return p;
    // Chunk length.  The first upload and the last download are not overlapped, so a call wants many chunks (about sixteen); the kernels
    // want groups of a few frames on small batches (a 4096-stream batch runs 4-frame groups at 0.8 of its 24-frame rate, a 65 536-stream
    // batch is within 15 % of its best on one-frame groups -- and still twice as fast as the bus).  Measured with page-locked buffers
    // against the link's own both-ways peak of 97 GB/s (profiles/r5_host_boundary.txt): 4096 streams x 48 frames f32 at 4 / 8 / 16-frame
    // chunks 84 / 79 / 69 GB/s both ways (round 4 used 8), 65 536 x 24 at 1 / 2 / 4 / 8: 90 / 87 / 81 / 71 (int16: 81 / 84 / 77 / 66).
    // Chunks under a megabyte are not worth their launches.
    int chunk = h->paths.host_chunk;
    if (chunk < 0) {
        constexpr int HC = 16;   // longest chunk
        chunk = n_frames / 16;
        if (chunk < 1) chunk = 1;
        if (h->S_pad <= 8192 && chunk < 4) chunk = 4;
        if (chunk > HC) chunk = HC;
        while (chunk < HC && (size_t)chunk * fr * groups < HOST_CHUNK_MIN_BYTES) chunk *= 2;
        if ((size_t)chunk * fr * groups < HOST_CHUNK_MIN_BYTES) chunk = 0;
    }
    // (the chunks' downloads go straight into the caller's buffers, whole rows of every stream: with streams held the call takes the
    // one-piece route, whose copy back leaves out what a held stream owns)
    const bool chunked = chunk > 0 && n_frames > chunk && L.frame_stride == (size_t)FRAME * L.channels && !h->n_held;
    p.route = chunked ? HOST_CHUNKED : HOST_ONE_PIECE;
    if (chunked) p.chunk = chunk, p.n_chunks = (n_frames + chunk - 1) / chunk;
    return p;
}
// The training host call's chunk length (nnn_train_process_host): 16 frames (tuned on the bus, not tied to the kernels' group length) for
// calls of more than two such chunks that are worth their launches, otherwise one piece; NNN_HOST_CHUNK (tests) overrides it.
static int plan_train_chunk(const nnn_batch *h, int n_frames)
{
    constexpr int HC = 16;
    if (const int hc = h->paths.host_chunk; hc >= 0) return hc > 0 && hc < n_frames ? hc : n_frames;
    return n_frames > 2 * HC && (size_t)h->S * HC * FRAME * 4 >= HOST_CHUNK_MIN_BYTES ? HC : n_frames;
}

// Chunked host calls (the denoiser's and the training rows'): chunk i + 1 crosses the bus on one copy stream while chunk i is processed on
// the batch's stream and chunk i - 1 returns on another (PCIe is full duplex).  upload(t0, n) enqueues n frames from t0 on copy_in,
// run(t0, n) processes them on h->stream, download(t0, n) enqueues what comes back on copy_out.  Nothing more is enqueued after the
// first error; all three streams are drained either way.  The copy streams and an event pair per chunk are made on first use.
template <class Up, class Run, class Down> static int pump_chunks(nnn_batch *h, int n_frames, int C, Up upload, Run run, Down download)
{
    const int nch = (n_frames + C - 1) / C;
    if (!h->copy_in || (int)h->ev_up.size() < nch) {
        NNN_RT_LOCK;
        if (!h->copy_in) {
            HIPCHK(hipStreamCreateWithFlags(&h->copy_in, hipStreamNonBlocking));
            HIPCHK(hipStreamCreateWithFlags(&h->copy_out, hipStreamNonBlocking));
        }
        while ((int)h->ev_up.size() < nch) {
            hipEvent_t a, b;
            HIPCHK(hipEventCreateWithFlags(&a, hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&b, hipEventDisableTiming));
            h->ev_up.push_back(a);
            h->ev_run.push_back(b);
        }
    }
    // (the previous call ended with every stream drained, so the staging is free)
    int rc = 0;
    hipError_t err = hipSuccess;
    for (int i = 0; i < nch && !rc && err == hipSuccess; i++) {
        const int t0 = i * C, n = t0 + C < n_frames ? C : n_frames - t0;
        err = upload(t0, n);
        if (err == hipSuccess) err = hipEventRecord(h->ev_up[i], h->copy_in);
        if (err == hipSuccess) err = hipStreamWaitEvent(h->stream, h->ev_up[i], 0);
        if (err != hipSuccess) break;
        rc = run(t0, n);
        if (rc) break;
        err = hipEventRecord(h->ev_run[i], h->stream);
        if (err == hipSuccess) err = hipStreamWaitEvent(h->copy_out, h->ev_run[i], 0);
        if (err == hipSuccess) err = download(t0, n);
    }
    const hipError_t e1 = hipStreamSynchronize(h->copy_in), e2 = hipStreamSynchronize(h->stream), e3 = hipStreamSynchronize(h->copy_out);
    if (rc) return rc;
    if (err == hipSuccess) err = e1 != hipSuccess ? e1 : (e2 != hipSuccess ? e2 : e3);
    if (err != hipSuccess) return fail("host transfer failed: %s", hipGetErrorString(err));
    return 0;
}

// A long host-buffer call with gap-free frames runs in chunks of p.chunk frames, every transfer a 2-D copy of groups x chunk-bytes
// straight between the caller's buffers and the device staging (DMA when they are page-locked -- nnn_host_alloc -- and staged by the
// runtime when not).  The device staging has the layout of the host buffers.
static int process_host_chunked(nnn_batch *h, const char *in, char *out, float *vad, int n_frames, const nnn_pcm_layout *L, const HostPlan &p)
{
    const size_t e = (size_t)pcm_elem_bytes(L->format), groups = (size_t)(h->S / L->channels), fr = (size_t)FRAME * L->channels * e;
    const size_t pitch = groups > 1 ? L->group_stride * e : (size_t)n_frames * fr, S = (size_t)h->S;
    char *const d = h->stage.p;
    float *const dv = vad ? h->stage_vad.p : nullptr;
    // with a dropped first frame every output sits one frame earlier than its input: a chunk of frames t0 .. t0 + n - 1 then writes frames
    // t0 - 1 .. t0 + n - 2, in place behind inputs that the chunk before has consumed (same stream), and returns those
    auto out0 = [&](int t0) { return (size_t)(t0 ? t0 - p.drop : 0); };
    const int rc = pump_chunks(h, n_frames, p.chunk,
        [&](int t0, int n) { return hipMemcpy2DAsync(d + t0 * fr, pitch, in + t0 * fr, pitch, n * fr, groups, hipMemcpyHostToDevice, h->copy_in); },
        [&](int t0, int n) { return nnn_batch_process_pcm_device(h, d + t0 * fr, d + out0(t0) * fr, dv ? dv + t0 * S : nullptr, n, L, h->stream); },
        [&](int t0, int n) {
            const size_t o0 = out0(t0), o1 = (size_t)(t0 + n - p.drop);
            hipError_t err = hipSuccess;
            if (o1 > o0) err = hipMemcpy2DAsync(out + o0 * fr, pitch, d + o0 * fr, pitch, (o1 - o0) * fr, groups, hipMemcpyDeviceToHost, h->copy_out);
            if (err == hipSuccess && vad) err = hipMemcpyAsync(vad + t0 * S, dv + t0 * S, n * S * sizeof(float), hipMemcpyDeviceToHost, h->copy_out);
            return err;
        });
    return rc ? rc : nnn_batch_synchronize(h);   // (also reports a frame hand-off that never arrived)
}

// The copies back of the host-buffer calls: the frames the call wrote, from a host image `src` of the device buffer into the caller's.
// A held stream's samples and VAD entries are not the call's to write (nnn_batch_hold_streams): the caller's bytes stay as they were,
// per channel where held and live channels share an interleaved group.
static void host_frames_back(const nnn_batch *h, char *out, const char *src, const nnn_pcm_layout *L, int n_out)
{
    const size_t e = (size_t)pcm_elem_bytes(L->format), ch = (size_t)L->channels, groups = (size_t)h->S / ch, fr = (size_t)FRAME * ch * e;
    for (size_t g = 0; g < groups; g++) {
        size_t n_live = ch;
        for (size_t c = 0; c < ch && h->n_held > 0; c++) n_live -= h->held[g * ch + c] ? 1 : 0;
        if (!n_live) continue;
        for (int t = 0; t < n_out; t++) {
            const size_t o = g * L->group_stride * e + (size_t)t * L->frame_stride * e;
            if (n_live == ch) { memcpy(out + o, src + o, fr); continue; }
            for (size_t c = 0; c < ch; c++)
                if (!h->held[g * ch + c])
                    for (size_t i = 0; i < (size_t)FRAME; i++) memcpy(out + o + (i * ch + c) * e, src + o + (i * ch + c) * e, e);
        }
    }
}
static void host_vad_back(const nnn_batch *h, float *vad, const float *src, int n_frames)
{
    if (!h->n_held) { memcpy(vad, src, (size_t)n_frames * h->S * sizeof(float)); return; }
    for (int t = 0; t < n_frames; t++)
        for (int s = 0; s < h->S; s++)
            if (!h->held[(size_t)s]) vad[(size_t)t * h->S + s] = src[(size_t)t * h->S + s];
}

// Host buffers: ship the bounding span of the (possibly strided) layout, run, bring the written frames back, by plan_host_call's route.
static int process_host_span(nnn_batch *h, const void *in, void *out, float *vad, int n_frames, const nnn_pcm_layout *L)
{
    struct InHostCall {   // (nnn_batch::host_call, until the call returns)
        nnn_batch *h;
        ~InHostCall() { h->host_call = false; }
    } in_host_call{h};
    h->host_call = true;
    HIPCHK(hipSetDevice(h->device));
    const HostPlan p = plan_host_call(h, n_frames, *L, vad != nullptr);
    if (p.route == HOST_ZERO_COPY) {
        if (!h->zc_dev) {   // (first use, or an earlier one that failed half-way: zc_dev is set last, and is what says that both exist)
            NNN_RT_LOCK;
            if (int rc = grow(h, true, h->zc_host, ZC_MAX, ZC_MAX)) return rc;
            HIPCHK(hipHostGetDevicePointer((void **)&h->zc_dev, h->zc_host.p, 0));
        }
        memcpy(h->zc_host.p, in, p.span);
        int rc = nnn_batch_process_pcm_device(h, h->zc_dev, h->zc_dev, vad ? (float *)(h->zc_dev + p.vofs) : nullptr, n_frames, L, h->stream);
        if (!rc) rc = nnn_batch_synchronize(h);   // (also reports a frame hand-off that never arrived)
        else hipStreamSynchronize(h->stream);
        if (!rc) {
            host_frames_back(h, (char *)out, h->zc_host.p, L, n_frames - p.drop);
            if (vad) host_vad_back(h, vad, (const float *)(h->zc_host.p + p.vofs), n_frames);
        }
        return rc;
    }
    if (p.span > h->stage.cap || p.vbytes > h->stage_vad.cap) {   // the staging grows by half as much again as is asked for (the VAD rows: twice)
        NNN_RT_LOCK;   // (one lock and one drain for both)
        if (int rc = quiesce(h)) return rc;
        if (p.span > h->stage.cap && grow(h, false, h->stage, p.span + p.span / 2, p.span + p.span / 2)) return 1;
        if (p.vbytes > h->stage_vad.cap && grow(h, false, h->stage_vad, 2 * p.vbytes, 2 * p.vbytes)) return 1;
    }
    if (p.route == HOST_CHUNKED) return process_host_chunked(h, (const char *)in, (char *)out, vad, n_frames, L, p);
    char *d = h->stage.p;
    float *dv = vad ? h->stage_vad.p : nullptr;
    hipError_t err = hipMemcpyAsync(d, in, p.span, hipMemcpyHostToDevice, h->stream);
    int rc = 0;
    if (err != hipSuccess) rc = fail("host staging failed: %s", hipGetErrorString(err));
    if (!rc) rc = nnn_batch_process_pcm_device(h, d, d, dv, n_frames, L, h->stream);
    if (!rc) {
        // `out` may alias `in` and may be strided: bring the span back and copy only real frames
        std::vector<char> &tmp = h->stage_host;
        const size_t image = p.vofs + (p.vad_masked ? p.vbytes : 0);
        if (tmp.size() < image) tmp.resize(image);
        err = hipMemcpyAsync(tmp.data(), d, p.span, hipMemcpyDeviceToHost, h->stream);
        if (err == hipSuccess && vad) err = hipMemcpyAsync(p.vad_masked ? (void *)(tmp.data() + p.vofs) : (void *)vad, dv, p.vbytes, hipMemcpyDeviceToHost, h->stream);
        if (err == hipSuccess) err = hipStreamSynchronize(h->stream);
        if (err == hipSuccess) {
            host_frames_back(h, (char *)out, tmp.data(), L, n_frames - p.drop);
            if (p.vad_masked) host_vad_back(h, vad, (const float *)(tmp.data() + p.vofs), n_frames);
        }
        if (err != hipSuccess) rc = fail("copy back failed: %s", hipGetErrorString(err));
        if (!rc) rc = nnn_batch_synchronize(h);   // (also reports a frame hand-off that never arrived)
    } else {
        hipStreamSynchronize(h->stream);
    }
    return rc;
}

extern "C" int nnn_batch_process_host(nnn_batch *h, const float *in, float *out, float *vad, int n_frames,
                                      size_t stream_stride, size_t frame_stride)
{
    if (!h) return fail("null batch");
    if (int rc = refuse_pending(h, "nnn_batch_process_host")) return rc;
    if (n_frames <= 0) return 0;
    if (!in || !out) return fail("null buffer");
    if (n_frames > 1 && frame_stride < (size_t)FRAME) return fail("frame_stride smaller than one frame");
    nnn_pcm_layout L = {NNN_PCM_F32, 1, 0, 0, stream_stride, frame_stride};
    return process_host_span(h, in, out, vad, n_frames, &L);
}

extern "C" int nnn_batch_process_pcm_host(nnn_batch *h, const void *in, void *out, float *vad, int n_frames,
                                          const nnn_pcm_layout *L)
{
    if (!h) return fail("null batch");
    if (int rc = refuse_pending(h, "nnn_batch_process_pcm_host")) return rc;
    if (n_frames <= 0) return 0;
    if (!in || !out) return fail("null buffer");
    if (int rc = check_layout(h, L)) return rc;
    return process_host_span(h, in, out, vad, n_frames, L);
}
