// nnn_batch_streams.hip -- per-stream state records (reset, export, import) and hold / resume, which is an export into and an import
// from the batch's own parked records.  Includes nnn_stream_state.hip (the record layout and the k_ss_* kernels).
// Needs nnn_batch_core.hip: fail / HIPCHK, struct nnn_batch, grow, dalloc, quiesce.
#pragma once

// ---- per-stream state records (include/nnn_batch.h, NNN_STREAM_STATE_*) ---------------------------------------------------------
// A record is one stream's DenoiseState in the reference's terms.  Export reads the history ring through the batch's frame count
// (input_mem comes out oldest first).  Import writes input_mem into the ring slots the next frame reads (frame_count - 1 and the
// 1248 samples before it) and re-derives what the batch keeps beside the ring with the high-pass kernels' arithmetic (k_hp / k_hp2):
// the decimated values of the last three frames (and their mirror), x_lp[0] of the next frame's slot and the last filtered sample --
// the bits the batch itself would have made.  Nothing per-frame (lpc, lpc_head, the scratch sets, pflag) is touched: the next frame
// remakes it before reading it, and k_pitch takes the last pitch of a call's first frame from last_period / last_gain, which the record
// holds.  Records are handled as 32-bit words (bit copies; ints and floats alike).
#include "nnn_stream_state.hip"   // the record layout (SS_*), SsArgs and the k_ss_* kernels

static void ss_dims_host(const nnn_batch *h, int s, int d[3])
{
    for (const nnn_batch::ModelGroup &G : h->groups)
        if (s / TILE >= G.tile0 && s / TILE < G.tile0 + G.ntiles) {
            d[0] = G.plan.vad.n;
            d[1] = G.plan.noise.n;
            d[2] = G.plan.dn.n;
            return;
        }
    d[0] = d[1] = d[2] = -1;
}
enum SsOp { SS_RESET = 0, SS_EXPORT = 1, SS_IMPORT = 2, SS_HOLD = 3, SS_RESUME = 4 };
// Everything a call can check on the host, before it writes anything.  host_rec: an import's records in host memory (checked here),
// or nullptr.  Also used by the node (nnn_node.cpp) to check every shard's part of a list before any shard is written.
int nnn_batch_check_streams(const nnn_batch *h, int op, const int *streams, int n, const void *host_rec, size_t bytes, bool need_buf)
{
    if (!h) return fail("null batch");
    static const char *const kOpNames[] = {"nnn_batch_reset_streams", "nnn_batch_export_streams", "nnn_batch_import_streams", "nnn_batch_hold_streams", "nnn_batch_resume_streams"};
    if (int rc = refuse_pending(h, kOpNames[op])) return rc;
    if (n < 0) return fail("negative stream count");
    if (n > 0 && !streams) return fail("null stream list");
    if (op == SS_EXPORT && nnn_batch_fault(h)) return fail("export refused: the batch is faulted (nnn_batch_fault); its state is invalid");
    if (op == SS_HOLD && nnn_batch_fault(h)) return fail("hold refused: the batch is faulted (nnn_batch_fault); its state is invalid");
    if (need_buf && n > 0 && !host_rec) return fail("null record buffer");
    if (need_buf && bytes < (size_t)n * NNN_STREAM_STATE_BYTES)
        return fail("record buffer too small: %zu bytes for %d records of %d", bytes, n, NNN_STREAM_STATE_BYTES);
    std::vector<char> seen(op == SS_EXPORT ? 0 : (size_t)h->S, 0);
    for (int i = 0; i < n; i++) {
        const int s = streams[i];
        if (s < 0 || s >= h->S) return fail("stream index %d (entry %d) outside [0, %d)", s, i, h->S);
        if (op != SS_EXPORT) {
            if (seen[(size_t)s]) return fail("stream %d listed twice", s);
            seen[(size_t)s] = 1;
        }
        const bool is_held = h->n_held > 0 && h->held[(size_t)s];
        if (op == SS_HOLD && is_held) return fail("stream %d (entry %d) is already held", s, i);
        if (op == SS_RESUME && !is_held) return fail("stream %d (entry %d) is not held", s, i);
    }
    if (op == SS_IMPORT && host_rec)
        for (int i = 0; i < n; i++) {
            uint32_t w[6];
            memcpy(w, (const char *)host_rec + (size_t)i * NNN_STREAM_STATE_BYTES, sizeof(w));
            if (w[0] != NNN_STREAM_STATE_MAGIC) return fail("record %d: not a stream state record (magic %08x)", i, w[0]);
            if (w[1] != NNN_STREAM_STATE_VERSION) return fail("record %d: version %u, this library reads version %d", i, w[1], NNN_STREAM_STATE_VERSION);
            if (w[2] != NNN_STREAM_STATE_BYTES) return fail("record %d: size %u, expected %d", i, w[2], NNN_STREAM_STATE_BYTES);
            int d[3];
            ss_dims_host(h, streams[i], d);
            if ((int)w[3] != d[0] || (int)w[4] != d[1] || (int)w[5] != d[2])
                return fail("record %d: GRU sizes %d/%d/%d, stream %d's model has %d/%d/%d", i, (int)w[3], (int)w[4], (int)w[5], streams[i], d[0], d[1], d[2]);
        }
    return 0;
}

// first use: the per-tile GRU sizes, the check flag, the mapped report word
static int ss_prepare(nnn_batch *h)
{
    HIPCHK(hipSetDevice(h->device));
    if (h->ss_dims) return 0;
    NNN_RT_LOCK;
    std::vector<int> dims((size_t)h->NT, 0);
    for (const nnn_batch::ModelGroup &G : h->groups)
        for (int t = G.tile0; t < G.tile0 + G.ntiles; t++) dims[(size_t)t] = G.plan.vad.n | G.plan.noise.n << 8 | G.plan.dn.n << 16;
    HIPCHK(hipMalloc((void **)&h->ss_flag, sizeof(int)));
    HIPCHK(hipMemset(h->ss_flag, 0, sizeof(int)));
    {
        void *hp = nullptr, *dp = nullptr;
        HIPCHK(hipHostMalloc(&hp, sizeof(int), hipHostMallocMapped));
        *(volatile int *)hp = 0;
        h->ss_bad_host = (volatile int *)hp;
        HIPCHK(hipHostGetDevicePointer(&dp, hp, 0));
        h->ss_bad_dev = (int *)dp;
    }
    HIPCHK(hipEventCreateWithFlags(&h->ev_ss_idx, hipEventDisableTiming));
    int *d = nullptr;
    HIPCHK(hipMalloc((void **)&d, dims.size() * sizeof(int)));
    HIPCHK(hipMemcpy(d, dims.data(), dims.size() * sizeof(int), hipMemcpyHostToDevice));
    h->ss_dims = d;
    return 0;
}
// Calls of a batch are ordered even when consecutive ones arrive on different streams (processing, state and hold calls alike):
// call_begin picks the call's stream and, if the batch's last call was made on another one, has it wait for that call's end (`e`: how
// that went); call_end makes this call the batch's last one.  A state or hold call also clears prev_pipe, which a pipelined call before
// it leaves set: the next call's high-pass must not start early (nnn_batch_set_inputs_ready) on rings this call writes -- what
// nnn_batch_load_state does.
static hipStream_t call_begin(nnn_batch *h, void *hip_stream, hipError_t &e)
{
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : h->stream;
    e = (h->have_last && h->last_stream != st) ? hipStreamWaitEvent(st, h->ev_last, 0) : hipSuccess;
    return st;
}
static hipError_t call_end(nnn_batch *h, hipStream_t st)
{
    const hipError_t e = hipEventRecord(h->ev_last, st);
    h->last_stream = st;
    h->have_last = true;
    return e;
}
static int ss_args(nnn_batch *h, const int *streams, int n, hipStream_t st, SsArgs &a, bool &tiles)
{
    memset(&a, 0, sizeof(a));
    a.dims = h->ss_dims;
    a.n = n;
    a.first = streams[0];
    bool run = true;
    for (int i = 1; i < n && run; i++) run = streams[i] == streams[0] + i;
    tiles = run && n >= TILE;
    if (run) a.mode = 0;
    else if (n <= SS_SMALL) {
        a.mode = 1;
        for (int i = 0; i < n; i++) a.small[i] = streams[i];
    } else {
        a.mode = 2;
        if ((size_t)n > h->ss_idx.cap) {   // (drained first: the old list may still be read)
            if (int rc = grow(h, true, h->ss_idx, (size_t)n * sizeof(int), (size_t)n, &h->ss_idx_pin, (size_t)n * sizeof(int))) return rc;
            h->ss_idx_busy = false;
        }
        if (h->ss_idx_busy) HIPCHK(hipEventSynchronize(h->ev_ss_idx));   // the page-locked list of the previous call has been copied
        memcpy(h->ss_idx_pin.p, streams, (size_t)n * sizeof(int));
        HIPCHK(hipMemcpyAsync(h->ss_idx.p, h->ss_idx_pin.p, (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
        HIPCHK(hipEventRecord(h->ev_ss_idx, st));
        h->ss_idx_busy = true;
        a.idx = h->ss_idx.p;
    }
    const int nslot = h->nslot, N = (int)(h->frame_count % (uint64_t)nslot);
    a.rb_in = ring_base((N + nslot - 1) % nslot, nslot);
    a.dec_row0 = 240 * ((N + nslot - 3) % nslot);
    a.slot_next = N;
    return 0;
}
static void ss_launch(nnn_batch *h, bool to_records, const SsArgs &a, bool tiles, const void *src, void *dst, hipStream_t st)
{
    const Buffers &b = h->b[0];
    const unsigned grid = tiles ? (unsigned)((a.first + a.n - 1) / TILE - a.first / TILE + 1) : (unsigned)a.n;
    if (to_records) {
        if (tiles) hipLaunchKernelGGL(k_ss_export_tiles, dim3(grid), dim3(256), 0, st, b, a, (unsigned *)dst);
        else hipLaunchKernelGGL(k_ss_export_streams, dim3(grid), dim3(256), 0, st, b, a, (unsigned *)dst);
    } else {
        if (tiles) hipLaunchKernelGGL(k_ss_import_tiles, dim3(grid), dim3(256), 0, st, b, a, (const unsigned *)src);
        else hipLaunchKernelGGL(k_ss_import_streams, dim3(grid), dim3(256), 0, st, b, a, (const unsigned *)src);
    }
}
// one state call: checks, ordering, list, kernels (to_records: export), optional copies of the host variants
static int ss_call(nnn_batch *h, SsOp op, const int *streams, int n, const void *host_src, void *host_dst, const void *d_src, void *d_dst,
                   void *hip_stream, bool device_check)
{
    if (n == 0) return 0;
    if (int rc = ss_prepare(h)) return rc;
    const size_t bytes = (size_t)n * NNN_STREAM_STATE_BYTES;
    if ((host_src || host_dst) && bytes > h->ss_stage.cap && grow(h, false, h->ss_stage, bytes, bytes)) return 1;   // (no drain: host variants wait for their work)
    hipError_t e;
    hipStream_t st = call_begin(h, hip_stream, e);
    if (e != hipSuccess) return fail("could not order the call after the batch's earlier work: %s", hipGetErrorString(hipGetLastError()));
    SsArgs a;
    bool tiles = false;
    if (int rc = ss_args(h, streams, n, st, a, tiles)) return rc;
    if (host_src) {
        HIPCHK(hipMemcpyAsync(h->ss_stage.p, host_src, bytes, hipMemcpyHostToDevice, st));
        d_src = h->ss_stage.p;
    }
    if (device_check) {
        HIPCHK(hipMemsetAsync(h->ss_flag, 0, sizeof(int), st));
        hipLaunchKernelGGL(k_ss_check, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, (const unsigned *)d_src, h->ss_flag, h->ss_bad_dev);
        a.flag = h->ss_flag;
    }
    if (op == SS_EXPORT) ss_launch(h, true, a, tiles, nullptr, host_dst ? (void *)h->ss_stage.p : d_dst, st);
    else ss_launch(h, false, a, tiles, op == SS_RESET ? nullptr : d_src, nullptr, st);
    bool any_held = false;
    for (int i = 0; i < n && h->n_held > 0 && !any_held; i++) any_held = h->held[(size_t)streams[i]] != 0;
    if (any_held)
        hipLaunchKernelGGL(k_ss_parked, dim3((unsigned)n), dim3(256), 0, st, a, (const unsigned long long *)h->live, h->park, op == SS_EXPORT ? 1 : 0,
                           (unsigned *)(host_dst ? (void *)h->ss_stage.p : d_dst), (const unsigned *)(op == SS_IMPORT ? d_src : nullptr));
    if (host_dst) HIPCHK(hipMemcpyAsync(host_dst, h->ss_stage.p, bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipGetLastError());
    HIPCHK(call_end(h, st));
    h->prev_pipe = false;
    if (host_src || host_dst) HIPCHK(hipStreamSynchronize(st));
    return 0;
}

extern "C" int nnn_batch_reset_streams(nnn_batch *h, const int *streams, int n)
{
    if (int rc = nnn_batch_check_streams(h, SS_RESET, streams, n, nullptr, 0, false)) return rc;
    return ss_call(h, SS_RESET, streams, n, nullptr, nullptr, nullptr, nullptr, nullptr, false);
}
extern "C" int nnn_batch_export_streams(nnn_batch *h, const int *streams, int n, void *host_dst, size_t dst_bytes)
{
    if (int rc = nnn_batch_check_streams(h, SS_EXPORT, streams, n, host_dst, dst_bytes, true)) return rc;
    return ss_call(h, SS_EXPORT, streams, n, nullptr, host_dst, nullptr, nullptr, nullptr, false);
}
extern "C" int nnn_batch_import_streams(nnn_batch *h, const int *streams, int n, const void *host_src, size_t src_bytes)
{
    if (int rc = nnn_batch_check_streams(h, SS_IMPORT, streams, n, host_src, src_bytes, true)) return rc;
    return ss_call(h, SS_IMPORT, streams, n, host_src, nullptr, nullptr, nullptr, nullptr, false);
}
extern "C" int nnn_batch_export_streams_device(nnn_batch *h, const int *streams, int n, void *d_dst, void *hip_stream)
{
    if (int rc = nnn_batch_check_streams(h, SS_EXPORT, streams, n, nullptr, 0, false)) return rc;
    if (n > 0 && (!d_dst || ((uintptr_t)d_dst & 3))) return fail("null or unaligned record buffer");
    return ss_call(h, SS_EXPORT, streams, n, nullptr, nullptr, nullptr, d_dst, hip_stream, false);
}
extern "C" int nnn_batch_import_streams_device(nnn_batch *h, const int *streams, int n, const void *d_src, void *hip_stream)
{
    if (int rc = nnn_batch_check_streams(h, SS_IMPORT, streams, n, nullptr, 0, false)) return rc;
    if (n > 0 && (!d_src || ((uintptr_t)d_src & 3))) return fail("null or unaligned record buffer");
    return ss_call(h, SS_IMPORT, streams, n, nullptr, nullptr, d_src, nullptr, hip_stream, true);
}

// ---- hold and resume (include/nnn_batch.h) ---------------------------------------------------------------------
// Hold = the export above into the batch's own parked records, resume = the import from them (which re-phases the history into the ring
// slots the frame counter of NOW reads); the same launch flips the streams' bits of the live mask the processing kernels look at.
static std::vector<unsigned long long> live_all(const nnn_batch *h)
{
    std::vector<unsigned long long> w((size_t)h->NT, ~0ull);
    if (h->S % TILE) w.back() = (1ull << (h->S % TILE)) - 1ull;   // (padding streams are never live)
    return w;
}
static int hold_prepare(nnn_batch *h)
{
    if (h->park) return 0;
    NNN_RT_LOCK;
    if (int rc = quiesce(h)) return rc;
    unsigned *park = nullptr;
    unsigned long long *live = nullptr;
    HIPCHK(dalloc(h, &park, (size_t)h->S * SS_WORDS, false));
    HIPCHK(dalloc(h, &live, (size_t)h->NT, false));
    const std::vector<unsigned long long> w = live_all(h);
    HIPCHK(hipMemcpy(live, w.data(), w.size() * sizeof(w[0]), hipMemcpyHostToDevice));
    HIPCHK(hipDeviceSynchronize());
    h->park = park;
    h->live = live;
    h->held.assign((size_t)h->S, 0);
    h->n_held = 0;
    for (int set = 0; set < NSET; set++) h->b[set].live = live;   // (every argument block, the ones a later nnn_batch_set_taps re-derives included)
    return 0;
}
static int hold_call(nnn_batch *h, bool hold, const int *streams, int n)
{
    if (int rc = nnn_batch_check_streams(h, hold ? SS_HOLD : SS_RESUME, streams, n, nullptr, 0, false)) return rc;
    // (the first hold of a batch allocates the parked records and the mask, which waits for the device: a host that cannot stall at its
    // first mute makes an empty hold -- n = 0 -- when it creates the batch)
    if (n == 0 && !hold) return 0;
    if (int rc = ss_prepare(h)) return rc;
    if (int rc = hold_prepare(h)) return rc;
    if (n == 0) return 0;
    hipError_t e;
    hipStream_t st = call_begin(h, nullptr, e);
    if (e != hipSuccess) return fail("could not order the call after the batch's earlier work: %s", hipGetErrorString(hipGetLastError()));
    SsArgs a;
    bool tiles = false;
    if (int rc = ss_args(h, streams, n, st, a, tiles)) return rc;
    a.by_stream = 1;
    a.live_op = hold ? 1 : 2;
    a.live = h->live;
    unsigned *rec0 = h->park + (tiles ? (size_t)a.first * SS_WORDS : 0);   // (the tile kernels count records from the list's first stream)
    ss_launch(h, hold, a, tiles, rec0, rec0, st);
    // (the launch is enqueued and will flip the device's bits: the host's copy follows it whatever the bookkeeping below reports)
    for (int i = 0; i < n; i++) h->held[(size_t)streams[i]] = hold ? 1 : 0;
    h->n_held += hold ? n : -n;
    HIPCHK(hipGetLastError());
    HIPCHK(call_end(h, st));
    h->prev_pipe = false;
    return 0;
}
extern "C" int nnn_batch_hold_streams(nnn_batch *h, const int *streams, int n) { return hold_call(h, true, streams, n); }
extern "C" int nnn_batch_resume_streams(nnn_batch *h, const int *streams, int n) { return hold_call(h, false, streams, n); }
extern "C" int nnn_batch_num_held(const nnn_batch *h) { return h ? h->n_held : 0; }
extern "C" int nnn_batch_held_mask(const nnn_batch *h, uint8_t *held, size_t n)
{
    if (!h || !held) return fail("null argument");
    if (n < (size_t)h->S) return fail("mask buffer too small: %d entries needed", h->S);
    for (int s = 0; s < h->S; s++) held[s] = h->n_held > 0 ? h->held[(size_t)s] : 0;
    return 0;
}
// nnn_batch_reset: every stream takes part again
static int hold_release_all(nnn_batch *h)
{
    if (!h->live) return 0;
    const std::vector<unsigned long long> w = live_all(h);
    HIPCHK(hipMemcpy(h->live, w.data(), w.size() * sizeof(w[0]), hipMemcpyHostToDevice));
    h->held.assign((size_t)h->S, 0);
    h->n_held = 0;
    return 0;
}
