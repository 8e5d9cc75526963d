// nnn_batch_floor.hip -- per-stream gain floors (include/nnn_batch.h "Gain floors"): the scatter kernel that writes the
// listed streams' floor rows, and set / get / num_floored.  The floor itself is applied in the gains sinks of the RNN kernels (rnn_gain_out
// of nnn_rnn.hip, the output layer's sink in k_back) and nowhere else.
// Needs nnn_batch_core.hip (fail / HIPCHK, struct nnn_batch, grow, dalloc, quiesce) and call_begin / call_end of nnn_batch_streams.hip.
#pragma once

// floors[i * 22 + band] into row `band` of stream streams[i]: one thread per value (a listed stream appears once: no two threads share a word)
__global__ void __launch_bounds__(256) k_floor_set(float *gfloor, const int *streams, const float *floors, int n)
{
    const int e = (int)(blockIdx.x * 256 + threadIdx.x);
    if (e >= n * NB) return;
    const int i = e / NB, band = e - i * NB, s = streams[i];
    NNN_TI(gfloor, NB, s / TILE, s % TILE)[(size_t)band * TILE] = floors[e];
}

// Everything a set or get call can check on the host, before it changes anything (floors = nullptr: a get, whose list may repeat).  Also
// used by the node (nnn_node.cpp) to check every shard's part of a list before any shard is changed.
int nnn_batch_check_gain_floor(const nnn_batch *h, const int *streams, int n, const float *floors, int bands, bool set)
{
    if (!h) return fail("null batch");
    if (n < 0) return fail("negative stream count");
    if (n > 0 && !streams) return fail("null stream list");
    if (n > 0 && !floors) return fail(set ? "null floor values" : "null floor buffer");
    if (!set) bands = NB;
    if (bands != 1 && bands != NB) return fail("bands is %d: a stream takes 1 floor (all %d bands) or %d", bands, NB, NB);
    std::vector<char> seen(set ? (size_t)h->S : 0, 0);
    for (int i = 0; i < n; i++) {
        const int s = streams[i];
        if (s < 0 || s >= h->S) return fail("stream index %d (entry %d) outside [0, %d)", s, i, h->S);
        if (!set) continue;
        if (seen[(size_t)s]) return fail("stream %d listed twice", s);
        seen[(size_t)s] = 1;
        for (int k = 0; k < bands; k++) {
            const float v = floors[(size_t)i * bands + k];
            if (!(v >= 0.0f && v <= 1.0f)) return fail("floor %g (stream %d, value %d) outside [0, 1]", (double)v, s, k);   // (NaN fails both)
        }
    }
    return 0;
}

// first use: the floor rows (zero: off) and the host's copy.  Waits for the batch's work and synchronises the device, like the first hold.
static int floor_prepare(nnn_batch *h)
{
    HIPCHK(hipSetDevice(h->device));
    if (h->gfloor) return 0;
    NNN_RT_LOCK;
    if (int rc = quiesce(h)) return rc;
    float *rows = nullptr;
    HIPCHK(dalloc(h, &rows, (size_t)h->S_pad * NB, false));
    HIPCHK(hipEventCreateWithFlags(&h->ev_fl, hipEventDisableTiming));
    HIPCHK(hipDeviceSynchronize());
    h->gfloor = rows;
    h->gfloor_host.assign((size_t)h->S * NB, 0.0f);
    h->n_floored = 0;
    return 0;
}
// the argument blocks see the rows only while some floor is above 0 (every block, the ones a later nnn_batch_set_taps re-derives included)
static void floor_publish(nnn_batch *h)
{
    for (int set = 0; set < NSET; set++) h->b[set].gfloor = h->n_floored > 0 ? h->gfloor : nullptr;
}
static bool floor_any(const nnn_batch *h, int s)
{
    for (int k = 0; k < NB; k++)
        if (h->gfloor_host[(size_t)s * NB + k] > 0.0f) return true;
    return false;
}

extern "C" int nnn_batch_set_gain_floor(nnn_batch *h, const int *streams, int n, const float *floors, int bands)
{
    if (int rc = nnn_batch_check_gain_floor(h, streams, n, floors, bands, true)) return rc;
    // (the first set of a batch allocates the rows, which waits for the device: a host that cannot stall at its first floor makes an empty
    // set -- n = 0 -- when it creates the batch)
    if (int rc = floor_prepare(h)) return rc;
    if (n == 0) return 0;
    const size_t vbytes = (size_t)n * NB * sizeof(float), bytes = vbytes + (size_t)n * sizeof(int);
    if ((size_t)n > h->fl_stage.cap) {   // (drained first: the old list may still be read)
        if (int rc = grow(h, true, h->fl_stage, bytes, (size_t)n, &h->fl_pin, bytes)) return rc;
        h->fl_busy = false;
    }
    if (h->fl_busy) HIPCHK(hipEventSynchronize(h->ev_fl));   // the page-locked values of the previous set have been copied
    float *pv = (float *)h->fl_pin.p;
    for (int i = 0; i < n; i++)
        for (int k = 0; k < NB; k++) pv[(size_t)i * NB + k] = floors[(size_t)i * bands + (bands == 1 ? 0 : k)];
    memcpy(h->fl_pin.p + vbytes, streams, (size_t)n * sizeof(int));
    hipError_t e;
    hipStream_t st = call_begin(h, nullptr, e);
    if (e != hipSuccess) return fail("could not order the call after the batch's earlier work: %s", hipGetErrorString(hipGetLastError()));
    HIPCHK(hipMemcpyAsync(h->fl_stage.p, h->fl_pin.p, bytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(h->ev_fl, st));
    h->fl_busy = true;
    hipLaunchKernelGGL(k_floor_set, dim3((unsigned)((n * NB + 255) / 256)), dim3(256), 0, st, h->gfloor, (const int *)(h->fl_stage.p + vbytes),
                       (const float *)h->fl_stage.p, n);
    // (the launch is enqueued and will write the device's rows: the host's copy follows it whatever the bookkeeping below reports)
    for (int i = 0; i < n; i++) {
        const int s = streams[i];
        h->n_floored -= floor_any(h, s) ? 1 : 0;
        memcpy(&h->gfloor_host[(size_t)s * NB], pv + (size_t)i * NB, NB * sizeof(float));
        h->n_floored += floor_any(h, s) ? 1 : 0;
    }
    floor_publish(h);
    HIPCHK(hipGetLastError());
    HIPCHK(call_end(h, st));
    h->prev_pipe = false;
    return 0;
}

// the rows as the device holds them once the batch's work is done (a batch that never allocated them: zeros)
extern "C" int nnn_batch_get_gain_floor(nnn_batch *h, const int *streams, int n, float *floors)
{
    if (int rc = nnn_batch_check_gain_floor(h, streams, n, floors, NB, false)) return rc;
    if (n == 0) return 0;
    if (!h->gfloor) {
        memset(floors, 0, (size_t)n * NB * sizeof(float));
        return 0;
    }
    NNN_RT_LOCK;
    if (int rc = quiesce(h)) return rc;
    std::vector<float> rows((size_t)h->S_pad * NB);
    HIPCHK(hipMemcpy(rows.data(), h->gfloor, rows.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++)
        for (int k = 0; k < NB; k++) floors[(size_t)i * NB + k] = *NNN_TI(rows.data() + (size_t)k * TILE, NB, streams[i] / TILE, streams[i] % TILE);
    return 0;
}
extern "C" int nnn_batch_num_floored(const nnn_batch *h) { return h ? h->n_floored : 0; }

// nnn_batch_clone: the clone `c` (just created, idle) takes h's floors (h is quiescent)
static int floor_clone(nnn_batch *c, const nnn_batch *h)
{
    if (!h->gfloor) return 0;
    if (int rc = floor_prepare(c)) return rc;
    HIPCHK(hipMemcpy(c->gfloor, h->gfloor, (size_t)h->S_pad * NB * sizeof(float), hipMemcpyDeviceToDevice));
    HIPCHK(hipDeviceSynchronize());
    c->gfloor_host = h->gfloor_host;
    c->n_floored = h->n_floored;
    floor_publish(c);
    return 0;
}
