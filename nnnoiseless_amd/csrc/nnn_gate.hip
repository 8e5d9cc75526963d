// nnn_gate.hip -- the VAD gate (include/nnn_gate.h): threshold, grace and look-back per stream behind the denoiser.
// One call = k_gate_scan (a lane per stream, serial over the call's frames: the counter, the decisions, the only sequential part) and
// k_gate_apply (a thread per stream and four consecutive samples, the same four in every frame of the call, walking the frames from the
// last to the first), on the caller's stream.
// Needs fail / HIPCHK / NNN_RT_LOCK (nnn_batch_core.hip), pcm_to_i16 and the PCM_* formats (nnn_common.hip), pk_s16 (nnn_pack.hip).
#pragma once

#include "../../include/nnn_gate.h"

// ---- the kernels ------------------------------------------------------------------------------------------------------------------------
constexpr int GATE_THREADS = 256;
constexpr int GATE_VEC = 4;                           // consecutive samples of its stream a thread of k_gate_apply owns
constexpr int GATE_COLS = FRAME / GATE_VEC;           // 120 threads per stream
constexpr int GATE_RUN = 4;                           // frames whose sources a thread fetches before it writes the first of them
constexpr int GATE_SCAN_RUN = 8;                      // VAD values a lane of k_gate_scan fetches before it stores their decisions
constexpr int GATE_HMAX = NNN_GATE_MAX_LOOKBACK;
static_assert(FRAME == NNN_GATE_FRAME && FRAME % GATE_VEC == 0, "");

struct GateScanArgs {
    const float *vad;                 // [T][S]
    const unsigned char *live;        // NULL or [S]
    const float *thr;                 // [S]
    const int *grace, *look;          // [S]
    int *since, *was;                 // [S]: the state
    unsigned char *pair;              // [T][S]: bit 0 = open_n, bit 1 = open_(n-1)
    unsigned char *open;              // NULL or [T][S]
    int S, T;
};

// Lane = stream: steps 1 to 3 of the header's rule over the call's frames in order.  The reads of vad[t * S + s] and the writes of the
// pair and d_open bytes are coalesced across the lanes; nothing else in a call is sequential.
__global__ void __launch_bounds__(GATE_THREADS) k_gate_scan(GateScanArgs a)
{
    const int s = (int)(blockIdx.x * GATE_THREADS + threadIdx.x);
    if (s >= a.S || (a.live && !a.live[s])) return;
    const float thr = a.thr[s];
    const int lim = a.grace[s] + a.look[s];
    int since = a.since[s], prev = a.was[s];
    for (int t0 = 0; t0 < a.T; t0 += GATE_SCAN_RUN) {              // (a run's loads first: a store between two loads would order them)
        float v[GATE_SCAN_RUN];
#pragma unroll
        for (int k = 0; k < GATE_SCAN_RUN; k++)
            if (t0 + k < a.T) v[k] = a.vad[(size_t)(t0 + k) * a.S + s];
#pragma unroll
        for (int k = 0; k < GATE_SCAN_RUN; k++) {
            if (t0 + k >= a.T) break;
            const size_t at = (size_t)(t0 + k) * a.S + s;
            const bool voiced = v[k] >= thr;                        // (false for NaN)
            since = voiced ? 0 : since == NNN_GATE_NEVER ? NNN_GATE_NEVER : since + 1;
            const int open = since <= lim;
            a.pair[at] = (unsigned char)(open | prev << 1);
            if (a.open) a.open[at] = (unsigned char)open;
            prev = open;
        }
    }
    a.since[s] = since, a.was[s] = prev;
}

struct GateArgs {
    const char *in;                   // element (s, t, i) at (s / C) * gs + t * fs + i * C + s % C, in elements of the format
    char *out;
    const unsigned char *pair;        // [T][S], k_gate_scan's
    const unsigned char *live;        // NULL or [S]
    const int *look;                  // [S]
    const float *level;               // [S]
    float *hist;                      // [S][H][480]: row r < R of stream s is its input frame n - R + r
    const float *ramp;                // [480]: (float)(i + 1) / 480.0f
    long long gs, fs;
    int S, T, C, H, inplace;
};

struct Gate4 { unsigned v[GATE_VEC]; };   // four samples as the bits of their floats: a copy moves bits, whatever they encode

// The four elements e, e + C, e + 2 C, e + 3 C of the caller's audio as floats' bits.  One channel and an address that allows it: one
// 16-byte access (8 for int16), as nnn_pack.hip's accesses decide it; else word by word, or element by element.
template <int FMT> __device__ __forceinline__ Gate4 gate_load(const char *base, long long e, int C)
{
    Gate4 r;
    if (FMT == PCM_I16) {
        const short *p = (const short *)base + e;
        const uintptr_t a = (uintptr_t)p;
        if (C == 1 && (a & 7) == 0) {
            const uint2 w = *(const uint2 *)p;
            r.v[0] = __float_as_uint(pk_s16(w.x)), r.v[1] = __float_as_uint(pk_s16(w.x >> 16));
            r.v[2] = __float_as_uint(pk_s16(w.y)), r.v[3] = __float_as_uint(pk_s16(w.y >> 16));
        } else if (C == 1 && (a & 3) == 0) {
            const unsigned w0 = ((const unsigned *)p)[0], w1 = ((const unsigned *)p)[1];
            r.v[0] = __float_as_uint(pk_s16(w0)), r.v[1] = __float_as_uint(pk_s16(w0 >> 16));
            r.v[2] = __float_as_uint(pk_s16(w1)), r.v[3] = __float_as_uint(pk_s16(w1 >> 16));
        } else {
#pragma unroll
            for (int k = 0; k < GATE_VEC; k++) r.v[k] = __float_as_uint((float)p[(long long)k * C]);
        }
    } else {
        const unsigned *p = (const unsigned *)base + e;
        if (C == 1 && ((uintptr_t)p & 15) == 0) {
            const uint4 w = *(const uint4 *)p;
            r.v[0] = w.x, r.v[1] = w.y, r.v[2] = w.z, r.v[3] = w.w;
        } else {
#pragma unroll
            for (int k = 0; k < GATE_VEC; k++) r.v[k] = p[(long long)k * C];
        }
    }
    return r;
}

template <int FMT> __device__ __forceinline__ void gate_store(char *base, long long e, int C, const Gate4 &y)
{
    if (FMT == PCM_I16) {
        short *q = (short *)base + e;
        unsigned s[GATE_VEC];
#pragma unroll
        for (int k = 0; k < GATE_VEC; k++) s[k] = (unsigned short)pcm_to_i16(__uint_as_float(y.v[k]));
        const uintptr_t a = (uintptr_t)q;
        if (C == 1 && (a & 7) == 0) {
            uint2 w;
            w.x = s[0] | s[1] << 16, w.y = s[2] | s[3] << 16;
            *(uint2 *)q = w;
        } else if (C == 1 && (a & 3) == 0) {
            ((unsigned *)q)[0] = s[0] | s[1] << 16;
            ((unsigned *)q)[1] = s[2] | s[3] << 16;
        } else {
#pragma unroll
            for (int k = 0; k < GATE_VEC; k++) q[(long long)k * C] = (short)s[k];
        }
    } else {
        unsigned *q = (unsigned *)base + e;
        if (C == 1 && ((uintptr_t)q & 15) == 0) {
            uint4 w;
            w.x = y.v[0], w.y = y.v[1], w.z = y.v[2], w.w = y.v[3];
            *(uint4 *)q = w;
        } else {
#pragma unroll
            for (int k = 0; k < GATE_VEC; k++) q[(long long)k * C] = y.v[k];
        }
    }
}

__device__ __forceinline__ Gate4 gate_hist_load(const float *row)
{
    const uint4 w = *(const uint4 *)row;
    Gate4 r;
    r.v[0] = w.x, r.v[1] = w.y, r.v[2] = w.z, r.v[3] = w.w;
    return r;
}

// Steps 4 to 7 of the header's rule.  A thread owns samples i0 .. i0 + 3 of stream s in EVERY frame of the call -- the same elements of
// the caller's rows and of the history rows, which nobody else touches.  It (1) loads the call's last R source frames, the history the
// next call begins with, (2) walks the frames from the last to the first, writing out_t from in_(t-R) or, before the call's first frame,
// from the old history, and (3) stores the new history.  In place (out == in exactly) frame t is written when every source the thread
// still needs lies below t and the tail is in registers, so no second buffer and no ordering between threads or blocks is needed; the
// sources of GATE_RUN frames are fetched ahead of their writes, which is safe for the same reason (a load made early sees the caller's
// data; only a store made early could hurt).  Where the contract makes the bytes known nothing moves: an open frame at R = 0 in place is
// neither read nor written, a muted frame is not read.
template <int FMT> __global__ void __launch_bounds__(GATE_THREADS) k_gate_apply(GateArgs a)
{
#pragma clang fp contract(off)
    const long long id = (long long)blockIdx.x * GATE_THREADS + threadIdx.x;
    const int s = (int)(id / GATE_COLS), i0 = (int)(id % GATE_COLS) * GATE_VEC;
    if (s >= a.S || (a.live && !a.live[s])) return;
    const int R = a.look[s], C = a.C, T = a.T;
    const float level = a.level[s];
    const long long col = (long long)(s / C) * a.gs + (long long)i0 * C + s % C;   // the thread's first element in frame 0
    float *hrow = a.hist + ((size_t)s * a.H) * FRAME + i0;
    const float4 rp = *(const float4 *)(a.ramp + i0);
    const float ramp[GATE_VEC] = {rp.x, rp.y, rp.z, rp.w};

    // source frame j of the call (j >= -R): the caller's frame j, or row j + R of the history
    auto source = [&](int j) { return j >= 0 ? gate_load<FMT>(a.in, col + (long long)j * a.fs, C) : gate_hist_load(hrow + (size_t)(j + R) * FRAME); };

    Gate4 tail[GATE_HMAX];
#pragma unroll
    for (int r = 0; r < GATE_HMAX; r++)
        if (r < R) tail[r] = source(T - R + r);

    // the decisions of frames t1, t1 - 1, ...: fetched a run ahead, so that no source load waits for the byte that says whether it is needed
    auto decisions = [&](int t1, unsigned char *pr) {
#pragma unroll
        for (int k = 0; k < GATE_RUN; k++) pr[k] = t1 - k >= 0 ? a.pair[(size_t)(t1 - k) * a.S + s] : (unsigned char)0;
    };
    unsigned char ahead[GATE_RUN];
    decisions(T - 1, ahead);
    for (int t1 = T - 1; t1 >= 0; t1 -= GATE_RUN) {
        Gate4 x[GATE_RUN];
        unsigned char pr[GATE_RUN];
#pragma unroll
        for (int k = 0; k < GATE_RUN; k++) pr[k] = ahead[k];
        decisions(t1 - GATE_RUN, ahead);
#pragma unroll
        for (int k = 0; k < GATE_RUN; k++) {
            const int t = t1 - k;
            if (t < 0) break;
            const float hn = (pr[k] & 1) ? 1.0f : level, hp = (pr[k] & 2) ? 1.0f : level;
            const bool flat = hp == hn;
            const bool skip = flat && (hn == 0.0f || (hn == 1.0f && R == 0 && a.inplace));
            if (!skip) x[k] = source(t - R);
            else x[k].v[0] = x[k].v[1] = x[k].v[2] = x[k].v[3] = 0u;
        }
#pragma unroll
        for (int k = 0; k < GATE_RUN; k++) {
            const int t = t1 - k;
            if (t < 0) break;
            const float hn = (pr[k] & 1) ? 1.0f : level, hp = (pr[k] & 2) ? 1.0f : level;
            if (hp == hn && hn == 1.0f && R == 0 && a.inplace) continue;
            Gate4 y;
#pragma unroll
            for (int q = 0; q < GATE_VEC; q++) {
                const float g = hp == hn ? hn : hp + (hn - hp) * ramp[q];
                y.v[q] = g == 1.0f ? x[k].v[q] : g == 0.0f ? 0u : __float_as_uint(__uint_as_float(x[k].v[q]) * g);
            }
            gate_store<FMT>(a.out, col + (long long)t * a.fs, C, y);
        }
    }

#pragma unroll
    for (int r = 0; r < GATE_HMAX; r++)
        if (r < R) {
            uint4 w;
            w.x = tail[r].v[0], w.y = tail[r].v[1], w.z = tail[r].v[2], w.w = tail[r].v[3];
            *(uint4 *)(hrow + (size_t)r * FRAME) = w;
        }
}

// since, was_open and the history of the flagged streams to their reset values (a block per stream)
__global__ void __launch_bounds__(128) k_gate_clear(const unsigned char *flag, float *hist, int *since, int *was, int S, int H)
{
    const int s = blockIdx.x;
    if (s >= S || !flag[s]) return;
    for (int j = threadIdx.x; j < H * FRAME; j += 128) hist[(size_t)s * H * FRAME + j] = 0.0f;
    if (threadIdx.x == 0) since[s] = NNN_GATE_NEVER, was[s] = 0;
}

// ---- the host side ------------------------------------------------------------------------------------------------------------------------
struct nnn_gate {
    int S = 0, H = 0, device = 0;                   // H = max_lookback: the history's rows per stream
    std::vector<nnn_gate_params> par;               // as the host set them; the four device arrays are their copy
    float *d_thr = nullptr, *d_level = nullptr;
    int *d_grace = nullptr, *d_look = nullptr;
    int *d_since = nullptr, *d_was = nullptr;       // [S]
    float *d_hist = nullptr;                        // [S][H][480]
    float *d_ramp = nullptr;                        // [480]
    unsigned char *d_flag = nullptr;                // [S]: the streams a reset names
    unsigned char *d_pair = nullptr;                // [T][S] of the longest call (grow only)
    size_t pair_cap = 0;
    hipStream_t own_stream = nullptr;
    hipEvent_t ev_last = nullptr;                   // end of the most recent call, on the stream it was made on
    hipStream_t last_stream = nullptr;
    bool have_last = false;
    // device buffers of the host entry point (made on first use, grow only)
    float *h_audio = nullptr, *h_vad = nullptr;
    unsigned char *h_live = nullptr, *h_open = nullptr;
    size_t h_audio_cap = 0, h_vad_cap = 0, h_live_cap = 0, h_open_cap = 0;   // bytes
};

extern "C" void nnn_gate_destroy(nnn_gate *h)
{
    if (!h) return;
    NNN_RT_LOCK;
    hipSetDevice(h->device);
    if (h->have_last) hipEventSynchronize(h->ev_last);
    hipFree(h->d_thr); hipFree(h->d_level); hipFree(h->d_grace); hipFree(h->d_look); hipFree(h->d_since); hipFree(h->d_was);
    hipFree(h->d_hist); hipFree(h->d_ramp); hipFree(h->d_flag); hipFree(h->d_pair);
    hipFree(h->h_audio); hipFree(h->h_vad); hipFree(h->h_live); hipFree(h->h_open);
    if (h->own_stream) hipStreamDestroy(h->own_stream);
    if (h->ev_last) hipEventDestroy(h->ev_last);
    delete h;
}

// everything enqueued so far is done
static int gate_drain(nnn_gate *h)
{
    HIPCHK(hipSetDevice(h->device));
    if (h->have_last) HIPCHK(hipEventSynchronize(h->ev_last));
    return 0;
}

// the host's parameters to the device; the caller holds the lock and has drained the object
static int gate_upload_params(nnn_gate *h)
{
    const size_t S = (size_t)h->S;
    std::vector<float> f(2 * S);
    std::vector<int> i(2 * S);
    for (size_t s = 0; s < S; s++) f[s] = h->par[s].threshold, f[S + s] = h->par[s].level, i[s] = h->par[s].grace, i[S + s] = h->par[s].lookback;
    HIPCHK(hipMemcpy(h->d_thr, f.data(), S * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_level, f.data() + S, S * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_grace, i.data(), S * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_look, i.data() + S, S * sizeof(int), hipMemcpyHostToDevice));
    return 0;
}

// reset the listed streams (idx == NULL: streams 0 .. n - 1); the caller holds the lock and has drained the object
static int gate_clear(nnn_gate *h, const int *idx, int n)
{
    std::vector<unsigned char> flag((size_t)h->S, 0);
    for (int i = 0; i < n; i++) flag[(size_t)(idx ? idx[i] : i)] = 1;
    HIPCHK(hipMemcpy(h->d_flag, flag.data(), flag.size(), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_gate_clear, dim3((unsigned)h->S), dim3(128), 0, h->own_stream, (const unsigned char *)h->d_flag, h->d_hist, h->d_since, h->d_was,
                       h->S, h->H);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->own_stream));
    return 0;
}

extern "C" nnn_gate *nnn_gate_create(int n_streams, int max_lookback, int device)
{
    if (n_streams < 1 || (long long)n_streams * GATE_COLS > 0x7fffffffll) { fail("nnn_gate_create: n_streams = %d", n_streams); return nullptr; }
    if (max_lookback < 0 || max_lookback > NNN_GATE_MAX_LOOKBACK) {
        fail("nnn_gate_create: max_lookback = %d outside [0, %d]", max_lookback, NNN_GATE_MAX_LOOKBACK);
        return nullptr;
    }
    NNN_RT_LOCK;
    if (hipSetDevice(device) != hipSuccess) { fail("nnn_gate_create: no such HIP device"); return nullptr; }
    nnn_gate *h = new nnn_gate();
    h->S = n_streams, h->H = max_lookback, h->device = device;
    h->par.assign((size_t)n_streams, nnn_gate_params{0.0f, 0, 0, 0.0f});
    const size_t S = (size_t)n_streams, hist = (S * h->H ? S * h->H * FRAME : 4) * sizeof(float);
    bool ok = true;
    auto dev = [&](auto **q, size_t bytes) { ok = ok && hipMalloc((void **)q, bytes) == hipSuccess && hipMemset(*q, 0, bytes) == hipSuccess; };
    dev(&h->d_thr, S * sizeof(float)), dev(&h->d_level, S * sizeof(float));
    dev(&h->d_grace, S * sizeof(int)), dev(&h->d_look, S * sizeof(int));
    dev(&h->d_since, S * sizeof(int)), dev(&h->d_was, S * sizeof(int));
    dev(&h->d_hist, hist);
    dev(&h->d_ramp, FRAME * sizeof(float));
    dev(&h->d_flag, S);
    ok = ok && hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&h->ev_last, hipEventDisableTiming) == hipSuccess;
    if (ok) {
        float ramp[FRAME];
        for (int i = 0; i < FRAME; i++) ramp[i] = (float)(i + 1) / 480.0f;
        std::vector<int> never(S, NNN_GATE_NEVER);
        ok = hipMemcpy(h->d_ramp, ramp, sizeof(ramp), hipMemcpyHostToDevice) == hipSuccess
             && hipMemcpy(h->d_since, never.data(), S * sizeof(int), hipMemcpyHostToDevice) == hipSuccess;
    }
    ok = ok && hipDeviceSynchronize() == hipSuccess;   // (the memsets above are on the legacy stream; the calls are on non-blocking ones)
    if (!ok) {
        nnn_gate_destroy(h);
        fail("nnn_gate_create: allocation failed (%d bytes for each of %d streams)", 1920 * max_lookback + 25, n_streams);
        return nullptr;
    }
    return h;
}

// an index list of a call: inside the object, and no stream twice where `once` asks for that
static int gate_streams(const nnn_gate *h, const int *idx, int n, bool once, const char *who)
{
    if (n < 0) return fail("%s: n = %d", who, n);
    if (!idx && n > h->S) return fail("%s: %d entries for %d streams", who, n, h->S);
    std::vector<char> seen(once && idx ? (size_t)h->S : 0, 0);
    for (int i = 0; idx && i < n; i++) {
        if (idx[i] < 0 || idx[i] >= h->S) return fail("%s: stream %d outside [0, %d)", who, idx[i], h->S);
        if (once) {
            if (seen[(size_t)idx[i]]) return fail("%s: stream %d is listed twice", who, idx[i]);
            seen[(size_t)idx[i]] = 1;
        }
    }
    return 0;
}

static int gate_params_ok(const nnn_gate_params &p, int max_lookback, int i, const char *who)
{
    if (!(p.threshold >= 0.0f && p.threshold <= 1.0f)) return fail("%s: entry %d: threshold %g outside [0, 1]", who, i, (double)p.threshold);
    if (p.grace < 0 || p.grace > NNN_GATE_MAX_GRACE) return fail("%s: entry %d: grace %d outside [0, %d]", who, i, (int)p.grace, NNN_GATE_MAX_GRACE);
    if (p.lookback < 0 || p.lookback > max_lookback) return fail("%s: entry %d: lookback %d outside [0, %d]", who, i, (int)p.lookback, max_lookback);
    if (!(p.level >= 0.0f && p.level <= 1.0f)) return fail("%s: entry %d: level %g outside [0, 1]", who, i, (double)p.level);
    return 0;
}

extern "C" int nnn_gate_set_params(nnn_gate *h, const int *idx, int n, const nnn_gate_params *params)
{
    if (!h) return fail("null gate");
    if (int rc = gate_streams(h, idx, n, true, "nnn_gate_set_params")) return rc;
    if (n == 0) return 0;
    if (!params) return fail("nnn_gate_set_params: null params");
    for (int i = 0; i < n; i++)
        if (int rc = gate_params_ok(params[i], h->H, i, "nnn_gate_set_params")) return rc;
    NNN_RT_LOCK;
    if (int rc = gate_drain(h)) return rc;
    for (int i = 0; i < n; i++) h->par[(size_t)(idx ? idx[i] : i)] = params[i];
    if (int rc = gate_upload_params(h)) return rc;
    return gate_clear(h, idx, n);
}

extern "C" int nnn_gate_get_params(nnn_gate *h, const int *idx, int n, nnn_gate_params *params)
{
    if (!h) return fail("null gate");
    if (int rc = gate_streams(h, idx, n, false, "nnn_gate_get_params")) return rc;
    if (n == 0) return 0;
    if (!params) return fail("nnn_gate_get_params: null params");
    for (int i = 0; i < n; i++) params[i] = h->par[(size_t)(idx ? idx[i] : i)];
    return 0;
}

extern "C" int nnn_gate_reset(nnn_gate *h, const int *idx, int n)
{
    if (!h) return fail("null gate");
    if (!idx) n = h->S;
    if (int rc = gate_streams(h, idx, n, false, "nnn_gate_reset")) return rc;
    if (n == 0) return 0;
    NNN_RT_LOCK;
    if (int rc = gate_drain(h)) return rc;
    return gate_clear(h, idx, n);
}

// one call on the unified addressing: element (s, t, i) at (s / C) * gs + t * fs + i * C + s % C; everything is validated by now
static int gate_enqueue(nnn_gate *h, int fmt, const void *d_in, void *d_out, const float *d_vad, const uint8_t *d_live, uint8_t *d_open, int n_frames,
                        int C, size_t gs, size_t fs, void *hip_stream)
{
    HIPCHK(hipSetDevice(h->device));
    const size_t rows = (size_t)n_frames * h->S;
    if (rows > h->pair_cap) {
        NNN_RT_LOCK;
        if (int rc = gate_drain(h)) return rc;
        HIPCHK(hipFree(h->d_pair));
        h->d_pair = nullptr, h->pair_cap = 0;
        HIPCHK(hipMalloc((void **)&h->d_pair, rows));
        h->pair_cap = rows;
    }
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : h->own_stream;
    if (h->have_last && h->last_stream != st) HIPCHK(hipStreamWaitEvent(st, h->ev_last, 0));   // (state and scratch are the previous call's until then)
    GateScanArgs sa = {};
    sa.vad = d_vad, sa.live = d_live, sa.thr = h->d_thr, sa.grace = h->d_grace, sa.look = h->d_look, sa.since = h->d_since, sa.was = h->d_was;
    sa.pair = h->d_pair, sa.open = d_open, sa.S = h->S, sa.T = n_frames;
    hipLaunchKernelGGL(k_gate_scan, dim3((unsigned)((h->S + GATE_THREADS - 1) / GATE_THREADS)), dim3(GATE_THREADS), 0, st, sa);
    GateArgs a = {};
    a.in = (const char *)d_in, a.out = (char *)d_out, a.pair = h->d_pair, a.live = d_live, a.look = h->d_look, a.level = h->d_level;
    a.hist = h->d_hist, a.ramp = h->d_ramp, a.gs = (long long)gs, a.fs = (long long)fs;
    a.S = h->S, a.T = n_frames, a.C = C, a.H = h->H, a.inplace = d_in == d_out;
    const dim3 grid((unsigned)(((long long)h->S * GATE_COLS + GATE_THREADS - 1) / GATE_THREADS)), block(GATE_THREADS);
    if (fmt == PCM_I16) hipLaunchKernelGGL(k_gate_apply<PCM_I16>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(k_gate_apply<PCM_F32>, grid, block, 0, st, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev_last, st));
    h->last_stream = st;
    h->have_last = true;
    return 0;
}

static int gate_call_ok(const nnn_gate *h, const void *d_in, const void *d_out, const float *d_vad, int n_frames)
{
    if (!h) return fail("null gate");
    if (!d_in || !d_out) return fail("nnn_gate_apply: null %s", d_in ? "output" : "input");
    if (!d_vad) return fail("nnn_gate_apply: null vad");
    if (n_frames < 1) return fail("nnn_gate_apply: n_frames = %d", n_frames);
    if ((long long)n_frames * h->S > 0x7fffffffll) return fail("nnn_gate_apply: %d frames of %d streams are more than a call holds", n_frames, h->S);
    if ((uintptr_t)d_vad & 3) return fail("nnn_gate_apply: the vad rows are not aligned to their 4-byte values");
    return 0;
}

extern "C" int nnn_gate_apply_device(nnn_gate *h, const float *d_in, float *d_out, const float *d_vad, const uint8_t *d_live, uint8_t *d_open,
                                     int n_frames, size_t stream_stride, size_t frame_stride, void *hip_stream)
{
    if (int rc = gate_call_ok(h, d_in, d_out, d_vad, n_frames)) return rc;
    if (frame_stride < (size_t)FRAME) return fail("nnn_gate_apply: frame_stride = %zu is below a frame's %d elements", frame_stride, FRAME);
    if (((uintptr_t)d_in | (uintptr_t)d_out) & 3) return fail("nnn_gate_apply: the audio is not aligned to its 4-byte samples");
    return gate_enqueue(h, PCM_F32, d_in, d_out, d_vad, d_live, d_open, n_frames, 1, stream_stride, frame_stride, hip_stream);
}

extern "C" int nnn_gate_apply_pcm_device(nnn_gate *h, const void *d_in, void *d_out, const float *d_vad, const uint8_t *d_live, uint8_t *d_open,
                                         int n_frames, const nnn_pcm_layout *layout, void *hip_stream)
{
    if (int rc = gate_call_ok(h, d_in, d_out, d_vad, n_frames)) return rc;
    if (!layout) return fail("nnn_gate_apply: null layout");
    const int fmt = layout->format, C = layout->channels;
    if (fmt != PCM_F32 && fmt != PCM_I16 && fmt != PCM_F32_UNIT) return fail("nnn_gate_apply: bad format %d", fmt);
    if (C < 1 || h->S % C) return fail("nnn_gate_apply: channels = %d does not divide the %d streams", C, h->S);
    if (layout->discard_first) return fail("nnn_gate_apply: discard_first must be 0");
    if (layout->frame_stride < (size_t)FRAME * C) return fail("nnn_gate_apply: frame_stride = %zu is below a frame's %d elements", layout->frame_stride, FRAME * C);
    if (((uintptr_t)d_in | (uintptr_t)d_out) & (fmt == PCM_I16 ? 1 : 3)) return fail("nnn_gate_apply: the audio is not aligned to its %d-byte samples", fmt == PCM_I16 ? 2 : 4);
    return gate_enqueue(h, fmt == PCM_I16 ? PCM_I16 : PCM_F32, d_in, d_out, d_vad, d_live, d_open, n_frames, C, layout->group_stride, layout->frame_stride,
                        hip_stream);
}

template <class T> static int gate_room(nnn_gate *h, T *&q, size_t &cap, size_t bytes)
{
    if (bytes <= cap) return 0;
    NNN_RT_LOCK;
    if (int rc = gate_drain(h)) return rc;
    HIPCHK(hipFree(q));
    q = nullptr, cap = 0;
    HIPCHK(hipMalloc((void **)&q, bytes));
    cap = bytes;
    return 0;
}

extern "C" int nnn_gate_apply_host(nnn_gate *h, const float *in, float *out, const float *vad, const uint8_t *live, uint8_t *open, int n_frames)
{
    if (int rc = gate_call_ok(h, in, out, vad, n_frames)) return rc;
    HIPCHK(hipSetDevice(h->device));
    const size_t S = (size_t)h->S, rows = (size_t)n_frames * S, per = (size_t)n_frames * FRAME;
    if (int rc = gate_room(h, h->h_audio, h->h_audio_cap, rows * FRAME * sizeof(float))) return rc;
    if (int rc = gate_room(h, h->h_vad, h->h_vad_cap, rows * sizeof(float))) return rc;
    if (live)
        if (int rc = gate_room(h, h->h_live, h->h_live_cap, S)) return rc;
    if (open)
        if (int rc = gate_room(h, h->h_open, h->h_open_cap, rows)) return rc;
    hipStream_t st = h->own_stream;
    if (h->have_last && h->last_stream != st) HIPCHK(hipStreamWaitEvent(st, h->ev_last, 0));   // (the staging may be an earlier call's until then)
    HIPCHK(hipMemcpyAsync(h->h_audio, in, rows * FRAME * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(h->h_vad, vad, rows * sizeof(float), hipMemcpyHostToDevice, st));
    if (live) HIPCHK(hipMemcpyAsync(h->h_live, live, S, hipMemcpyHostToDevice, st));
    if (int rc = gate_enqueue(h, PCM_F32, h->h_audio, h->h_audio, h->h_vad, live ? h->h_live : nullptr, open ? h->h_open : nullptr, n_frames, 1, per, FRAME, st))
        return rc;
    std::vector<unsigned char> op;
    if (!live) {
        HIPCHK(hipMemcpyAsync(out, h->h_audio, rows * FRAME * sizeof(float), hipMemcpyDeviceToHost, st));
        if (open) HIPCHK(hipMemcpyAsync(open, h->h_open, rows, hipMemcpyDeviceToHost, st));
    } else {
        for (size_t s = 0; s < S;) {   // the live streams' rows, a run of neighbours at a time
            if (!live[s]) { s++; continue; }
            size_t e = s;
            while (e < S && live[e]) e++;
            HIPCHK(hipMemcpyAsync(out + s * per, h->h_audio + s * per, (e - s) * per * sizeof(float), hipMemcpyDeviceToHost, st));
            s = e;
        }
        if (open) {
            op.resize(rows);
            HIPCHK(hipMemcpyAsync(op.data(), h->h_open, rows, hipMemcpyDeviceToHost, st));
        }
    }
    HIPCHK(hipStreamSynchronize(st));
    if (live && open)
        for (size_t t = 0; t < (size_t)n_frames; t++)
            for (size_t s = 0; s < S; s++)
                if (live[s]) open[t * S + s] = op[t * S + s];
    return 0;
}

// ---- state transfer -------------------------------------------------------------------------------------------------------------------------
struct GateRecord {   // the first 48 bytes of a record (include/nnn_gate.h)
    uint32_t magic, version, size;
    float threshold;
    int32_t grace, lookback;
    float level;
    int32_t since;
    uint32_t was_open;
    uint32_t zero[3];
};
static_assert(sizeof(GateRecord) == 48 && NNN_GATE_STATE_BYTES == 48 + GATE_HMAX * FRAME * 4, "");

extern "C" size_t nnn_gate_state_bytes(const nnn_gate *h)
{
    if (!h) { fail("null gate"); return 0; }
    return NNN_GATE_STATE_BYTES;
}

extern "C" int nnn_gate_export_streams(nnn_gate *h, const int *idx, int n, void *records, size_t bytes)
{
    if (!h) return fail("null gate");
    if (int rc = gate_streams(h, idx, n, false, "nnn_gate_export_streams")) return rc;
    if (n == 0) return 0;
    if (!records) return fail("nnn_gate_export_streams: null records");
    if (bytes < (size_t)n * NNN_GATE_STATE_BYTES) return fail("nnn_gate_export_streams: %zu bytes for %d records of %d", bytes, n, (int)NNN_GATE_STATE_BYTES);
    NNN_RT_LOCK;
    if (int rc = gate_drain(h)) return rc;
    std::vector<int> since((size_t)h->S), was((size_t)h->S);
    HIPCHK(hipMemcpy(since.data(), h->d_since, since.size() * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(was.data(), h->d_was, was.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++) {
        const size_t s = (size_t)(idx ? idx[i] : i);
        char *rec = (char *)records + (size_t)i * NNN_GATE_STATE_BYTES;
        memset(rec, 0, NNN_GATE_STATE_BYTES);
        const nnn_gate_params &p = h->par[s];
        GateRecord r = {NNN_GATE_STATE_MAGIC, NNN_GATE_STATE_VERSION, NNN_GATE_STATE_BYTES, p.threshold, p.grace, p.lookback, p.level, since[s],
                        (uint32_t)(was[s] != 0), {0, 0, 0}};
        memcpy(rec, &r, sizeof(r));
        if (p.lookback > 0)
            HIPCHK(hipMemcpy(rec + sizeof(r), h->d_hist + s * h->H * FRAME, (size_t)p.lookback * FRAME * sizeof(float), hipMemcpyDeviceToHost));
    }
    return 0;
}

extern "C" int nnn_gate_import_streams(nnn_gate *h, const int *idx, int n, const void *records, size_t bytes)
{
    const char *who = "nnn_gate_import_streams";
    if (!h) return fail("null gate");
    if (int rc = gate_streams(h, idx, n, true, who)) return rc;
    if (n == 0) return 0;
    if (!records) return fail("%s: null records", who);
    if (bytes < (size_t)n * NNN_GATE_STATE_BYTES) return fail("%s: %zu bytes for %d records of %d", who, bytes, n, (int)NNN_GATE_STATE_BYTES);
    std::vector<GateRecord> recs((size_t)n);
    for (int i = 0; i < n; i++) {
        GateRecord &r = recs[(size_t)i];
        memcpy(&r, (const char *)records + (size_t)i * NNN_GATE_STATE_BYTES, sizeof(r));
        if (r.magic != NNN_GATE_STATE_MAGIC) return fail("%s: record %d is not a gate record (magic 0x%08x)", who, i, r.magic);
        if (r.version != NNN_GATE_STATE_VERSION) return fail("%s: record %d has version %u, this library reads %d", who, i, r.version, NNN_GATE_STATE_VERSION);
        if (r.size != NNN_GATE_STATE_BYTES) return fail("%s: record %d says %u bytes, a record has %d", who, i, r.size, (int)NNN_GATE_STATE_BYTES);
        if (r.lookback > h->H && r.lookback <= NNN_GATE_MAX_LOOKBACK)
            return fail("%s: record %d has lookback %d, this object's max_lookback is %d", who, i, (int)r.lookback, h->H);
        const nnn_gate_params p = {r.threshold, r.grace, r.lookback, r.level};
        if (int rc = gate_params_ok(p, h->H, i, who)) return rc;
        if (r.since < 0 || r.was_open > 1u) return fail("%s: record %d has a state no gate reaches (since %d, was_open %u)", who, i, (int)r.since, r.was_open);
    }
    NNN_RT_LOCK;
    if (int rc = gate_drain(h)) return rc;
    std::vector<int> since((size_t)h->S), was((size_t)h->S);
    HIPCHK(hipMemcpy(since.data(), h->d_since, since.size() * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(was.data(), h->d_was, was.size() * sizeof(int), hipMemcpyDeviceToHost));
    std::vector<float> rows((size_t)h->H * FRAME);
    for (int i = 0; i < n; i++) {
        const size_t s = (size_t)(idx ? idx[i] : i);
        const GateRecord &r = recs[(size_t)i];
        h->par[s] = nnn_gate_params{r.threshold, r.grace, r.lookback, r.level};
        since[s] = r.since, was[s] = (int)r.was_open;
        if (h->H > 0) {
            std::fill(rows.begin(), rows.end(), 0.0f);
            memcpy(rows.data(), (const char *)records + (size_t)i * NNN_GATE_STATE_BYTES + sizeof(r), (size_t)r.lookback * FRAME * sizeof(float));
            HIPCHK(hipMemcpy(h->d_hist + s * h->H * FRAME, rows.data(), rows.size() * sizeof(float), hipMemcpyHostToDevice));
        }
    }
    HIPCHK(hipMemcpy(h->d_since, since.data(), since.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_was, was.data(), was.size() * sizeof(int), hipMemcpyHostToDevice));
    return gate_upload_params(h);
}
