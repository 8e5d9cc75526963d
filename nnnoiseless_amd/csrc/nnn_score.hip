// nnn_score.hip -- the scorer (include/nnn_score.h): per-stream sums A, B, C, E between a reference and a test signal,
// carried across calls.  One call = k_score (a wave per stream and run of frames: each frame's four sums, in the header's order) and
// k_score_fold (a wave per stream: the call's frame sums into the totals in frame order, the call's last samples into the history), on the
// caller's stream.
// Needs fail / HIPCHK / NNN_RT_LOCK (nnn_batch_core.hip).
#pragma once

#include "../../include/nnn_score.h"

// ---- the kernels ------------------------------------------------------------------------------------------------------------------------
constexpr int SCORE_WAVES = 4;                        // waves (streams) per block of both kernels
constexpr int SCORE_RUN = 4;                          // consecutive frames of its stream a wave of k_score takes
constexpr int SCORE_TERMS = (FRAME + 63) / 64;        // 8: lane L owns samples L + 64 k
static_assert(FRAME == NNN_SCORE_FRAME && NNN_SCORE_MAX_DELAY == 2 * FRAME && NNN_SCORE_SUMS == 4, "");

struct ScoreArgs {
    const float *ref, *test;          // sample i of frame f of stream s at s * ss + f * fs + i
    const unsigned char *valid;       // NULL or [T][S]
    double *fsum;                     // [T][S][4]
    const float *hist;                // [S][HL]: sample n < 0 (counted from the call's first sample) of stream s at s * HL + HL + n
    const int *delay;                 // [S]
    long long ss, fs;
    int S, T, HL;
};

// where sample n of a stream lies (n counted from the call's first sample; n >= -HL): in one of the call's frames or in the history
__device__ __forceinline__ const float *score_at(const float *rs, const float *hs, long long fs, int n)
{
    return n >= 0 ? rs + (long long)(n / FRAME) * fs + n % FRAME : hs + n;
}

// one frame of a stream as the lanes hold it: lane L has samples L + 64 k of the test frame and of the reference window
struct ScoreFrame { float r[SCORE_TERMS], y[SCORE_TERMS]; };

// Frame f's loads.  ts / rs: the stream's first test / reference sample of the call; hs: where the call's sample 0 would lie in the history
// row; dq = ceil(delay / 480) and rem = dq * 480 - delay say where the window begins: sample `rem` of frame f - dq.  A window covers at
// most two frames, each one of the call's (wherever frame_stride puts it) or, before the call's first, 480 contiguous floats of the
// history.  Every instruction fetches 64 consecutive floats, or two runs where the window crosses into its second frame.
__device__ __forceinline__ void score_load(const ScoreArgs &a, const float *ts, const float *rs, const float *hs, int f, int dq, int rem, int lane, ScoreFrame &v)
{
    const float *tp = ts + (long long)f * a.fs;
    const int q0 = f - dq;
    const float *w0 = q0 >= 0 ? rs + (long long)q0 * a.fs : hs + (long long)q0 * FRAME;
    const float *w1 = q0 + 1 >= 0 ? rs + (long long)(q0 + 1) * a.fs : hs + (long long)(q0 + 1) * FRAME;
#pragma unroll
    for (int k = 0; k < SCORE_TERMS; k++) {
        const int i = lane + 64 * k, j = rem + i;
        v.r[k] = v.y[k] = 0.0f;
        if (i < FRAME) {
            v.y[k] = ld_global<float>(tp + i);
            v.r[k] = ld_global<float>(j < FRAME ? w0 + j : w1 + (j - FRAME));
        }
    }
}

// the header's arithmetic on a loaded frame; lane 0 stores the four sums
__device__ __forceinline__ void score_sums(const ScoreFrame &v, int lane, double *out)
{
#pragma clang fp contract(off)
    // step 1: this lane's partial sums over its samples in ascending order
    double A = 0.0, B = 0.0, C = 0.0, E = 0.0;
#pragma unroll
    for (int k = 0; k < SCORE_TERMS; k++) {
        if (lane + 64 * k < FRAME) {
            const double rd = (double)v.r[k], yd = (double)v.y[k];
            const double df = rd - yd;
            A = A + rd * rd;
            B = B + yd * yd;
            C = C + rd * yd;
            E = E + df * df;
        }
    }
    // step 2: p_L <- p_L + p_(L xor m), m = 32 .. 1
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        A = A + __shfl_xor(A, m);
        B = B + __shfl_xor(B, m);
        C = C + __shfl_xor(C, m);
        E = E + __shfl_xor(E, m);
    }
    if (lane == 0) out[0] = A, out[1] = B, out[2] = C, out[3] = E;
}

// A wave per stream (blockIdx.x) and run of SCORE_RUN consecutive frames (blockIdx.y, striding over the runs where the call has more
// of them than a grid has rows).  Lane L loads samples L + 64 k themselves, the assignment the summation order is stated in, so nothing
// crosses lanes before the tree; the next frame's sixteen loads are issued before the current frame's arithmetic and land behind it.
// (A variant that fetched 16 bytes a lane and turned the frame round in LDS ran at 0.86 of this one's rate: DESIGN.md section 23.)
__global__ void __launch_bounds__(64 * SCORE_WAVES) k_score(ScoreArgs a)
{
    const int lane = threadIdx.x & 63, s = blockIdx.x * SCORE_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (s >= a.S) return;                                              // (whole waves; the kernel has no block barrier)
    const int d = ld_global<int>(a.delay + s);
    const int dq = (d + FRAME - 1) / FRAME, rem = dq * FRAME - d;
    const float *ts = a.test + (long long)s * a.ss, *rs = a.ref + (long long)s * a.ss, *hs = a.hist + (size_t)s * a.HL + a.HL;
    const int runs = (a.T + SCORE_RUN - 1) / SCORE_RUN;
    for (int run = blockIdx.y; run < runs; run += gridDim.y) {
        const int f0 = run * SCORE_RUN;
        ScoreFrame v[2];
        bool on = !a.valid || ld_global<unsigned char>(a.valid + (size_t)f0 * a.S + s) != 0;
        if (on) score_load(a, ts, rs, hs, f0, dq, rem, lane, v[0]);
#pragma unroll
        for (int j = 0; j < SCORE_RUN; j++) {
            const int f = f0 + j;
            if (f < a.T) {
                const bool on_next = j + 1 < SCORE_RUN && f + 1 < a.T && (!a.valid || ld_global<unsigned char>(a.valid + (size_t)(f + 1) * a.S + s) != 0);
                if (on_next) score_load(a, ts, rs, hs, f + 1, dq, rem, lane, v[(j + 1) & 1]);
                double *out = a.fsum + ((size_t)f * a.S + s) * 4;
                if (on) score_sums(v[j & 1], lane, out);
                else if (lane < 4) out[lane] = 0.0;
                on = on_next;
            }
        }
    }
}

struct ScoreFoldArgs {
    const float *ref;
    const unsigned char *valid;
    const double *fsum;               // [T][S][4]
    const float *hist_in;             // [S][HL]: the history the call began with
    float *hist_out;                  // the other buffer: the history the next call begins with
    double *tot;                      // [S][4]
    unsigned long long *cnt;          // [S]
    long long ss, fs;
    int S, T, HL;
};

// One wave per stream, behind k_score on the same stream.  Lanes 0 .. 3 add the call's frame sums to one total each, in frame order,
// frames marked 0 left out; every lane moves the last HL samples before the call's end into the new history -- from the call's frames,
// or from the old history where the call is shorter than that.
__global__ void __launch_bounds__(64 * SCORE_WAVES) k_score_fold(ScoreFoldArgs a)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, s = blockIdx.x * SCORE_WAVES + (int)(threadIdx.x >> 6);
    if (s >= a.S) return;
    if (lane < 4) {
        double t = a.tot[(size_t)s * 4 + lane];
        unsigned long long c = a.cnt[s];
        for (int f = 0; f < a.T; f++) {
            const size_t at = (size_t)f * a.S + s;
            if (!a.valid || a.valid[at]) {
                t = t + a.fsum[at * 4 + lane];
                c++;
            }
        }
        a.tot[(size_t)s * 4 + lane] = t;
        if (lane == 0) a.cnt[s] = c;
    }
    const float *rs = a.ref + (long long)s * a.ss, *hs = a.hist_in + (size_t)s * a.HL + a.HL;
    float *ho = a.hist_out + (size_t)s * a.HL;
    const long long N = (long long)a.T * FRAME;   // (n below fits an int: the host refuses calls of 2^31 samples a stream)
    for (int j = lane; j < a.HL; j += 64) ho[j] = *score_at(rs, hs, a.fs, (int)(N - a.HL + j));
}

// history, totals and count of the flagged streams to zero (a wave per stream)
__global__ void __launch_bounds__(64 * SCORE_WAVES) k_score_clear(const unsigned char *flag, float *hist, double *tot, unsigned long long *cnt, int S, int HL)
{
    const int lane = threadIdx.x & 63, s = blockIdx.x * SCORE_WAVES + (int)(threadIdx.x >> 6);
    if (s >= S || !flag[s]) return;
    for (int j = lane; j < HL; j += 64) hist[(size_t)s * HL + j] = 0.0f;
    if (lane < 4) tot[(size_t)s * 4 + lane] = 0.0;
    if (lane == 0) cnt[s] = 0ull;
}

// ---- the host side ------------------------------------------------------------------------------------------------------------------------
struct nnn_score {
    int S = 0, max_delay = 0, HL = 0, device = 0;   // HL = max_delay: the history's row length
    std::vector<int32_t> delay;                     // as the host set them; d_delay is their copy
    int32_t *d_delay = nullptr;
    float *d_hist[2] = {nullptr, nullptr};          // [S][HL] each; cur says which one the next call reads
    int cur = 0;
    double *d_tot = nullptr;                        // [S][4]
    unsigned long long *d_cnt = nullptr;            // [S]
    unsigned char *d_flag = nullptr;                // [S]: the streams a reset names
    double *d_fsum = nullptr;                       // the frame sums of a call that hands in no table (grow only)
    size_t fsum_cap = 0;
    hipStream_t own_stream = nullptr;
    hipEvent_t ev_last = nullptr;                   // end of the most recent call, on the stream it was made on
    hipStream_t last_stream = nullptr;
    bool have_last = false;
    // device buffers of the host entry point (made on first use, grow only)
    float *h_audio = nullptr;
    unsigned char *h_valid = nullptr;
    double *h_fsum = nullptr;
    size_t h_audio_cap = 0, h_valid_cap = 0, h_fsum_cap = 0;   // bytes
};

extern "C" void nnn_score_destroy(nnn_score *h)
{
    if (!h) return;
    NNN_RT_LOCK;
    hipSetDevice(h->device);
    if (h->have_last) hipEventSynchronize(h->ev_last);
    hipFree(h->d_delay); hipFree(h->d_hist[0]); hipFree(h->d_hist[1]); hipFree(h->d_tot); hipFree(h->d_cnt); hipFree(h->d_flag); hipFree(h->d_fsum);
    hipFree(h->h_audio); hipFree(h->h_valid); hipFree(h->h_fsum);
    if (h->own_stream) hipStreamDestroy(h->own_stream);
    if (h->ev_last) hipEventDestroy(h->ev_last);
    delete h;
}

extern "C" nnn_score *nnn_score_create(int n_streams, int max_delay, int device)
{
    if (n_streams < 1) { fail("nnn_score_create: n_streams = %d", n_streams); return nullptr; }
    if (max_delay < 0 || max_delay > NNN_SCORE_MAX_DELAY) { fail("nnn_score_create: max_delay = %d outside [0, %d]", max_delay, NNN_SCORE_MAX_DELAY); return nullptr; }
    NNN_RT_LOCK;
    if (hipSetDevice(device) != hipSuccess) { fail("nnn_score_create: no such HIP device"); return nullptr; }
    nnn_score *h = new nnn_score();
    h->S = n_streams, h->max_delay = max_delay, h->HL = max_delay, h->device = device;
    h->delay.assign((size_t)n_streams, 0);
    const size_t S = (size_t)n_streams, hist = (S * h->HL ? S * h->HL : 4) * sizeof(float);
    bool ok = true;
    auto dev = [&](auto **q, size_t bytes) { ok = ok && hipMalloc((void **)q, bytes) == hipSuccess && hipMemset(*q, 0, bytes) == hipSuccess; };
    dev(&h->d_delay, S * sizeof(int32_t));
    dev(&h->d_hist[0], hist), dev(&h->d_hist[1], hist);
    dev(&h->d_tot, S * 4 * sizeof(double));
    dev(&h->d_cnt, S * sizeof(unsigned long long));
    dev(&h->d_flag, S);
    ok = ok && hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&h->ev_last, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipDeviceSynchronize() == hipSuccess;   // (the memsets above are on the legacy stream; the calls are on non-blocking ones)
    if (!ok) {
        nnn_score_destroy(h);
        fail("nnn_score_create: allocation failed (%d bytes for each of %d streams)", 8 * max_delay + 45, n_streams);
        return nullptr;
    }
    return h;
}

// everything enqueued so far is done
static int score_drain(nnn_score *h)
{
    HIPCHK(hipSetDevice(h->device));
    if (h->have_last) HIPCHK(hipEventSynchronize(h->ev_last));
    return 0;
}

static int score_streams(const nnn_score *h, const int *idx, int n, const char *who)
{
    if (n < 0) return fail("%s: n = %d", who, n);
    if (!idx && n > h->S) return fail("%s: %d entries for %d streams", who, n, h->S);
    for (int i = 0; idx && i < n; i++)
        if (idx[i] < 0 || idx[i] >= h->S) return fail("%s: stream %d outside [0, %d)", who, idx[i], h->S);
    return 0;
}

// zero the listed streams (idx == NULL: streams 0 .. n - 1); the caller holds the lock and has drained the object
static int score_clear(nnn_score *h, const int *idx, int n)
{
    std::vector<unsigned char> flag((size_t)h->S, 0);
    for (int i = 0; i < n; i++) flag[(size_t)(idx ? idx[i] : i)] = 1;
    HIPCHK(hipMemcpy(h->d_flag, flag.data(), flag.size(), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_score_clear, dim3((unsigned)((h->S + SCORE_WAVES - 1) / SCORE_WAVES)), dim3(64 * SCORE_WAVES), 0, h->own_stream,
                       (const unsigned char *)h->d_flag, h->d_hist[h->cur], h->d_tot, h->d_cnt, h->S, h->HL);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->own_stream));
    return 0;
}

extern "C" int nnn_score_set_delay(nnn_score *h, const int *idx, int n, const int32_t *delays)
{
    if (!h) return fail("null scorer");
    if (int rc = score_streams(h, idx, n, "nnn_score_set_delay")) return rc;
    if (n == 0) return 0;
    if (!delays) return fail("nnn_score_set_delay: null delays");
    for (int i = 0; i < n; i++)
        if (delays[i] < 0 || delays[i] > h->max_delay) return fail("nnn_score_set_delay: entry %d: delay %d outside [0, %d]", i, (int)delays[i], h->max_delay);
    NNN_RT_LOCK;
    if (int rc = score_drain(h)) return rc;
    for (int i = 0; i < n; i++) h->delay[(size_t)(idx ? idx[i] : i)] = delays[i];
    HIPCHK(hipMemcpy(h->d_delay, h->delay.data(), h->delay.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    return score_clear(h, idx, n);
}

extern "C" int nnn_score_get_delay(nnn_score *h, const int *idx, int n, int32_t *delays)
{
    if (!h) return fail("null scorer");
    if (int rc = score_streams(h, idx, n, "nnn_score_get_delay")) return rc;
    if (n == 0) return 0;
    if (!delays) return fail("nnn_score_get_delay: null delays");
    for (int i = 0; i < n; i++) delays[i] = h->delay[(size_t)(idx ? idx[i] : i)];
    return 0;
}

extern "C" int nnn_score_reset(nnn_score *h, const int *idx, int n)
{
    if (!h) return fail("null scorer");
    if (!idx) n = h->S;
    if (int rc = score_streams(h, idx, n, "nnn_score_reset")) return rc;
    if (n == 0) return 0;
    NNN_RT_LOCK;
    if (int rc = score_drain(h)) return rc;
    return score_clear(h, idx, n);
}

extern "C" int nnn_score_accumulate_device(nnn_score *h, const float *d_ref, const float *d_test, const uint8_t *d_valid, double *d_frame_sums,
                                           int n_frames, size_t stream_stride, size_t frame_stride, void *hip_stream)
{
    if (!h) return fail("null scorer");
    if (!d_ref || !d_test) return fail("nnn_score_accumulate: null %s signal", d_ref ? "test" : "reference");
    if (n_frames < 1) return fail("nnn_score_accumulate: n_frames = %d", n_frames);
    if ((long long)n_frames * FRAME > 0x7fffffffll || (long long)n_frames * h->S > 0x7fffffffll)
        return fail("nnn_score_accumulate: %d frames of %d streams are more than a call holds", n_frames, h->S);
    if (((uintptr_t)d_ref | (uintptr_t)d_test) & 3) return fail("nnn_score_accumulate: the signals are not aligned to their 4-byte samples");
    if (d_frame_sums && ((uintptr_t)d_frame_sums & 7)) return fail("nnn_score_accumulate: the frame sums are not aligned to their 8-byte values");
    HIPCHK(hipSetDevice(h->device));
    const size_t rows = (size_t)n_frames * h->S;
    double *fsum = d_frame_sums;
    if (!fsum) {
        if (rows * 4 * sizeof(double) > h->fsum_cap) {
            NNN_RT_LOCK;
            if (int rc = score_drain(h)) return rc;
            HIPCHK(hipFree(h->d_fsum));
            h->d_fsum = nullptr, h->fsum_cap = 0;
            HIPCHK(hipMalloc((void **)&h->d_fsum, rows * 4 * sizeof(double)));
            h->fsum_cap = rows * 4 * sizeof(double);
        }
        fsum = h->d_fsum;
    }
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : h->own_stream;
    if (h->have_last && h->last_stream != st) HIPCHK(hipStreamWaitEvent(st, h->ev_last, 0));   // (history and totals are the previous call's until then)
    ScoreArgs a = {};
    a.ref = d_ref, a.test = d_test, a.valid = d_valid, a.fsum = fsum, a.hist = h->d_hist[h->cur], a.delay = h->d_delay;
    a.ss = (long long)stream_stride, a.fs = (long long)frame_stride;
    a.S = h->S, a.T = n_frames, a.HL = h->HL;
    const unsigned sblocks = (unsigned)((h->S + SCORE_WAVES - 1) / SCORE_WAVES), runs = (unsigned)((n_frames + SCORE_RUN - 1) / SCORE_RUN);
    const dim3 block(64 * SCORE_WAVES);
    hipLaunchKernelGGL(k_score, dim3(sblocks, runs < 65535u ? runs : 65535u), block, 0, st, a);
    ScoreFoldArgs g = {};
    g.ref = d_ref, g.valid = d_valid, g.fsum = fsum, g.hist_in = h->d_hist[h->cur], g.hist_out = h->d_hist[h->cur ^ 1], g.tot = h->d_tot, g.cnt = h->d_cnt;
    g.ss = a.ss, g.fs = a.fs, g.S = h->S, g.T = n_frames, g.HL = h->HL;
    hipLaunchKernelGGL(k_score_fold, dim3(sblocks), block, 0, st, g);
    h->cur ^= 1;
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev_last, st));
    h->last_stream = st;
    h->have_last = true;
    return 0;
}

template <class T> static int score_room(nnn_score *h, T *&q, size_t &cap, size_t bytes)
{
    if (bytes <= cap) return 0;
    NNN_RT_LOCK;
    if (int rc = score_drain(h)) return rc;
    HIPCHK(hipFree(q));
    q = nullptr, cap = 0;
    HIPCHK(hipMalloc((void **)&q, bytes));
    cap = bytes;
    return 0;
}

extern "C" int nnn_score_accumulate_host(nnn_score *h, const float *ref, const float *test, const uint8_t *valid, double *frame_sums, int n_frames)
{
    if (!h) return fail("null scorer");
    if (!ref || !test) return fail("nnn_score_accumulate: null %s signal", ref ? "test" : "reference");
    if (n_frames < 1) return fail("nnn_score_accumulate: n_frames = %d", n_frames);
    HIPCHK(hipSetDevice(h->device));
    const size_t rows = (size_t)n_frames * h->S, na = rows * FRAME;
    if (int rc = score_room(h, h->h_audio, h->h_audio_cap, 2 * na * sizeof(float))) return rc;
    if (valid)
        if (int rc = score_room(h, h->h_valid, h->h_valid_cap, rows)) return rc;
    if (frame_sums)
        if (int rc = score_room(h, h->h_fsum, h->h_fsum_cap, rows * 4 * sizeof(double))) return rc;
    hipStream_t st = h->own_stream;
    if (h->have_last && h->last_stream != st) HIPCHK(hipStreamWaitEvent(st, h->ev_last, 0));   // (the staging may be an earlier call's until then)
    HIPCHK(hipMemcpyAsync(h->h_audio, ref, na * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(h->h_audio + na, test, na * sizeof(float), hipMemcpyHostToDevice, st));
    if (valid) HIPCHK(hipMemcpyAsync(h->h_valid, valid, rows, hipMemcpyHostToDevice, st));
    if (int rc = nnn_score_accumulate_device(h, h->h_audio, h->h_audio + na, valid ? h->h_valid : nullptr, frame_sums ? h->h_fsum : nullptr, n_frames,
                                             (size_t)n_frames * FRAME, FRAME, st))
        return rc;
    if (frame_sums) HIPCHK(hipMemcpyAsync(frame_sums, h->h_fsum, rows * 4 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

extern "C" int nnn_score_totals(nnn_score *h, double *out, uint64_t *counts)
{
    if (!h) return fail("null scorer");
    NNN_RT_LOCK;
    if (int rc = score_drain(h)) return rc;
    if (out) HIPCHK(hipMemcpy(out, h->d_tot, (size_t)h->S * 4 * sizeof(double), hipMemcpyDeviceToHost));
    if (counts) HIPCHK(hipMemcpy(counts, h->d_cnt, (size_t)h->S * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int nnn_score_totals_device(nnn_score *h, double *d_out, uint64_t *d_counts, void *hip_stream)
{
    if (!h) return fail("null scorer");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : h->own_stream;
    if (h->have_last && h->last_stream != st) HIPCHK(hipStreamWaitEvent(st, h->ev_last, 0));
    if (d_out) HIPCHK(hipMemcpyAsync(d_out, h->d_tot, (size_t)h->S * 4 * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (d_counts) HIPCHK(hipMemcpyAsync(d_counts, h->d_cnt, (size_t)h->S * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    HIPCHK(hipEventRecord(h->ev_last, st));   // (the next call's fold overwrites the totals: it must come behind this copy)
    h->last_stream = st;
    h->have_last = true;
    return 0;
}
