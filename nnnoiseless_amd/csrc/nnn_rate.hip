// nnn_rate.hip -- the rate adapter (include/nnn_rate.h): streams at another sample rate in and out of a batch.  One
// call = k_rate_in (source rate -> 48 kHz, behind the carried partial frame) -> the batch's ordinary call over the whole frames ->
// k_rate_out (48 kHz -> source rate), all on the caller's stream, with no synchronisation.
// Needs struct nnn_batch, fail / HIPCHK, refuse_pending and report_fault (nnn_batch_core.hip), nnn_batch_process_device (nnn_batch_launch.hip)
// and the PCM conversions (nnn_common.hip); the schedule, the weights and the fold are nnn_rs_sched.h's, shared with nnn_resample.hip.
// ref: src/nnnoiseless.rs:106-131 (Resample<RS>), :179-227 (the CLI resamples, then denoises).
#pragma once

#include <algorithm>

#include "../../include/nnn_rate.h"
#include "nnn_rs_sched.h"

// ---- the two kernels ---------------------------------------------------------------------------------------------------------------
// A block of 256 threads covers one SPAN of 64 consecutive outputs for `nsb` streams.  What depends on the output alone -- sixteen f64
// weights and a schedule entry each, 144 bytes -- is staged in LDS once per block and reused by all its streams (each thread keeps the
// weights of its output in registers across its streams); the source window of the span (the samples from 16 before its first output's
// ring to its last output's newest, span * ratio + 16 or so) is read once per stream, so neighbouring outputs do not fetch their
// fifteen shared samples again.
//   LDS:  wl   [16][65] f64   weight k of output m at wl[k * 65 + m]: lane = output, so a wave's ds_read_b64 covers 64 consecutive
//                             doubles -- 256 contiguous bytes per 32-lane half, every bank once, conflict-free; the odd row length
//                             spreads the transposing writes of the staging (lanes k, k + 1, ... of one output) over the banks
//         cons [64] i32       where output m's ring starts in the window;  meta [64] i32  idx | nd << 8
//         win  [nsb][win] f32 a wave works on one stream at a time: its lanes read 16 floats each from offsets that grow by the
//                             schedule's step (0 or 1 going up in rate: broadcasts and neighbours, conflict-free)
// Block 0 of a stream group also writes the streams' next history (the other buffer of a pair: the other blocks still read this call's)
// and, in k_rate_in, moves the carried partial frame in front of the new samples.
constexpr int RT_SPAN = 64, RT_THREADS = 256, RT_WROW = RT_SPAN + 1;
constexpr int RT_CLEAR = 1, RT_SKIP = 2;   // per-stream flag bits: histories and carried samples read as zero; the stream sits the call out

struct RateLegArgs {
    const void *in;                 // k_rate_in: the caller's rows (FMT); k_rate_out: the staging (f32)
    long long in_stride;            // elements
    long n_in;
    const float *hist_old;          // [S][16]: the 16 source samples before this call's
    float *hist_new;
    const RsOut *sched;             // the leg's table for this call
    const double *w;
    int n_out;
    void *out;                      // k_rate_in: the staging (f32); k_rate_out: the caller's rows (FMT)
    long long out_stride;
    const float *carry_old;         // k_rate_in: [S][480] the partial frame carried into / out of this call
    float *carry_new;
    int carried;                    // samples in carry_old
    long split;                     // k_rate_in: 48 kHz sample j of the call (carried ones first) goes to the staging if j < split, else to
                                    // carry_new[j - split]: split = 480 * the frames the call completes
    const unsigned char *flags;     // [S] RT_CLEAR | RT_SKIP (MASK instantiations only)
    int n_streams, nsb, win;        // streams per block, floats per stream in `win`
};

template <bool UP, int FMT, bool MASK> __device__ __forceinline__ float rate_load(const RateLegArgs &a, int s, long p, int f)
{
    if (MASK && (f & RT_SKIP)) return 0.0f;
    if (p >= 0) {
        if (UP && FMT == PCM_I16) return (float)((const short *)a.in)[(long long)s * a.in_stride + p];
        return ((const float *)a.in)[(long long)s * a.in_stride + p];
    }
    if (MASK && (f & RT_CLEAR)) return 0.0f;
    return a.hist_old[(size_t)s * RS_TAPS + (RS_TAPS + p)];
}

template <bool UP, int FMT, bool MASK> __device__ __forceinline__ void rate_store(const RateLegArgs &a, int s, long j, float v, int f)
{
    if (UP) {
        if (j < a.split) ((float *)a.out)[(long long)s * a.out_stride + j] = v;
        else a.carry_new[(size_t)s * FRAME + (j - a.split)] = v;
        return;
    }
    if (MASK && (f & RT_SKIP)) return;
    if (FMT == PCM_I16) ((short *)a.out)[(long long)s * a.out_stride + j] = pcm_to_i16(v);
    else ((float *)a.out)[(long long)s * a.out_stride + j] = v;
}

template <bool UP, int FMT, bool MASK> __device__ __forceinline__ void rate_leg(const RateLegArgs &a)
{
    HIP_DYNAMIC_SHARED(double, rate_lds)
    double *wl = rate_lds;
    int *cons = (int *)(wl + RS_TAPS * RT_WROW);
    int *meta = cons + RT_SPAN;
    float *win = (float *)(meta + RT_SPAN);
    const int tid = threadIdx.x;
    const int m0 = blockIdx.x * RT_SPAN, s0 = blockIdx.y * a.nsb;
    const int left = a.n_out - m0, nm = left < RT_SPAN ? left : RT_SPAN;   // (<= 0: a call that completes no output still moves the histories)
    int p0 = 0, wlen = 0;
    if (nm > 0) {
        p0 = a.sched[m0].consumed - RS_TAPS;
        wlen = a.sched[m0 + nm - 1].consumed - p0;
    }
    if (blockIdx.x == 0) {
        for (int sb = 0; sb < a.nsb; sb += RT_THREADS / RS_TAPS) {
            const int sl = sb + (tid >> 4), s = s0 + sl, i = tid & 15;
            if (sl < a.nsb && s < a.n_streams) {
                const int f = MASK ? a.flags[s] : 0;
                a.hist_new[(size_t)s * RS_TAPS + i] = rate_load<UP, FMT, MASK>(a, s, a.n_in - RS_TAPS + i, f);
                if (UP)
                    for (int j = i; j < a.carried; j += RS_TAPS)
                        rate_store<UP, FMT, MASK>(a, s, j, (MASK && f) ? 0.0f : a.carry_old[(size_t)s * FRAME + j], 0);
            }
        }
    }
    for (int g = tid; g < nm * RS_TAPS; g += RT_THREADS) wl[(g & 15) * RT_WROW + (g >> 4)] = a.w[(size_t)m0 * RS_TAPS + g];
    if (tid < nm) {
        const RsOut o = a.sched[m0 + tid];
        cons[tid] = o.consumed - RS_TAPS - p0;
        meta[tid] = o.idx | (o.nd << 8);
    }
    for (int sb = 0; sb < a.nsb; sb += RT_THREADS / RS_TAPS) {
        const int sl = sb + (tid >> 4), s = s0 + sl;
        if (sl < a.nsb && s < a.n_streams) {
            const int f = MASK ? a.flags[s] : 0;
            for (int i = tid & 15; i < wlen; i += RS_TAPS) win[sl * a.win + i] = rate_load<UP, FMT, MASK>(a, s, (long)p0 + i, f);
        }
    }
    __syncthreads();
    const int m = tid & (RT_SPAN - 1);
    if (m < nm) {
        double wr[RS_TAPS];
#pragma unroll
        for (int k = 0; k < RS_TAPS; k++) wr[k] = wl[k * RT_WROW + m];
        const int c = cons[m], idx = meta[m] & 255, nd = meta[m] >> 8;
        for (int sl = tid >> 6; sl < a.nsb; sl += RT_THREADS / RT_SPAN) {
            const int s = s0 + sl;
            if (s >= a.n_streams) break;
            const int f = MASK ? a.flags[s] : 0;
            rate_store<UP, FMT, MASK>(a, s, (long)a.carried + m0 + m, sinc_fold<true>(win + sl * a.win + c, wr, nd, idx), f);
        }
    }
}

template <int FMT, bool MASK> __global__ void __launch_bounds__(RT_THREADS) k_rate_in(RateLegArgs a) { rate_leg<true, FMT, MASK>(a); }
template <int FMT, bool MASK> __global__ void __launch_bounds__(RT_THREADS) k_rate_out(RateLegArgs a) { rate_leg<false, FMT, MASK>(a); }

// ---- the host side -----------------------------------------------------------------------------------------------------------------
constexpr int RT_MEMO = 4;   // tables a leg keeps resident on the device
constexpr int RT_PIN = 4;    // page-locked upload slots: a slot is written again only after its event says the copies out of it are done

struct RateLeg {
    double ratio = 1.0;
    RsPos pos;                      // as of the calls made so far
    float *hist[2] = {};            // device [S][16], the pair k_rate_* alternate between
    int par = 0;                    // hist[par] is the current one
    long cap = 0;                   // outputs a table holds
    int win = 0, nsb = 0;
    size_t lds = 0;
    struct Memo {                   // a resident table and its key: the schedule is a pure function of (position bits, idx, credit, n_in)
        bool valid = false;
        uint64_t pos_bits = 0, used = 0;
        int idx = 0;
        long credit = 0, n_in = 0, n_out = 0;
        RsPos after;
        RsOut *sched = nullptr;     // device
        double *w = nullptr;
    } memo[RT_MEMO];
    long built = 0;
    double build_us = 0.0;
};

struct nnn_rate {
    nnn_batch *b = nullptr;
    int S = 0, device = 0;          // (its own copy: destroy must not look into a batch that may be gone)
    long max_in = 0;
    RateLeg leg[2];                 // [0] up: source rate -> 48 kHz, [1] down
    float *stage = nullptr;         // device [S][stage_stride]: the whole frames of a call, denoised in place
    long stage_stride = 0;
    float *carry[2] = {};           // device [S][480], a pair like the histories
    int carry_par = 0;
    long carried = 0;
    unsigned char *flags = nullptr; // device [S]
    std::vector<unsigned char> reset_mark;   // streams nnn_rate_reset_streams listed since the last call
    int n_reset = 0;
    struct Pin {
        char *p = nullptr;          // page-locked: the up-leg's table, the down-leg's table, the flags
        hipEvent_t ev = nullptr;
        bool busy = false;
    } pin[RT_PIN];
    size_t pin_off[3] = {};
    int pin_next = 0;
    uint64_t tick = 0;
    hipEvent_t ev_last = nullptr;   // end of the most recent call, on the stream it was made on
    hipStream_t last_stream = nullptr;
    bool have_last = false;
    char *h_in = nullptr, *h_out = nullptr;   // device staging of the host variant (made on first use)
    float *h_vad = nullptr;
    size_t h_in_cap = 0, h_out_cap = 0, h_vad_cap = 0;
};

static size_t rate_lds_bytes(int nsb, int win) { return (size_t)RS_TAPS * RT_WROW * sizeof(double) + 2 * RT_SPAN * sizeof(int) + (size_t)nsb * win * sizeof(float); }

extern "C" void nnn_rate_destroy(nnn_rate *a)
{
    if (!a) return;
    NNN_RT_LOCK;
    hipSetDevice(a->device);
    if (a->have_last) hipEventSynchronize(a->ev_last);
    for (auto &p : a->pin) {
        if (p.busy) hipEventSynchronize(p.ev);
        if (p.p) hipHostFree(p.p);
        if (p.ev) hipEventDestroy(p.ev);
    }
    for (auto &l : a->leg) {
        hipFree(l.hist[0]); hipFree(l.hist[1]);
        for (auto &m : l.memo) { hipFree(m.sched); hipFree(m.w); }
    }
    hipFree(a->stage); hipFree(a->carry[0]); hipFree(a->carry[1]); hipFree(a->flags);
    hipFree(a->h_in); hipFree(a->h_out); hipFree(a->h_vad);
    if (a->ev_last) hipEventDestroy(a->ev_last);
    delete a;
}

extern "C" long nnn_rate_max_output(const nnn_rate *a, long n_in)
{
    return a ? rs_max_output(a->leg[1].ratio, (long)nnn_rate_max_frames(a, n_in) * FRAME) : 0;
}
extern "C" int nnn_rate_max_frames(const nnn_rate *a, long n_in)
{
    return a ? (int)((FRAME - 1 + rs_max_output(a->leg[0].ratio, n_in < 0 ? 0 : n_in)) / FRAME) : 0;
}
extern "C" long nnn_rate_carried(const nnn_rate *a) { return a ? a->carried : 0; }

extern "C" nnn_rate *nnn_rate_create(nnn_batch *b, double source_rate, long max_in)
{
    if (!b) { fail("nnn_rate_create: null batch"); return nullptr; }
    if (!(source_rate > 0.0)) { fail("nnn_rate_create: the source rate must be positive"); return nullptr; }
    if (source_rate == 48000.0) { fail("nnn_rate_create: 48000 Hz needs no adapter: use the batch itself"); return nullptr; }
    if (source_rate < 1000.0 || source_rate > 2400000.0) { fail("nnn_rate_create: source rates from 1 kHz to 2.4 MHz"); return nullptr; }
    if (max_in < 1) { fail("nnn_rate_create: max_in must be at least 1"); return nullptr; }
    NNN_RT_LOCK;
    if (hipSetDevice(b->device) != hipSuccess) { fail("nnn_rate_create: no such HIP device"); return nullptr; }
    nnn_rate *a = new nnn_rate();
    a->b = b;
    a->S = b->S;
    a->device = b->device;
    a->max_in = max_in;
    a->leg[0].ratio = source_rate / 48000.0;
    a->leg[1].ratio = 48000.0 / source_rate;
    const double frames = ((double)max_in + 2.0) / a->leg[0].ratio / FRAME + 2.0;
    if (frames * FRAME > 1e9 || (frames * FRAME + 2.0) / a->leg[1].ratio > 1e9) {
        fail("nnn_rate_create: max_in = %ld is more than a call's 32-bit sample counts hold", max_in);
        delete a;
        return nullptr;
    }
    a->stage_stride = (long)nnn_rate_max_frames(a, max_in) * FRAME;
    a->leg[0].cap = rs_max_output(a->leg[0].ratio, max_in);
    a->leg[1].cap = rs_max_output(a->leg[1].ratio, a->stage_stride);
    const size_t S = (size_t)a->S;
    bool ok = true;
    auto dev = [&](auto **p, size_t bytes) {
        ok = ok && hipMalloc((void **)p, bytes ? bytes : 4) == hipSuccess && hipMemset(*p, 0, bytes) == hipSuccess;
    };
    for (auto &l : a->leg) {
        l.win = (int)ceil(RT_SPAN * l.ratio) + RS_TAPS + 2;   // 63 steps of at most ceil(ratio) samples, the first output's ring, slack
        for (l.nsb = 32; l.nsb > 4 && rate_lds_bytes(l.nsb, l.win) > 40 * 1024; l.nsb /= 2) {}   // (four blocks to the compute unit or more)
        l.lds = rate_lds_bytes(l.nsb, l.win);
        ok = ok && l.lds <= 64 * 1024;
        dev(&l.hist[0], S * RS_TAPS * sizeof(float));
        dev(&l.hist[1], S * RS_TAPS * sizeof(float));
        for (auto &m : l.memo) {
            dev(&m.sched, (size_t)l.cap * sizeof(RsOut));
            dev(&m.w, (size_t)l.cap * RS_TAPS * sizeof(double));
        }
    }
    dev(&a->stage, S * (size_t)a->stage_stride * sizeof(float));
    dev(&a->carry[0], S * FRAME * sizeof(float));
    dev(&a->carry[1], S * FRAME * sizeof(float));
    dev(&a->flags, S);
    const size_t per_out = sizeof(RsOut) + RS_TAPS * sizeof(double);
    a->pin_off[0] = 0;
    a->pin_off[1] = (size_t)a->leg[0].cap * per_out;
    a->pin_off[2] = a->pin_off[1] + (size_t)a->leg[1].cap * per_out;
    for (auto &p : a->pin)
        ok = ok && hipHostMalloc((void **)&p.p, a->pin_off[2] + S, hipHostMallocDefault) == hipSuccess &&
             hipEventCreateWithFlags(&p.ev, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&a->ev_last, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipDeviceSynchronize() == hipSuccess;   // (the memsets above are on the legacy stream; the calls run on non-blocking ones)
    a->reset_mark.assign(S, 0);
    if (!ok) {
        nnn_rate_destroy(a);
        fail("nnn_rate_create: allocation failed");
        return nullptr;
    }
    return a;
}

extern "C" int nnn_rate_reset_streams(nnn_rate *a, const int *streams, int n)
{
    if (!a) return fail("null adapter");
    if (n < 0 || (n > 0 && !streams)) return fail("nnn_rate_reset_streams: bad stream list");
    for (int i = 0; i < n; i++)
        if (streams[i] < 0 || streams[i] >= a->S) return fail("nnn_rate_reset_streams: stream %d outside [0, %d)", streams[i], a->S);
    for (int i = 0; i < n; i++)
        if (!a->reset_mark[(size_t)streams[i]]) a->reset_mark[(size_t)streams[i]] = 1, a->n_reset++;
    return 0;
}

extern "C" int nnn_rate_reset(nnn_rate *a)
{
    if (!a) return fail("null adapter");
    // every stream's histories and carried samples read as zero at the head of the next call (nothing to wait for, nothing to clear now)
    std::fill(a->reset_mark.begin(), a->reset_mark.end(), (unsigned char)1);
    a->n_reset = a->S;
    for (auto &l : a->leg) l.pos = RsPos();
    a->carried = 0;
    return 0;
}

extern "C" int nnn_rate_debug_tables(const nnn_rate *a, long tables[2], double host_us[2])
{
    if (!a) return fail("null adapter");
    for (int k = 0; k < 2; k++) {
        if (tables) tables[k] = a->leg[k].built;
        if (host_us) host_us[k] = a->leg[k].build_us;
    }
    return 0;
}

// The table of a leg's call of n_in samples at the leg's state: the resident one whose key matches, or a new one built into `pin` (page-locked)
// in place of the least recently used.  `up` says whether it has to be uploaded.
static int rate_plan(nnn_rate *a, RateLeg &l, long n_in, char *pin, RateLeg::Memo *&out, bool &up)
{
    uint64_t bits;
    memcpy(&bits, &l.pos.pos, sizeof(bits));
    RateLeg::Memo *lru = &l.memo[0];
    up = false;
    for (auto &m : l.memo) {
        if (m.valid && m.pos_bits == bits && m.idx == l.pos.idx && m.credit == l.pos.credit && m.n_in == n_in) {
            m.used = ++a->tick;
            out = &m;
            return 0;
        }
        if (!m.valid || (lru->valid && m.used < lru->used)) lru = &m;
    }
    const auto t0 = std::chrono::steady_clock::now();
    RsOut *sched = (RsOut *)pin;
    double *w = (double *)(pin + (size_t)l.cap * sizeof(RsOut));
    RateLeg::Memo &m = *lru;
    m.valid = false;
    m.after = l.pos;
    long n = 0, widest = 0;
    rs_schedule(l.ratio, m.after, n_in, l.cap, [&](const RsOut &o, const double *ow) {
        sched[n] = o;
        memcpy(w + (size_t)n * RS_TAPS, ow, RS_TAPS * sizeof(double));
        const long span0 = n - n % RT_SPAN;   // the window of the span this output belongs to, as the kernels lay it out
        const long wlen = (long)o.consumed - (sched[span0].consumed - RS_TAPS);
        if (wlen > widest) widest = wlen;
        n++;
    });
    if (widest > l.win) return fail("rate adapter: a span of %d outputs reaches over %ld source samples, more than the %d planned for", RT_SPAN, widest, l.win);
    m.pos_bits = bits;
    m.idx = l.pos.idx;
    m.credit = l.pos.credit;
    m.n_in = n_in;
    m.n_out = n;
    m.used = ++a->tick;
    m.valid = true;
    l.built++;
    l.build_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    out = &m;
    up = n > 0;
    return 0;
}

template <bool UP> static void rate_launch(const RateLeg &l, const RateLegArgs &args, int fmt, bool mask, hipStream_t st)
{
    void (*k)(RateLegArgs);
    if (UP) k = fmt == PCM_I16 ? (mask ? k_rate_in<PCM_I16, true> : k_rate_in<PCM_I16, false>) : (mask ? k_rate_in<PCM_F32, true> : k_rate_in<PCM_F32, false>);
    else k = fmt == PCM_I16 ? (mask ? k_rate_out<PCM_I16, true> : k_rate_out<PCM_I16, false>) : (mask ? k_rate_out<PCM_F32, true> : k_rate_out<PCM_F32, false>);
    const unsigned spans = args.n_out > 0 ? (unsigned)((args.n_out + RT_SPAN - 1) / RT_SPAN) : 1u;
    hipLaunchKernelGGL(k, dim3(spans, (unsigned)((args.n_streams + l.nsb - 1) / l.nsb)), dim3(RT_THREADS), l.lds, st, args);
}

extern "C" int nnn_rate_process_device(nnn_rate *a, const void *d_in, long n_in, size_t in_stride, void *d_out, long cap_out, size_t out_stride,
                                       long *n_out, float *d_vad, int cap_frames, int *n_frames, int format, void *hip_stream)
{
    if (!a || !n_out || !n_frames) return fail("null argument");
    *n_out = 0;
    *n_frames = 0;
    nnn_batch *b = a->b;
    if (format != PCM_F32 && format != PCM_I16) return fail("nnn_rate_process: format must be NNN_PCM_F32 or NNN_PCM_I16 (mono rows)");
    if (n_in < 0 || (n_in > 0 && !d_in) || !d_out) return fail("nnn_rate_process: bad buffer");
    if (n_in > a->max_in) return fail("nnn_rate_process: n_in = %ld is above the adapter's max_in = %ld", n_in, a->max_in);
    if (cap_out < nnn_rate_max_output(a, n_in)) return fail("nnn_rate_process: cap_out = %ld is below nnn_rate_max_output(a, n_in) = %ld", cap_out, nnn_rate_max_output(a, n_in));
    if (cap_frames < nnn_rate_max_frames(a, n_in)) return fail("nnn_rate_process: cap_frames = %d is below nnn_rate_max_frames(a, n_in) = %d", cap_frames, nnn_rate_max_frames(a, n_in));
    if (int rc = refuse_pending(b, "nnn_rate_process")) return rc;
    if (int rc = report_fault(b)) return rc;
    if (b->paths.inputs_ready) return fail("nnn_rate_process refused: the batch is under nnn_batch_set_inputs_ready(b, 1), and the frames it reads are produced by this call");
    HIPCHK(hipSetDevice(b->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : b->stream;
    if (a->have_last && a->last_stream != st) HIPCHK(hipStreamWaitEvent(st, a->ev_last, 0));
    // ---- the call's schedule: host arithmetic, or nothing at all where both keys are resident
    const bool mask = a->n_reset > 0 || b->n_held > 0;
    nnn_rate::Pin &pin = a->pin[a->pin_next];
    if (pin.busy) {
        HIPCHK(hipEventSynchronize(pin.ev));   // (RT_PIN calls back: long done)
        pin.busy = false;
    }
    RateLeg &lu = a->leg[0], &ld = a->leg[1];
    RateLeg::Memo *mu = nullptr, *md = nullptr;
    bool up_u = false, up_d = false;
    if (int rc = rate_plan(a, lu, n_in, pin.p + a->pin_off[0], mu, up_u)) return rc;
    const long total = a->carried + mu->n_out, T = total / FRAME;
    if (T * FRAME > a->stage_stride) return fail("rate adapter: %ld frames in a call sized for %ld", T, a->stage_stride / FRAME);
    if (int rc = rate_plan(a, ld, T * FRAME, pin.p + a->pin_off[1], md, up_d)) return rc;
    // ---- uploads out of the page-locked slot, then the three pieces in stream order
    for (int k = 0; k < 2; k++) {
        const RateLeg &l = a->leg[k];
        const RateLeg::Memo *m = k ? md : mu;
        if (!(k ? up_d : up_u)) continue;
        const char *src = pin.p + a->pin_off[k];
        HIPCHK(hipMemcpyAsync(m->sched, src, (size_t)m->n_out * sizeof(RsOut), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(m->w, src + (size_t)l.cap * sizeof(RsOut), (size_t)m->n_out * RS_TAPS * sizeof(double), hipMemcpyHostToDevice, st));
    }
    if (mask) {
        unsigned char *f = (unsigned char *)pin.p + a->pin_off[2];
        for (int s = 0; s < a->S; s++) f[s] = (unsigned char)((a->reset_mark[(size_t)s] ? RT_CLEAR : 0) | (b->n_held && b->held[(size_t)s] ? RT_CLEAR | RT_SKIP : 0));
        HIPCHK(hipMemcpyAsync(a->flags, f, (size_t)a->S, hipMemcpyHostToDevice, st));
    }
    if (up_u || up_d || mask) {
        HIPCHK(hipEventRecord(pin.ev, st));
        pin.busy = true;
        a->pin_next = (a->pin_next + 1) % RT_PIN;
    }
    const bool run_up = n_in > 0 || mu->n_out > 0 || mask, run_down = T > 0 || md->n_out > 0 || mask;
    if (run_up) {
        RateLegArgs g = {};
        g.in = d_in, g.in_stride = (long long)in_stride, g.n_in = n_in;
        g.hist_old = lu.hist[lu.par], g.hist_new = lu.hist[lu.par ^ 1];
        g.sched = mu->sched, g.w = mu->w, g.n_out = (int)mu->n_out;
        g.out = a->stage, g.out_stride = a->stage_stride;
        g.carry_old = a->carry[a->carry_par], g.carry_new = a->carry[a->carry_par ^ 1];
        g.carried = (int)a->carried, g.split = T * FRAME;
        g.flags = a->flags, g.n_streams = a->S, g.nsb = lu.nsb, g.win = lu.win;
        rate_launch<true>(lu, g, format, mask, st);
        lu.par ^= 1;
        a->carry_par ^= 1;
    }
    lu.pos = mu->after;
    a->carried = total - T * FRAME;
    if (run_up || run_down) HIPCHK(hipGetLastError());
    if (T > 0)
        if (int rc = nnn_batch_process_device(b, a->stage, a->stage, d_vad, (int)T, (size_t)a->stage_stride, FRAME, st)) return rc;
    if (run_down) {
        RateLegArgs g = {};
        g.in = a->stage, g.in_stride = a->stage_stride, g.n_in = T * FRAME;
        g.hist_old = ld.hist[ld.par], g.hist_new = ld.hist[ld.par ^ 1];
        g.sched = md->sched, g.w = md->w, g.n_out = (int)md->n_out;
        g.out = d_out, g.out_stride = (long long)out_stride;
        g.split = 0;
        g.flags = a->flags, g.n_streams = a->S, g.nsb = ld.nsb, g.win = ld.win;
        rate_launch<false>(ld, g, format, mask, st);
        ld.par ^= 1;
        HIPCHK(hipGetLastError());
    }
    ld.pos = md->after;
    if (mask && a->n_reset) {
        std::fill(a->reset_mark.begin(), a->reset_mark.end(), (unsigned char)0);
        a->n_reset = 0;
    }
    HIPCHK(hipEventRecord(a->ev_last, st));
    a->last_stream = st;
    a->have_last = true;
    *n_out = md->n_out;
    *n_frames = (int)T;
    return 0;
}

extern "C" int nnn_rate_process_host(nnn_rate *a, const void *in, long n_in, void *out, long cap_out, long *n_out, float *vad, int cap_frames,
                                     int *n_frames, int format)
{
    if (!a || !n_out || !n_frames) return fail("null argument");
    *n_out = 0;
    *n_frames = 0;
    if (format != PCM_F32 && format != PCM_I16) return fail("nnn_rate_process: format must be NNN_PCM_F32 or NNN_PCM_I16 (mono rows)");
    if (n_in < 0 || cap_out < 0 || cap_frames < 0 || (n_in > 0 && !in) || !out) return fail("nnn_rate_process: bad buffer");
    nnn_batch *b = a->b;
    HIPCHK(hipSetDevice(b->device));
    const size_t S = (size_t)a->S, e = (size_t)pcm_elem_bytes(format);
    const size_t in_bytes = S * (size_t)n_in * e, out_bytes = S * (size_t)cap_out * e, vad_bytes = vad ? (size_t)cap_frames * S * sizeof(float) : 0;
    auto room = [&](auto *&p, size_t &cap, size_t bytes) -> int {
        if (bytes <= cap) return 0;
        NNN_RT_LOCK;
        if (int rc = quiesce(b)) return rc;
        if (a->have_last) HIPCHK(hipEventSynchronize(a->ev_last));
        HIPCHK(hipFree(p));
        p = nullptr, cap = 0;
        HIPCHK(hipMalloc((void **)&p, bytes + bytes / 2));
        cap = bytes + bytes / 2;
        return 0;
    };
    if (int rc = room(a->h_in, a->h_in_cap, in_bytes)) return rc;
    if (int rc = room(a->h_out, a->h_out_cap, out_bytes)) return rc;
    if (int rc = room(a->h_vad, a->h_vad_cap, vad_bytes)) return rc;
    hipStream_t st = b->stream;
    if (in_bytes) HIPCHK(hipMemcpyAsync(a->h_in, in, in_bytes, hipMemcpyHostToDevice, st));
    if (b->n_held) {   // held streams' rows are not written on the device: they come back as the caller has them
        if (out_bytes) HIPCHK(hipMemcpyAsync(a->h_out, out, out_bytes, hipMemcpyHostToDevice, st));
        if (vad_bytes) HIPCHK(hipMemcpyAsync(a->h_vad, vad, vad_bytes, hipMemcpyHostToDevice, st));
    }
    if (int rc = nnn_rate_process_device(a, a->h_in, n_in, (size_t)n_in, a->h_out, cap_out, (size_t)cap_out, n_out, vad ? a->h_vad : nullptr, cap_frames,
                                         n_frames, format, st))
        return rc;
    if (*n_out > 0)
        HIPCHK(hipMemcpy2DAsync(out, (size_t)cap_out * e, a->h_out, (size_t)cap_out * e, (size_t)*n_out * e, S, hipMemcpyDeviceToHost, st));
    if (vad && *n_frames > 0) HIPCHK(hipMemcpyAsync(vad, a->h_vad, (size_t)*n_frames * S * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}
