// nnn_sim.hip -- the noise simulator (include/nnn_sim.h): n_streams NoiseSimulator instances over two int16 arenas
// resident on the device.  One call = per frame group k_sim (offsets -> signal, noise, mix, cutoff, VAD label in the staging) and then
// the ordinary training-row call over the staging, all on the caller's stream.
// Needs fail / HIPCHK / NNN_RT_LOCK (nnn_batch_core.hip), struct nnn_train and nnn_train_process_device (nnn_train.hip) and pk_s16
// (nnn_pack.hip).
// ref: src/training.rs:263-422 (NoiseSimulator), src/util.rs:114-126 (Biquad::filter_in_place).
#pragma once

#include "../../include/nnn_sim.h"

// ---- the kernel -----------------------------------------------------------------------------------------------------------------------
// lane = triple; a block is two waves and serves a tile of 64 triples through all frames of the launch.  The two biquads are serial per
// triple and every f64 instruction of a chain has to issue from its one wave (13 a sample: 8 ns each issued back to back,
// profiles/r4_f64_latency.txt), so the signal's filter runs on wave 0 and the noise's on wave 1, on another SIMD: the launch is bound by
// one chain's issue, not by two (measured with both chains interleaved on one wave: 89 us a frame).  Memories and the
// VAD counter stay in registers from frame to frame.
// A triple's frame is 960 contiguous bytes wherever its offset puts them, so the samples cross LDS both ways in chunks of SIM_CH: eight
// lanes of a wave take one triple's chunk of the wave's arena (64 contiguous bytes, four samples a lane by 8-byte words whatever the
// address class, sim_fetch) and lay it out [triple][sample] with a row stride of SIM_CH + 1 floats; lane s then walks row s.  The
// results go back into the same rows and leave as 128 contiguous bytes per triple and array, as k_hp stores its history rows; the mix is
// added on the way out, half of it by each wave, behind the one block barrier that says both filters' rows are there.  With the odd
// stride both the cooperative accesses (bank = row + 4 * quarter + k over four rows and eight quarters per 32-lane half) and the row walk
// (bank = lane + j) are free of bank conflicts.  The next chunk's samples are requested before the current chunk's recurrence and land
// behind it; a frame's offsets are put into LDS one frame ahead.
constexpr int SIM_CH = 32, SIM_LD = SIM_CH + 1, SIM_NCH = FRAME / SIM_CH;
static_assert(FRAME % SIM_CH == 0 && SIM_CH == 32, "");

struct SimArgs {
    const short *arena[2];            // signal, noise
    unsigned long long elems[2];
    const unsigned long long *off[2]; // [g][S]: element where the frame begins
    const nnn_sim_params *par;        // [S]
    float *state;                     // [S][4]: signal_resp_mem, noise_resp_mem
    int *vadc;                        // [S]: vad_count
    int *fault;                       // set when a frame's offset leaves its arena
    float *out[3];                    // signal, noise, combined: sample i of frame f of triple s at s * stream_stride + f * frame_stride + i
    long long stream_stride, frame_stride;
    int *cutoff;                      // [g][S]
    float *vad;                       // [g][S]
    int S, g;
};

// A chunk of one arena as a wave gathers it: per pass, this lane's four samples of row 8 * pass + lane / 8, still as the bytes that hold
// them.  They are taken apart only when the chunk is laid out in LDS, one chunk later: nothing between the request and that point waits
// for a load, so the loads travel behind the recurrence.
struct SimRaw {
    uint2 lo[8], hi[8];   // the two aligned 8-byte words that hold the four samples
    unsigned sh[8];       // byte offset of the first sample in `lo`: 0, 2, 4 or 6
};

// frame f's offset of this lane's triple into the table the gathering lanes read; -1: the frame leaves its arena and reads as zeros
__device__ __forceinline__ void sim_offsets(const unsigned long long *off, unsigned long long elems, int *fault, int f, int S, int sc, int lane, long long *tab)
{
    const unsigned long long o = off[(size_t)f * S + sc];
    const bool ok = o <= elems && elems - o >= (unsigned long long)FRAME;
    if (!ok) *fault = 1;
    tab[lane] = ok ? (long long)o : -1ll;
}

// Four samples are 8 bytes at a 2-byte aligned address: inside the 16 bytes from the 8-byte boundary below them, which two 8-byte loads
// fetch whatever the address class (one of them is the whole run when the run is aligned).  Only where those 16 bytes would leave the
// arena -- its first and last few samples, or an arena that does not begin on an 8-byte boundary -- the samples come one by one, and a
// frame outside its arena (offset -1) is zeros: a rare branch that whole waves skip.
__device__ __forceinline__ void sim_fetch(const short *arena, unsigned long long elems, const long long *tab, int c, int lane, SimRaw &r)
{
    const uintptr_t B = (uintptr_t)arena, E = B + 2 * (uintptr_t)elems;
#pragma unroll
    for (int it = 0; it < 8; it++) {
        const long long o = tab[8 * it + (lane >> 3)];
        const short *p = arena + (o < 0 ? 0 : o) + c * SIM_CH + 4 * (lane & 7);
        const uintptr_t A = (uintptr_t)p, lo = A & ~(uintptr_t)7;
        if (o < 0 || lo < B || lo + 16 > E) {
            uint2 w = make_uint2(0u, 0u);
            if (o >= 0) {
                w.x = (unsigned)(unsigned short)ld_global<short>(p) | (unsigned)(unsigned short)ld_global<short>(p + 1) << 16;
                w.y = (unsigned)(unsigned short)ld_global<short>(p + 2) | (unsigned)(unsigned short)ld_global<short>(p + 3) << 16;
            }
            r.lo[it] = w, r.hi[it] = w, r.sh[it] = 0u;
        } else {
            const unsigned long long v0 = ld_global<unsigned long long>((const void *)lo);   // (global, not flat: a flat load would also count as
            const unsigned long long v1 = ld_global<unsigned long long>((const void *)(lo + 8));   // an LDS access, and the next pass's table read would wait for it)
            r.lo[it] = make_uint2((unsigned)v0, (unsigned)(v0 >> 32));
            r.hi[it] = make_uint2((unsigned)v1, (unsigned)(v1 >> 32));
            r.sh[it] = (unsigned)(A & 7);
        }
    }
}

// the four samples of a gathered run as floats
__device__ __forceinline__ float4 sim_unpack(uint2 lo, uint2 hi, unsigned sh)
{
    const bool s4 = (sh & 4u) != 0u, s2 = (sh & 2u) != 0u;
    const unsigned d0 = s4 ? lo.y : lo.x, d1 = s4 ? hi.x : lo.y, d2 = s4 ? hi.y : hi.x;
    const unsigned r0 = s2 ? (d0 >> 16) | (d1 << 16) : d0, r1 = s2 ? (d1 >> 16) | (d2 << 16) : d1;
    return make_float4(pk_s16(r0), pk_s16(r0 >> 16), pk_s16(r1), pk_s16(r1 >> 16));
}

// a chunk's results out of LDS: this wave's own array, and its half of the mix (combined[i] = x[i] + n[i], src/training.rs:402-404)
__device__ __forceinline__ void sim_store(const SimArgs &a, const float *Lo, int w, int tile, int lane, int f, int c)
{
#pragma unroll
    for (int it = 0; it < 8; it++) {
        const int r = 8 * it + (lane >> 3), sr = tile * TILE + r;
        if (sr < a.S) {
            const long long at = (long long)sr * a.stream_stride + (long long)f * a.frame_stride + c * SIM_CH + 4 * (lane & 7);
            const float *ys = Lo + r * SIM_LD + 4 * (lane & 7), *yn = ys + TILE * SIM_LD, *y = w ? yn : ys;
            *(float4 *)(a.out[w] + at) = make_float4(y[0], y[1], y[2], y[3]);
            if ((it >> 2) == w)   // rows 0 .. 31 by wave 0, 32 .. 63 by wave 1
                *(float4 *)(a.out[2] + at) = make_float4(__fadd_rn(ys[0], yn[0]), __fadd_rn(ys[1], yn[1]), __fadd_rn(ys[2], yn[2]), __fadd_rn(ys[3], yn[3]));
        }
    }
}

// The loop runs over the launch's chunks k = 15 f + c.  Per chunk: the samples requested one chunk ago are laid out in the wave's input
// rows (the one place that waits for memory: for loads and stores that are a whole recurrence old); the PREVIOUS chunk's results, which
// both waves left in the output rows before the block barrier, go out to memory; the next chunk's samples are requested; then the
// recurrence, into the other pair of output rows -- loads and stores travel behind it -- and the barrier.
__global__ void __launch_bounds__(128) k_sim(SimArgs a)
{
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), tile = blockIdx.x;   // w: 0 the signal's wave, 1 the noise's
    const int s = tile * TILE + lane;
    const int sc = s < a.S ? s : a.S - 1;   // padding lanes of the last tile compute on the last real triple's data and store nothing
    __shared__ float Lin[2][TILE * SIM_LD];       // [wave]: its arena's samples of the chunk
    __shared__ float Lout[2][2][TILE * SIM_LD];   // [chunk parity][wave]: its filter's results
    __shared__ long long Loffs[2][2][TILE];       // [wave][frame parity][triple]
    float *Li = Lin[w];
    const short *arena = a.arena[w];
    const unsigned long long elems = a.elems[w], *off = a.off[w];
    const nnn_sim_params p = a.par[sc];
    const float gain = w ? p.noise_gain : p.signal_gain;
    const double a0 = (double)(w ? p.noise_a[0] : p.sig_a[0]), a1 = (double)(w ? p.noise_a[1] : p.sig_a[1]);
    const double b0 = (double)(w ? p.noise_b[0] : p.sig_b[0]), b1 = (double)(w ? p.noise_b[1] : p.sig_b[1]);
    float m0 = a.state[(size_t)sc * 4 + 2 * w], m1 = a.state[(size_t)sc * 4 + 2 * w + 1];
    int vc = a.vadc[sc];
    float energy = 0.0f;
    SimRaw raw;
    sim_offsets(off, elems, a.fault, 0, a.S, sc, lane, Loffs[w][0]);
    wave_lds_sync();
    sim_fetch(arena, elems, Loffs[w][0], 0, lane, raw);
    const int nk = a.g * SIM_NCH;
    int f = 0, c = 0;
#pragma nounroll
    for (int k = 0; k < nk; k++) {
        if (c == 0 && f + 1 < a.g) sim_offsets(off, elems, a.fault, f + 1, a.S, sc, lane, Loffs[w][(f + 1) & 1]);   // (read from this frame's last chunk on)
#pragma unroll
        for (int it = 0; it < 8; it++) {
            float *q = Li + (8 * it + (lane >> 3)) * SIM_LD + 4 * (lane & 7);
            const float4 v = sim_unpack(raw.lo[it], raw.hi[it], raw.sh[it]);
            q[0] = v.x, q[1] = v.y, q[2] = v.z, q[3] = v.w;
        }
        wave_lds_sync();
        float xs[SIM_CH];
#pragma unroll
        for (int j = 0; j < SIM_CH; j++) xs[j] = Li[lane * SIM_LD + j];
        wave_lds_sync();   // (the rows have been read: the next chunk's samples may take them)
        if (k > 0) sim_store(a, Lout[(k - 1) & 1][0], w, tile, lane, c ? f : f - 1, c ? c - 1 : SIM_NCH - 1);
        if (c + 1 < SIM_NCH) sim_fetch(arena, elems, Loffs[w][f & 1], c + 1, lane, raw);
        else if (f + 1 < a.g) sim_fetch(arena, elems, Loffs[w][(f + 1) & 1], 0, lane, raw);
        // read_signal / read_noise and filter_in_place (src/training.rs:322-339, src/util.rs:114-126), every statement one IEEE operation
        // (the build has -ffp-contract=off).  b * x is exact in f64 (24 x 24 bits), so b x - fl(a y) is ONE rounding: what
        // fma(x, b, -fl(a y)) returns, as in hp_recurrence.  Thirteen f64 instructions a sample.
        if (w == 0) {
#pragma unroll
            for (int j = 0; j < SIM_CH; j++) energy = __fadd_rn(energy, __fmul_rn(xs[j], xs[j]));
        }
        float *Lo = Lout[k & 1][w] + lane * SIM_LD;
#pragma unroll
        for (int j = 0; j < SIM_CH; j++) {
            const double x64 = (double)__fmul_rn(xs[j], gain);
            const double y64 = x64 + (double)m0;
            m0 = (float)((double)m1 + fma(x64, b0, -(a0 * y64)));
            m1 = (float)fma(x64, b1, -(a1 * y64));
            Lo[j] = (float)y64;
        }
        __syncthreads();   // both filters' rows of chunk k are there (and every wave is done reading chunk k - 1's: their turn again at k + 1)
        if (++c == SIM_NCH) {
            if (w == 0) {   // vad() and the cutoff (src/training.rs:368-386, :409-413)
                if (energy > 1e9f) vc = 0;
                else if (energy > 1e8f) vc -= 5;
                else if (energy > 1e7f) vc += 1;
                else vc += 2;
                vc = vc < 0 ? 0 : vc > 15 ? 15 : vc;
                const float vad = vc >= 10 ? 0.0f : vc > 0 ? 0.5f : 1.0f;
                if (s < a.S) {
                    a.vad[(size_t)f * a.S + s] = vad;
                    a.cutoff[(size_t)f * a.S + s] = (vad == 0.0f && p.noise_gain == 0.0f) ? 0 : p.band_lp + 1;
                }
                energy = 0.0f;
            }
            c = 0, f++;
        }
    }
    if (nk > 0) sim_store(a, Lout[(nk - 1) & 1][0], w, tile, lane, a.g - 1, SIM_NCH - 1);
    if (s < a.S) {
        a.state[(size_t)s * 4 + 2 * w] = m0;
        a.state[(size_t)s * 4 + 2 * w + 1] = m1;
        if (w == 0) a.vadc[s] = vc;
    }
}

// ---- the host side --------------------------------------------------------------------------------------------------------------------
struct nnn_sim {
    nnn_train *t = nullptr;
    int S = 0, NT = 0, gmax = 0, device = 0;   // (its own copies: destroy must not look into a training object that may be gone)
    hipStream_t own_stream = nullptr;          // the training object's stream: where the calls without a stream of the caller's run
    const short *arena[2] = {nullptr, nullptr};
    short *owned[2] = {nullptr, nullptr};      // the arenas nnn_sim_load made
    uint64_t elems[2] = {0, 0};
    std::vector<nnn_sim_params> par;           // the parameters as the host set them; d_par is their copy
    nnn_sim_params *d_par = nullptr;
    float *d_state = nullptr;                  // [S][4]
    int *d_vadc = nullptr, *d_fault = nullptr;
    float *stage = nullptr, *stage_vad = nullptr;   // [3][S][gmax * 480]; [gmax][S]
    int32_t *stage_cut = nullptr;
    // device buffers of the host entry points (made on first use, grow only)
    uint64_t *h_off = nullptr;
    float *h_rows = nullptr, *h_audio = nullptr, *h_vad = nullptr;
    int32_t *h_cut = nullptr;
    size_t h_off_cap = 0, h_rows_cap = 0, h_audio_cap = 0, h_vad_cap = 0, h_cut_cap = 0;   // bytes
    hipEvent_t ev_last = nullptr;              // end of the most recent call, on the stream it was made on
    hipStream_t last_stream = nullptr;
    bool have_last = false;
};

static nnn_sim_params sim_default_params()
{
    nnn_sim_params p = {};
    p.signal_gain = p.noise_gain = 1.0f;
    p.band_lp = NB - 1;
    return p;
}

extern "C" void nnn_sim_destroy(nnn_sim *sim)
{
    if (!sim) return;
    NNN_RT_LOCK;
    hipSetDevice(sim->device);
    if (sim->have_last) hipEventSynchronize(sim->ev_last);
    hipFree(sim->owned[0]); hipFree(sim->owned[1]);
    hipFree(sim->d_par); hipFree(sim->d_state); hipFree(sim->d_vadc); hipFree(sim->d_fault);
    hipFree(sim->stage); hipFree(sim->stage_vad); hipFree(sim->stage_cut);
    hipFree(sim->h_off); hipFree(sim->h_rows); hipFree(sim->h_audio); hipFree(sim->h_vad); hipFree(sim->h_cut);
    if (sim->ev_last) hipEventDestroy(sim->ev_last);
    delete sim;
}

extern "C" nnn_sim *nnn_sim_create(nnn_train *t)
{
    if (!t) { fail("nnn_sim_create: null training object"); return nullptr; }
    nnn_batch *h = t->comb;
    NNN_RT_LOCK;
    if (hipSetDevice(h->device) != hipSuccess) { fail("nnn_sim_create: no such HIP device"); return nullptr; }
    nnn_sim *sim = new nnn_sim();
    sim->t = t;
    sim->S = h->S, sim->NT = h->NT, sim->gmax = h->gmax, sim->device = h->device, sim->own_stream = h->stream;
    sim->par.assign((size_t)sim->S, sim_default_params());
    const size_t S = (size_t)sim->S, G = (size_t)sim->gmax;
    bool ok = true;
    auto dev = [&](auto **q, size_t bytes) { ok = ok && hipMalloc((void **)q, bytes) == hipSuccess && hipMemset(*q, 0, bytes) == hipSuccess; };
    dev(&sim->d_par, S * sizeof(nnn_sim_params));
    dev(&sim->d_state, S * 4 * sizeof(float));
    dev(&sim->d_vadc, S * sizeof(int));
    dev(&sim->d_fault, sizeof(int));
    dev(&sim->stage, 3 * S * G * FRAME * sizeof(float));
    dev(&sim->stage_vad, G * S * sizeof(float));
    dev(&sim->stage_cut, G * S * sizeof(int32_t));
    ok = ok && hipMemcpy(sim->d_par, sim->par.data(), S * sizeof(nnn_sim_params), hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&sim->ev_last, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipDeviceSynchronize() == hipSuccess;   // (the memsets above are on the legacy stream; the calls are on non-blocking ones)
    if (!ok) {
        nnn_sim_destroy(sim);
        fail("nnn_sim_create: allocation failed (the staging is 3 x 1920 bytes x %d group frames for each of %d triples)", (int)G, (int)S);
        return nullptr;
    }
    return sim;
}

// everything enqueued so far is done (before memory a call may still read is released or rewritten from the host)
static int sim_drain(nnn_sim *sim)
{
    HIPCHK(hipSetDevice(sim->device));
    if (sim->have_last) HIPCHK(hipEventSynchronize(sim->ev_last));
    return 0;
}

static int sim_which(int which)
{
    return which == NNN_SIM_ARENA_SIGNAL || which == NNN_SIM_ARENA_NOISE ? 0 : fail("nnn_sim: which = %d is neither NNN_SIM_ARENA_SIGNAL (0) nor NNN_SIM_ARENA_NOISE (1)", which);
}

extern "C" int nnn_sim_adopt_device(nnn_sim *sim, int which, const int16_t *d_pcm, uint64_t elems)
{
    if (!sim) return fail("null simulator");
    if (int rc = sim_which(which)) return rc;
    if (!d_pcm || elems == 0) return fail("nnn_sim_adopt_device: null or empty arena");
    if ((uintptr_t)d_pcm & 1) return fail("nnn_sim_adopt_device: the arena is not aligned to its 2-byte elements");
    if (elems >= (1ull << 62)) return fail("nnn_sim_adopt_device: %llu elements are more than an arena counts", (unsigned long long)elems);
    NNN_RT_LOCK;
    if (int rc = sim_drain(sim)) return rc;
    if (sim->owned[which]) HIPCHK(hipFree(sim->owned[which]));
    sim->owned[which] = nullptr;
    sim->arena[which] = d_pcm;
    sim->elems[which] = elems;
    return 0;
}

extern "C" int nnn_sim_load(nnn_sim *sim, int which, const int16_t *pcm, uint64_t elems)
{
    if (!sim) return fail("null simulator");
    if (int rc = sim_which(which)) return rc;
    if (!pcm || elems == 0) return fail("nnn_sim_load: null or empty arena");
    if (elems >= (1ull << 62)) return fail("nnn_sim_load: %llu elements are more than an arena counts", (unsigned long long)elems);
    NNN_RT_LOCK;
    if (int rc = sim_drain(sim)) return rc;
    short *d = nullptr;
    HIPCHK(hipMalloc((void **)&d, (size_t)elems * sizeof(short)));
    if (hipMemcpy(d, pcm, (size_t)elems * sizeof(short), hipMemcpyHostToDevice) != hipSuccess) {
        hipFree(d);
        return fail("nnn_sim_load: the upload failed");
    }
    if (sim->owned[which]) HIPCHK(hipFree(sim->owned[which]));
    sim->owned[which] = d;
    sim->arena[which] = d;
    sim->elems[which] = elems;
    return 0;
}

static int sim_streams(const nnn_sim *sim, const int *streams, int n, const char *who)
{
    if (n < 0) return fail("%s: n = %d", who, n);
    if (!streams && n > sim->S) return fail("%s: %d records for %d triples", who, n, sim->S);
    for (int i = 0; streams && i < n; i++)
        if (streams[i] < 0 || streams[i] >= sim->S) return fail("%s: stream %d outside [0, %d)", who, streams[i], sim->S);
    return 0;
}

extern "C" int nnn_sim_set_params(nnn_sim *sim, const int *streams, int n, const nnn_sim_params *recs)
{
    if (!sim) return fail("null simulator");
    if (int rc = sim_streams(sim, streams, n, "nnn_sim_set_params")) return rc;
    if (n == 0) return 0;
    if (!recs) return fail("nnn_sim_set_params: null records");
    for (int i = 0; i < n; i++) {
        const nnn_sim_params &r = recs[i];
        const float v[10] = {r.signal_gain, r.noise_gain, r.sig_a[0], r.sig_a[1], r.sig_b[0], r.sig_b[1], r.noise_a[0], r.noise_a[1], r.noise_b[0], r.noise_b[1]};
        for (float x : v)
            if (!std::isfinite(x)) return fail("nnn_sim_set_params: record %d holds a value that is not finite", i);
        if (r.band_lp < 0 || r.band_lp > NB - 1) return fail("nnn_sim_set_params: record %d: band_lp = %d outside [0, %d]", i, r.band_lp, NB - 1);
    }
    NNN_RT_LOCK;
    if (int rc = sim_drain(sim)) return rc;   // (the calls enqueued so far keep the parameters they were made under)
    for (int i = 0; i < n; i++) sim->par[(size_t)(streams ? streams[i] : i)] = recs[i];
    HIPCHK(hipMemcpy(sim->d_par, sim->par.data(), sim->par.size() * sizeof(nnn_sim_params), hipMemcpyHostToDevice));
    return 0;
}

extern "C" int nnn_sim_get_params(nnn_sim *sim, const int *streams, int n, nnn_sim_params *recs)
{
    if (!sim) return fail("null simulator");
    if (int rc = sim_streams(sim, streams, n, "nnn_sim_get_params")) return rc;
    if (n == 0) return 0;
    if (!recs) return fail("nnn_sim_get_params: null records");
    for (int i = 0; i < n; i++) recs[i] = sim->par[(size_t)(streams ? streams[i] : i)];
    return 0;
}

extern "C" int nnn_sim_reset(nnn_sim *sim)
{
    if (!sim) return fail("null simulator");
    NNN_RT_LOCK;
    if (int rc = sim_drain(sim)) return rc;
    HIPCHK(hipMemset(sim->d_state, 0, (size_t)sim->S * 4 * sizeof(float)));
    HIPCHK(hipMemset(sim->d_vadc, 0, (size_t)sim->S * sizeof(int)));
    HIPCHK(hipDeviceSynchronize());
    return 0;
}

extern "C" int nnn_sim_fault(nnn_sim *sim)
{
    if (!sim) return -fail("null simulator");
    NNN_RT_LOCK;
    if (sim_drain(sim)) return -1;
    int v = 0;
    if (hipMemcpy(&v, sim->d_fault, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return -fail("nnn_sim_fault: the flag could not be read");
    return v ? 1 : 0;
}

// what every call checks before anything is enqueued, and the stream it runs on
static int sim_begin(nnn_sim *sim, const void *sig_off, const void *noise_off, int n_frames, void *hip_stream, const char *who, hipStream_t *st)
{
    if (n_frames < 0) return fail("%s: n_frames = %d", who, n_frames);
    if (!sim->arena[0] || !sim->arena[1]) return fail("%s: the %s arena is not loaded (nnn_sim_load / nnn_sim_adopt_device)", who, sim->arena[0] ? "noise" : "signal");
    if (!sig_off || !noise_off) return fail("%s: null offsets", who);
    HIPCHK(hipSetDevice(sim->device));
    *st = hip_stream ? (hipStream_t)hip_stream : sim->own_stream;
    if (sim->have_last && sim->last_stream != *st) HIPCHK(hipStreamWaitEvent(*st, sim->ev_last, 0));   // (the state and the staging are the previous call's until then)
    return 0;
}

static int sim_end(nnn_sim *sim, hipStream_t st)
{
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(sim->ev_last, st));
    sim->last_stream = st;
    sim->have_last = true;
    return 0;
}

// k_sim over frames f0 .. f0 + g - 1 of a call's offsets
static void sim_launch(const nnn_sim *sim, hipStream_t st, const uint64_t *d_sig_off, const uint64_t *d_noise_off, int f0, int g, float *o_sig, float *o_noise,
                       float *o_comb, size_t stream_stride, size_t frame_stride, int32_t *cutoff, float *vad)
{
    SimArgs a = {};
    for (int k = 0; k < 2; k++) a.arena[k] = sim->arena[k], a.elems[k] = sim->elems[k];
    a.off[0] = (const unsigned long long *)d_sig_off + (size_t)f0 * sim->S;
    a.off[1] = (const unsigned long long *)d_noise_off + (size_t)f0 * sim->S;
    a.par = sim->d_par, a.state = sim->d_state, a.vadc = sim->d_vadc, a.fault = sim->d_fault;
    a.out[0] = o_sig, a.out[1] = o_noise, a.out[2] = o_comb;
    a.stream_stride = (long long)stream_stride, a.frame_stride = (long long)frame_stride;
    a.cutoff = cutoff, a.vad = vad;
    a.S = sim->S, a.g = g;
    hipLaunchKernelGGL(k_sim, dim3((unsigned)sim->NT), dim3(128), 0, st, a);
}

extern "C" int nnn_sim_process_device(nnn_sim *sim, const uint64_t *d_sig_off, const uint64_t *d_noise_off, float *d_rows, int n_frames, void *hip_stream)
{
    if (!sim) return fail("null simulator");
    hipStream_t st;
    if (int rc = sim_begin(sim, d_sig_off, d_noise_off, n_frames, hip_stream, "nnn_sim_process", &st)) return rc;
    if (n_frames == 0) return 0;
    if (!d_rows) return fail("nnn_sim_process: null rows");
    const size_t S = (size_t)sim->S, row = (size_t)sim->gmax * FRAME, na = S * row;
    for (int f0 = 0; f0 < n_frames; f0 += sim->gmax) {
        const int g = n_frames - f0 < sim->gmax ? n_frames - f0 : sim->gmax;
        sim_launch(sim, st, d_sig_off, d_noise_off, f0, g, sim->stage, sim->stage + na, sim->stage + 2 * na, row, FRAME, sim->stage_cut, sim->stage_vad);
        if (int rc = nnn_train_process_device(sim->t, sim->stage, sim->stage + na, sim->stage + 2 * na, sim->stage_cut, sim->stage_vad,
                                              d_rows + (size_t)f0 * S * TRAIN_COLS, g, row, FRAME, st))
            return rc;
    }
    return sim_end(sim, st);
}

extern "C" int nnn_sim_signals_device(nnn_sim *sim, const uint64_t *d_sig_off, const uint64_t *d_noise_off, float *d_signal, float *d_noise,
                                      float *d_combined, int32_t *d_cutoff, float *d_vad, int n_frames, size_t stream_stride, size_t frame_stride,
                                      void *hip_stream)
{
    if (!sim) return fail("null simulator");
    hipStream_t st;
    if (int rc = sim_begin(sim, d_sig_off, d_noise_off, n_frames, hip_stream, "nnn_sim_signals", &st)) return rc;
    if (n_frames == 0) return 0;
    if (!d_signal || !d_noise || !d_combined || !d_cutoff || !d_vad) return fail("nnn_sim_signals: null buffer");
    if ((((uintptr_t)d_signal | (uintptr_t)d_noise | (uintptr_t)d_combined) & 15) || (stream_stride & 3) || (frame_stride & 3))
        return fail("nnn_sim_signals: the audio buffers and their strides must be multiples of 16 bytes");
    sim_launch(sim, st, d_sig_off, d_noise_off, 0, n_frames, d_signal, d_noise, d_combined, stream_stride, frame_stride, d_cutoff, d_vad);
    return sim_end(sim, st);
}

extern "C" int nnn_sim_debug_kernel(nnn_sim *sim, const uint64_t *d_sig_off, const uint64_t *d_noise_off, int n_frames, int reps, void *hip_stream)
{
    if (!sim) return fail("null simulator");
    if (n_frames < 1 || n_frames > sim->gmax || reps < 0) return fail("nnn_sim_debug_kernel: n_frames outside [1, %d] or negative reps", sim->gmax);
    hipStream_t st;
    if (int rc = sim_begin(sim, d_sig_off, d_noise_off, n_frames, hip_stream, "nnn_sim_debug_kernel", &st)) return rc;
    const size_t row = (size_t)sim->gmax * FRAME, na = (size_t)sim->S * row;
    for (int r = 0; r < reps; r++)
        sim_launch(sim, st, d_sig_off, d_noise_off, 0, n_frames, sim->stage, sim->stage + na, sim->stage + 2 * na, row, FRAME, sim->stage_cut, sim->stage_vad);
    return sim_end(sim, st);
}

// the host entry points' check: every frame inside its arena, or the whole call is refused before anything is enqueued
static int sim_check_offsets(const nnn_sim *sim, const uint64_t *sig_off, const uint64_t *noise_off, int n_frames, const char *who)
{
    const uint64_t *off[2] = {sig_off, noise_off};
    const size_t n = (size_t)n_frames * sim->S;
    for (int k = 0; k < 2; k++)
        for (size_t i = 0; i < n; i++)
            if (off[k][i] > sim->elems[k] || sim->elems[k] - off[k][i] < (uint64_t)FRAME)
                return fail("%s: frame %zu of triple %zu: %s offset %llu + 480 leaves the arena of %llu elements", who, i / sim->S, i % sim->S,
                            k ? "noise" : "signal", (unsigned long long)off[k][i], (unsigned long long)sim->elems[k]);
    return 0;
}

template <class T> static int sim_room(nnn_sim *sim, T *&q, size_t &cap, size_t bytes)
{
    if (bytes <= cap) return 0;
    NNN_RT_LOCK;
    if (int rc = sim_drain(sim)) return rc;
    HIPCHK(hipFree(q));
    q = nullptr, cap = 0;
    HIPCHK(hipMalloc((void **)&q, bytes));
    cap = bytes;
    return 0;
}

extern "C" int nnn_sim_process_host(nnn_sim *sim, const uint64_t *sig_off, const uint64_t *noise_off, float *rows, int n_frames)
{
    if (!sim) return fail("null simulator");
    hipStream_t st;
    if (int rc = sim_begin(sim, sig_off, noise_off, n_frames, nullptr, "nnn_sim_process", &st)) return rc;
    if (n_frames == 0) return 0;
    if (!rows) return fail("nnn_sim_process: null rows");
    if (int rc = sim_check_offsets(sim, sig_off, noise_off, n_frames, "nnn_sim_process")) return rc;
    const size_t nl = (size_t)n_frames * sim->S;
    if (int rc = sim_room(sim, sim->h_off, sim->h_off_cap, 2 * nl * sizeof(uint64_t))) return rc;
    if (int rc = sim_room(sim, sim->h_rows, sim->h_rows_cap, nl * TRAIN_COLS * sizeof(float))) return rc;
    HIPCHK(hipMemcpyAsync(sim->h_off, sig_off, nl * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(sim->h_off + nl, noise_off, nl * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    if (int rc = nnn_sim_process_device(sim, sim->h_off, sim->h_off + nl, sim->h_rows, n_frames, st)) return rc;
    HIPCHK(hipMemcpyAsync(rows, sim->h_rows, nl * TRAIN_COLS * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

extern "C" int nnn_sim_signals_host(nnn_sim *sim, const uint64_t *sig_off, const uint64_t *noise_off, float *signal, float *noise, float *combined,
                                    int32_t *cutoff, float *vad, int n_frames)
{
    if (!sim) return fail("null simulator");
    hipStream_t st;
    if (int rc = sim_begin(sim, sig_off, noise_off, n_frames, nullptr, "nnn_sim_signals", &st)) return rc;
    if (n_frames == 0) return 0;
    if (!signal || !noise || !combined || !cutoff || !vad) return fail("nnn_sim_signals: null buffer");
    if (int rc = sim_check_offsets(sim, sig_off, noise_off, n_frames, "nnn_sim_signals")) return rc;
    const size_t nl = (size_t)n_frames * sim->S, na = nl * FRAME;
    if (int rc = sim_room(sim, sim->h_off, sim->h_off_cap, 2 * nl * sizeof(uint64_t))) return rc;
    if (int rc = sim_room(sim, sim->h_audio, sim->h_audio_cap, 3 * na * sizeof(float))) return rc;
    if (int rc = sim_room(sim, sim->h_vad, sim->h_vad_cap, nl * sizeof(float))) return rc;
    if (int rc = sim_room(sim, sim->h_cut, sim->h_cut_cap, nl * sizeof(int32_t))) return rc;
    HIPCHK(hipMemcpyAsync(sim->h_off, sig_off, nl * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(sim->h_off + nl, noise_off, nl * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    float *d = sim->h_audio;
    if (int rc = nnn_sim_signals_device(sim, sim->h_off, sim->h_off + nl, d, d + na, d + 2 * na, sim->h_cut, sim->h_vad, n_frames,
                                        (size_t)n_frames * FRAME, FRAME, st))
        return rc;
    float *dst[3] = {signal, noise, combined};
    for (int k = 0; k < 3; k++) HIPCHK(hipMemcpyAsync(dst[k], d + k * na, na * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(cutoff, sim->h_cut, nl * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(vad, sim->h_vad, nl * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}
