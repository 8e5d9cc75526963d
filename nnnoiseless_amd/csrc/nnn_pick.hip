// nnn_pick.hip -- the talker picker (include/nnn_pick.h): the k loudest open gates of every room, with hysteresis,
// pins and the dominant speaker, between the VAD gate and the mixer.
// One call = k_pick_level (the bandwidth part, a wave per stream and run of frames: the energy of every open stream-frame in the scorer's
// summation order, into scratch) and k_pick_rank (the sequential part: the call's frames in order, level and selected carried, a room
// seated by its size on a lane, a run of lanes, a wave or a block), on the caller's stream.  The member tables (rooms as CSR, the rooms of
// each size class) are made on the host by the setters.
// Needs fail / HIPCHK / NNN_RT_LOCK (nnn_batch_core.hip), pcm_load and the PCM_* formats (nnn_common.hip), ld_global (nnn_mfma.h).
#pragma once

#include <float.h>
#include <limits.h>

#include "../../include/nnn_pick.h"

// ---- the kernels ------------------------------------------------------------------------------------------------------------------------
constexpr int PICK_WAVES = 4;                         // waves (streams) per block of k_pick_level
constexpr int PICK_RUN = 4;                           // consecutive frames of its stream a wave of k_pick_level takes
constexpr int PICK_TERMS = (FRAME + 63) / 64;         // 8: lane L owns samples L + 64 k
constexpr int PICK_THREADS = 256;                     // a block of k_pick_rank
constexpr int PICK_SEG = NNN_PICK_SEG_ROOM, PICK_WAVE = NNN_PICK_WAVE_ROOM;
static_assert(FRAME == NNN_PICK_FRAME && PICK_WAVE == 64 && PICK_THREADS % 64 == 0 && 64 % PICK_SEG == 0 && (PICK_SEG & (PICK_SEG - 1)) == 0, "");

struct PickLevelArgs {
    const char *in;                   // element (s, t, i) at (s / C) * gs + t * fs + i * C + s % C, in elements of the format
    const unsigned char *open;        // NULL or [T][S]
    const unsigned char *live;        // NULL or [S]
    double *e;                        // [T][S]: written where the stream is live and the gate open, nowhere else
    long long gs, fs;
    int S, T, C;
};

// Frame t's loads: lane L takes samples L + 64 k, the assignment the summation order is stated in.  One channel: every instruction
// fetches 64 consecutive elements.
template <int FMT> __device__ __forceinline__ void pick_load(const PickLevelArgs &a, long long col, int t, int lane, float *v)
{
    const char *p = a.in + (col + (long long)t * a.fs) * (FMT == PCM_I16 ? 2 : 4);
#pragma unroll
    for (int k = 0; k < PICK_TERMS; k++) {
        const int i = lane + 64 * k;
        v[k] = 0.0f;
        if (i < FRAME) v[k] = pcm_load<FMT>(p + (long long)i * a.C * (FMT == PCM_I16 ? 2 : 4));
    }
}

// step 1 of the header's rule on a loaded frame; every lane returns e_n
__device__ __forceinline__ double pick_energy(const float *v, int lane)
{
#pragma clang fp contract(off)
    double p = 0.0;
#pragma unroll
    for (int k = 0; k < PICK_TERMS; k++)
        if (lane + 64 * k < FRAME) {
            const double xd = (double)v[k];
            p = p + xd * xd;
        }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) p = p + __shfl_xor(p, m);
    return p <= DBL_MAX ? p : 0.0;
}

// A wave per stream (blockIdx.x) and run of PICK_RUN consecutive frames (blockIdx.y, striding over the runs where the call has more of
// them than a grid has rows): k_score's shape.  The next frame's eight loads are issued before the current frame's tree and land behind
// it.  A stream that is not live and a frame whose gate is closed load nothing and store nothing.
template <int FMT> __global__ void __launch_bounds__(64 * PICK_WAVES) k_pick_level(PickLevelArgs a)
{
    const int lane = threadIdx.x & 63, s = blockIdx.x * PICK_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (s >= a.S) return;                                              // (whole waves; the kernel has no block barrier)
    if (a.live && ld_global<unsigned char>(a.live + s) == 0) return;
    const long long col = (long long)(s / a.C) * a.gs + s % a.C;
    const int runs = (a.T + PICK_RUN - 1) / PICK_RUN;
    for (int run = blockIdx.y; run < runs; run += gridDim.y) {
        const int t0 = run * PICK_RUN;
        float v[2][PICK_TERMS];
        bool on = !a.open || ld_global<unsigned char>(a.open + (size_t)t0 * a.S + s) != 0;
        if (on) pick_load<FMT>(a, col, t0, lane, v[0]);
#pragma unroll
        for (int j = 0; j < PICK_RUN; j++) {
            const int t = t0 + j;
            if (t < a.T) {
                const bool on_next = j + 1 < PICK_RUN && t + 1 < a.T && (!a.open || ld_global<unsigned char>(a.open + (size_t)(t + 1) * a.S + s) != 0);
                if (on_next) pick_load<FMT>(a, col, t + 1, lane, v[(j + 1) & 1]);
                if (on) {
                    const double e = pick_energy(v[j & 1], lane);
                    if (lane == 0) a.e[(size_t)t * a.S + s] = e;
                }
                on = on_next;
            }
        }
    }
}

struct PickRankArgs {
    const double *e;                  // [T][S], k_pick_level's
    const unsigned char *open;        // NULL or [T][S]
    const unsigned char *live;        // NULL or [S]
    unsigned char *talk;              // [T][S]; may be `open`
    int *dominant;                    // NULL or [T][S]
    double *level_out;                // NULL or [T][S]
    double *level;                    // [S]: the state
    unsigned char *sel;               // [S]: the state
    unsigned long long *key;          // [S]: scratch of the rooms seated on a block
    const unsigned char *pin;         // [S]
    const int *off, *mem;             // rooms as CSR: room r's members, ascending, are mem[off[r] .. off[r + 1])
    const int *cls;                   // the rooms by class: n_blk rooms beyond WAVE_ROOM, n_wav up to it, n_seg up to SEG_ROOM, then the n_one lone STREAMS
    int n_blk, n_wav, n_seg, n_one;
    int b_wav, b_seg, b_one;          // the first block of each class after the first
    int S, T, K;
    double decay, stick;
};

// The ranking key of step 3 plus one: 0 says "no candidate", and for candidates bit 63 (free: a score is a non-negative double, at most
// +inf) carries the pin, so that one u64 comparison is "pinned descending, then score descending".
__device__ __forceinline__ unsigned long long pick_key(double level, int sel, int pin, double stick)
{
#pragma clang fp contract(off)
    const double score = sel ? level * stick : level;
    unsigned long long bits;
    memcpy(&bits, &score, sizeof(bits));
    return (bits | (unsigned long long)pin << 63) + 1ull;
}

// (ka, sa) ranks ahead of (kb, sb): key descending, stream index ascending
__device__ __forceinline__ bool pick_ahead(unsigned long long ka, int sa, unsigned long long kb, int sb) { return ka > kb || (ka == kb && sa < sb); }

// the first-ranked of W neighbouring lanes' (key, stream) pairs, in every one of them
template <int W> __device__ __forceinline__ void pick_first(unsigned long long &k, int &s)
{
#pragma unroll
    for (int m = W / 2; m >= 1; m >>= 1) {
        const unsigned long long ok = __shfl_xor(k, m);
        const int os = __shfl_xor(s, m);
        if (pick_ahead(ok, os, k, s)) k = ok, s = os;
    }
}

// Steps 2 to 5 for rooms of at most W members, a member a lane, W neighbouring lanes a room: level and selected stay in registers over
// the call's frames, the next frame's energy and gate byte are fetched before the current frame is ranked.  Selection is K rounds of
// "the first-ranked candidate behind the previous round's winner": nothing is marked, so the rounds need no state but the last winner,
// and afterwards talk = "a candidate ranked at or ahead of the last winner".  Every lane of the wave makes the same K rounds (a room with
// fewer candidates finds nobody in the later ones), so the shuffles never sit in divergent control flow.
template <int W> __device__ __forceinline__ void pick_rank_lanes(const PickRankArgs &a, int room, int j)
{
#pragma clang fp contract(off)
    int s = -1;
    if (W == 1) s = room;                                               // (the class of lone streams lists the streams themselves)
    else if (room >= 0) {
        const int m0 = a.off[room];
        if (j < a.off[room + 1] - m0) s = a.mem[m0 + j];
    }
    const bool live = s >= 0 && (!a.live || a.live[s] != 0);
    double level = 0.0;
    int sel = 0, pin = 0;
    if (live) level = a.level[s], sel = a.sel[s], pin = a.pin[s];
    double e_next = 0.0;
    bool o_next = false;
    auto fetch = [&](int t) {
        if (!live) return;
        const size_t at = (size_t)t * a.S + s;
        o_next = !a.open || a.open[at] != 0;
        e_next = a.e[at];                                               // (whatever lies there where the gate is closed: not used then)
    };
    fetch(0);
    for (int t = 0; t < a.T; t++) {
        const bool cand = live && o_next;
        const double e = cand ? e_next : 0.0;
        if (t + 1 < a.T) fetch(t + 1);
        const double d = level * a.decay;
        level = e > d ? e : d;
        const unsigned long long k1 = cand ? pick_key(level, sel, pin, a.stick) : 0ull;
        int talk, first;
        if (W == 1) talk = cand, first = cand ? s : -1;
        else {
            unsigned long long wk = ~0ull;                              // the last winner; nobody yet: every candidate is behind it
            int ws = -1;
            first = -1;
            for (int r = 0; r < a.K; r++) {
                const bool behind = k1 != 0 && pick_ahead(wk, ws, k1, s);
                unsigned long long bk = behind ? k1 : 0ull;
                int bs = behind ? s : INT_MAX;
                pick_first<W>(bk, bs);
                if (bk != 0) {
                    wk = bk, ws = bs;
                    if (r == 0) first = bs;
                }
            }
            talk = k1 != 0 && ws >= 0 && !pick_ahead(wk, ws, k1, s);
        }
        if (live) {
            const size_t at = (size_t)t * a.S + s;
            a.talk[at] = (unsigned char)talk;
            if (a.dominant) a.dominant[at] = first;
            if (a.level_out) a.level_out[at] = level;
            sel = talk;
        }
    }
    if (live) a.level[s] = level, a.sel[s] = (unsigned char)sel;
}

// The same for a room beyond a wave, a block to itself, its members strided over the threads: a thread's members are its own in every
// pass, so level, selected and the frame's keys go through global memory without any ordering between threads; only the winner of a
// round crosses them, wave by wave through LDS.  The rounds end when one finds nobody -- the same for the whole block.
__device__ __forceinline__ void pick_rank_block(const PickRankArgs &a, int room)
{
#pragma clang fp contract(off)
    __shared__ unsigned long long Lk[2][PICK_THREADS / 64];
    __shared__ int Ls[2][PICK_THREADS / 64];
    const int tid = (int)threadIdx.x, m0 = a.off[room], n = a.off[room + 1] - m0;
    for (int t = 0; t < a.T; t++) {
        unsigned long long bk = 0ull, wk = ~0ull;
        int bs = INT_MAX, ws = -1, first = -1;
        for (int j = tid; j < n; j += PICK_THREADS) {                   // step 2 and the keys
            const int s = a.mem[m0 + j];
            if (a.live && a.live[s] == 0) continue;
            const size_t at = (size_t)t * a.S + s;
            const bool cand = !a.open || a.open[at] != 0;
            const double e = cand ? a.e[at] : 0.0, d = a.level[s] * a.decay;
            const double level = e > d ? e : d;
            a.level[s] = level;
            if (a.level_out) a.level_out[at] = level;
            const unsigned long long k1 = cand ? pick_key(level, a.sel[s], a.pin[s], a.stick) : 0ull;
            a.key[s] = k1;
            if (k1 != 0 && pick_ahead(k1, s, bk, bs)) bk = k1, bs = s;
        }
        for (int r = 0; r < a.K; r++) {
            pick_first<64>(bk, bs);
            if ((tid & 63) == 0) Lk[r & 1][tid >> 6] = bk, Ls[r & 1][tid >> 6] = bs;
            __syncthreads();
            bk = 0ull, bs = INT_MAX;
#pragma unroll
            for (int w = 0; w < PICK_THREADS / 64; w++)
                if (pick_ahead(Lk[r & 1][w], Ls[r & 1][w], bk, bs)) bk = Lk[r & 1][w], bs = Ls[r & 1][w];
            if (bk == 0) break;
            wk = bk, ws = bs;
            if (r == 0) first = bs;
            bk = 0ull, bs = INT_MAX;
            if (r + 1 < a.K)
                for (int j = tid; j < n; j += PICK_THREADS) {           // the thread's first-ranked candidate behind the winner
                    const int s = a.mem[m0 + j];
                    if (a.live && a.live[s] == 0) continue;
                    const unsigned long long k1 = a.key[s];
                    if (k1 != 0 && pick_ahead(wk, ws, k1, s) && pick_ahead(k1, s, bk, bs)) bk = k1, bs = s;
                }
        }
        for (int j = tid; j < n; j += PICK_THREADS) {                   // steps 4 and 5
            const int s = a.mem[m0 + j];
            if (a.live && a.live[s] == 0) continue;
            const size_t at = (size_t)t * a.S + s;
            const unsigned long long k1 = a.key[s];
            const int talk = k1 != 0 && ws >= 0 && !pick_ahead(wk, ws, k1, s);
            a.talk[at] = (unsigned char)talk;
            if (a.dominant) a.dominant[at] = first;
            a.sel[s] = (unsigned char)talk;
        }
        __syncthreads();                                                // (the next frame's first round writes the LDS slots a slow thread may still read)
    }
}

// The blocks of a call, the longest-running first: a block per room beyond WAVE_ROOM members; a wave per room up to it; a run of
// SEG_ROOM lanes per room up to that; a lane per lone stream.
__global__ void __launch_bounds__(PICK_THREADS) k_pick_rank(PickRankArgs a)
{
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (b < a.b_wav) pick_rank_block(a, a.cls[b]);
    else if (b < a.b_seg) {
        const int q = (b - a.b_wav) * (PICK_THREADS / PICK_WAVE) + tid / PICK_WAVE;
        pick_rank_lanes<PICK_WAVE>(a, q < a.n_wav ? a.cls[a.n_blk + q] : -1, tid % PICK_WAVE);
    } else if (b < a.b_one) {
        const int q = (b - a.b_seg) * (PICK_THREADS / PICK_SEG) + tid / PICK_SEG;
        pick_rank_lanes<PICK_SEG>(a, q < a.n_seg ? a.cls[a.n_blk + a.n_wav + q] : -1, tid % PICK_SEG);
    } else {
        const int q = (b - a.b_one) * PICK_THREADS + tid;
        pick_rank_lanes<1>(a, q < a.n_one ? a.cls[a.n_blk + a.n_wav + a.n_seg + q] : -1, 0);
    }
}

// level and selected of the flagged streams to their reset values
__global__ void __launch_bounds__(256) k_pick_clear(const unsigned char *flag, double *level, unsigned char *sel, int S)
{
    const int s = (int)(blockIdx.x * 256 + threadIdx.x);
    if (s < S && flag[s]) level[s] = 0.0, sel[s] = 0;
}

// ---- the host side ------------------------------------------------------------------------------------------------------------------------
struct nnn_pick {
    int S = 0, device = 0;
    int n_blk = 0, n_wav = 0, n_seg = 0, n_one = 0;
    int K = 3;
    float decay = 0.875f, stick = 4.0f;
    std::vector<int32_t> room;                      // as the host set them; the tables are made from them
    std::vector<uint8_t> pinned;
    // page-locked staging of what the setters upload: off [S + 1], mem [S], cls [S] (ints), then pin [S], then flag [S] (bytes)
    int *stage = nullptr;
    int *d_off = nullptr, *d_mem = nullptr, *d_cls = nullptr;
    unsigned char *d_pin = nullptr, *d_sel = nullptr;
    double *d_level = nullptr;
    unsigned long long *d_key = nullptr;
    unsigned char *d_flag = nullptr;                // [S]: the streams a reset names
    double *d_e = nullptr;                          // [T][S] of the longest call (grow only)
    size_t e_cap = 0;                               // stream-frames
    hipStream_t own_stream = nullptr;
    hipEvent_t ev_last = nullptr;                   // end of the most recent call, on the stream it was made on
    hipStream_t last_stream = nullptr;
    bool have_last = false;
    // device buffers of the host entry point (made on first use, grow only)
    float *h_in = nullptr;
    unsigned char *h_open = nullptr, *h_live = nullptr, *h_talk = nullptr;
    int32_t *h_dom = nullptr;
    double *h_level = nullptr;
    size_t h_in_cap = 0, h_open_cap = 0, h_live_cap = 0, h_talk_cap = 0, h_dom_cap = 0, h_level_cap = 0;   // bytes
};

extern "C" void nnn_pick_destroy(nnn_pick *h)
{
    if (!h) return;
    NNN_RT_LOCK;
    hipSetDevice(h->device);
    if (h->have_last) hipEventSynchronize(h->ev_last);
    hipFree(h->d_off); hipFree(h->d_mem); hipFree(h->d_cls); hipFree(h->d_pin); hipFree(h->d_sel); hipFree(h->d_level); hipFree(h->d_key);
    hipFree(h->d_flag); hipFree(h->d_e);
    hipFree(h->h_in); hipFree(h->h_open); hipFree(h->h_live); hipFree(h->h_talk); hipFree(h->h_dom); hipFree(h->h_level);
    if (h->stage) hipHostFree(h->stage);
    if (h->own_stream) hipStreamDestroy(h->own_stream);
    if (h->ev_last) hipEventDestroy(h->ev_last);
    delete h;
}

// everything enqueued so far is done
static int pick_drain(nnn_pick *h)
{
    HIPCHK(hipSetDevice(h->device));
    if (h->have_last) HIPCHK(hipEventSynchronize(h->ev_last));
    return 0;
}

// The member tables from the host's rooms, and the pins, to the device; the caller holds the lock and has drained the object.  A room's
// members are its streams in ascending index (the streams are walked in that order); the rooms themselves are numbered by their first
// member, so no table depends on the labels.  The class lists hold the rooms in that numbering, the lone streams as themselves.
static int pick_upload(nnn_pick *h)
{
    const size_t S = (size_t)h->S;
    int *off = h->stage, *mem = off + S + 1, *cls = mem + S;
    unsigned char *pin = (unsigned char *)(cls + S);
    std::vector<int> of_label(S, -1), room_of(S), count;
    for (size_t s = 0; s < S; s++) {
        const int32_t label = h->room[s];
        int r = label < 0 ? -1 : of_label[(size_t)label];
        if (r < 0) {
            r = (int)count.size();
            count.push_back(0);
            if (label >= 0) of_label[(size_t)label] = r;
        }
        room_of[s] = r, count[(size_t)r]++;
    }
    const size_t R = count.size();
    off[0] = 0;
    for (size_t r = 0; r < R; r++) off[r + 1] = off[r] + count[r];
    std::vector<int> at(off, off + R);
    for (size_t s = 0; s < S; s++) mem[at[(size_t)room_of[s]]++] = (int)s;
    int n = 0;
    h->n_blk = h->n_wav = h->n_seg = h->n_one = 0;
    for (size_t r = 0; r < R; r++)
        if (count[r] > NNN_PICK_WAVE_ROOM) cls[n++] = (int)r, h->n_blk++;
    for (size_t r = 0; r < R; r++)
        if (count[r] > NNN_PICK_SEG_ROOM && count[r] <= NNN_PICK_WAVE_ROOM) cls[n++] = (int)r, h->n_wav++;
    for (size_t r = 0; r < R; r++)
        if (count[r] > 1 && count[r] <= NNN_PICK_SEG_ROOM) cls[n++] = (int)r, h->n_seg++;
    for (size_t r = 0; r < R; r++)
        if (count[r] == 1) cls[n++] = mem[off[r]], h->n_one++;
    for (size_t s = 0; s < S; s++) pin[s] = h->pinned[s];
    HIPCHK(hipMemcpy(h->d_off, off, (R + 1) * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_mem, mem, S * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_cls, cls, (size_t)n * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_pin, pin, S, hipMemcpyHostToDevice));
    return 0;
}

extern "C" nnn_pick *nnn_pick_create(int n_streams, int device)
{
    if (n_streams < 1 || n_streams > 0x0fffffff) { fail("nnn_pick_create: n_streams = %d", n_streams); return nullptr; }
    NNN_RT_LOCK;
    if (hipSetDevice(device) != hipSuccess) { fail("nnn_pick_create: no such HIP device"); return nullptr; }
    nnn_pick *h = new nnn_pick();
    h->S = n_streams, h->device = device;
    h->room.assign((size_t)n_streams, -1);
    h->pinned.assign((size_t)n_streams, 0);
    const size_t S = (size_t)n_streams;
    bool ok = true;
    auto dev = [&](auto **q, size_t bytes) { ok = ok && hipMalloc((void **)q, bytes) == hipSuccess && hipMemset(*q, 0, bytes) == hipSuccess; };
    dev(&h->d_off, (S + 1) * sizeof(int)), dev(&h->d_mem, S * sizeof(int)), dev(&h->d_cls, S * sizeof(int));
    dev(&h->d_pin, S), dev(&h->d_sel, S), dev(&h->d_flag, S);
    dev(&h->d_level, S * sizeof(double)), dev(&h->d_key, S * sizeof(unsigned long long));
    ok = ok && hipHostMalloc((void **)&h->stage, (3 * S + 1) * sizeof(int) + 2 * S, hipHostMallocDefault) == hipSuccess;
    ok = ok && hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&h->ev_last, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipDeviceSynchronize() == hipSuccess;   // (the memsets above are on the legacy stream; the calls are on non-blocking ones)
    ok = ok && pick_upload(h) == 0;
    if (!ok) {
        nnn_pick_destroy(h);
        fail("nnn_pick_create: allocation failed (about 40 bytes for each of %d streams)", n_streams);
        return nullptr;
    }
    return h;
}

// an index list of a call: inside the object, and no stream twice where `once` asks for that
static int pick_streams(const nnn_pick *h, const int *idx, int n, bool once, const char *who)
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

extern "C" int nnn_pick_set_rooms(nnn_pick *h, const int *idx, int n, const int32_t *room)
{
    const char *who = "nnn_pick_set_rooms";
    if (!h) return fail("null picker");
    if (int rc = pick_streams(h, idx, n, true, who)) return rc;
    if (n == 0) return 0;
    if (!room) return fail("%s: null rooms", who);
    for (int i = 0; i < n; i++)
        if (room[i] < -1 || room[i] >= h->S) return fail("%s: entry %d: room %d outside [-1, %d)", who, i, (int)room[i], h->S);
    NNN_RT_LOCK;
    if (int rc = pick_drain(h)) return rc;
    for (int i = 0; i < n; i++) h->room[(size_t)(idx ? idx[i] : i)] = room[i];
    return pick_upload(h);
}

extern "C" int nnn_pick_get_rooms(nnn_pick *h, const int *idx, int n, int32_t *room)
{
    if (!h) return fail("null picker");
    if (int rc = pick_streams(h, idx, n, false, "nnn_pick_get_rooms")) return rc;
    if (n == 0) return 0;
    if (!room) return fail("nnn_pick_get_rooms: null rooms");
    for (int i = 0; i < n; i++) room[i] = h->room[(size_t)(idx ? idx[i] : i)];
    return 0;
}

extern "C" int nnn_pick_set_pinned(nnn_pick *h, const int *idx, int n, const uint8_t *pinned)
{
    const char *who = "nnn_pick_set_pinned";
    if (!h) return fail("null picker");
    if (int rc = pick_streams(h, idx, n, true, who)) return rc;
    if (n == 0) return 0;
    if (!pinned) return fail("%s: null pins", who);
    for (int i = 0; i < n; i++)
        if (pinned[i] > 1) return fail("%s: entry %d: pinned %d is neither 0 nor 1", who, i, (int)pinned[i]);
    NNN_RT_LOCK;
    if (int rc = pick_drain(h)) return rc;
    for (int i = 0; i < n; i++) h->pinned[(size_t)(idx ? idx[i] : i)] = pinned[i];
    return pick_upload(h);
}

extern "C" int nnn_pick_get_pinned(nnn_pick *h, const int *idx, int n, uint8_t *pinned)
{
    if (!h) return fail("null picker");
    if (int rc = pick_streams(h, idx, n, false, "nnn_pick_get_pinned")) return rc;
    if (n == 0) return 0;
    if (!pinned) return fail("nnn_pick_get_pinned: null pins");
    for (int i = 0; i < n; i++) pinned[i] = h->pinned[(size_t)(idx ? idx[i] : i)];
    return 0;
}

extern "C" int nnn_pick_set_policy(nnn_pick *h, int k, float decay, float stick)
{
    const char *who = "nnn_pick_set_policy";
    if (!h) return fail("null picker");
    if (k < 1 || k > NNN_PICK_MAX_K) return fail("%s: k = %d outside [1, %d]", who, k, NNN_PICK_MAX_K);
    if (!(decay >= 0.0f && decay <= 1.0f)) return fail("%s: decay %g outside [0, 1]", who, (double)decay);
    if (!(stick >= 1.0f && stick <= (float)NNN_PICK_MAX_STICK)) return fail("%s: stick %g outside [1, %d]", who, (double)stick, NNN_PICK_MAX_STICK);
    NNN_RT_LOCK;
    if (int rc = pick_drain(h)) return rc;
    h->K = k, h->decay = decay, h->stick = stick;
    return 0;
}

extern "C" int nnn_pick_get_policy(nnn_pick *h, int *k, float *decay, float *stick)
{
    if (!h) return fail("null picker");
    if (k) *k = h->K;
    if (decay) *decay = h->decay;
    if (stick) *stick = h->stick;
    return 0;
}

extern "C" int nnn_pick_reset(nnn_pick *h, const int *idx, int n)
{
    if (!h) return fail("null picker");
    if (!idx) n = h->S;
    if (int rc = pick_streams(h, idx, n, false, "nnn_pick_reset")) return rc;
    if (n == 0) return 0;
    NNN_RT_LOCK;
    if (int rc = pick_drain(h)) return rc;
    unsigned char *flag = (unsigned char *)(h->stage + 3 * (size_t)h->S + 1) + (size_t)h->S;
    memset(flag, 0, (size_t)h->S);
    for (int i = 0; i < n; i++) flag[(size_t)(idx ? idx[i] : i)] = 1;
    HIPCHK(hipMemcpy(h->d_flag, flag, (size_t)h->S, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_pick_clear, dim3((unsigned)((h->S + 255) / 256)), dim3(256), 0, h->own_stream, (const unsigned char *)h->d_flag, h->d_level, h->d_sel,
                       h->S);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->own_stream));
    return 0;
}

// one call on the unified addressing: element (s, t, i) at (s / C) * gs + t * fs + i * C + s % C; everything is validated by now
static int pick_enqueue(nnn_pick *h, int fmt, const void *d_in, const uint8_t *d_open, const uint8_t *d_live, uint8_t *d_talk, int32_t *d_dominant,
                        double *d_level, int n_frames, int C, size_t gs, size_t fs, void *hip_stream)
{
    HIPCHK(hipSetDevice(h->device));
    const size_t rows = (size_t)n_frames * h->S;
    if (rows > h->e_cap) {
        NNN_RT_LOCK;
        if (int rc = pick_drain(h)) return rc;
        HIPCHK(hipFree(h->d_e));
        h->d_e = nullptr, h->e_cap = 0;
        HIPCHK(hipMalloc((void **)&h->d_e, rows * sizeof(double)));
        h->e_cap = rows;
    }
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : h->own_stream;
    if (h->have_last && h->last_stream != st) HIPCHK(hipStreamWaitEvent(st, h->ev_last, 0));   // (state and scratch are the previous call's until then)
    PickLevelArgs la = {};
    la.in = (const char *)d_in, la.open = d_open, la.live = d_live, la.e = h->d_e, la.gs = (long long)gs, la.fs = (long long)fs;
    la.S = h->S, la.T = n_frames, la.C = C;
    const unsigned sblocks = (unsigned)((h->S + PICK_WAVES - 1) / PICK_WAVES), runs = (unsigned)((n_frames + PICK_RUN - 1) / PICK_RUN);
    const dim3 lgrid(sblocks, runs < 65535u ? runs : 65535u), lblock(64 * PICK_WAVES);
    if (fmt == PCM_I16) hipLaunchKernelGGL(k_pick_level<PCM_I16>, lgrid, lblock, 0, st, la);
    else if (fmt == PCM_F32_UNIT) hipLaunchKernelGGL(k_pick_level<PCM_F32_UNIT>, lgrid, lblock, 0, st, la);
    else hipLaunchKernelGGL(k_pick_level<PCM_F32>, lgrid, lblock, 0, st, la);
    PickRankArgs a = {};
    a.e = h->d_e, a.open = d_open, a.live = d_live, a.talk = d_talk, a.dominant = d_dominant, a.level_out = d_level;
    a.level = h->d_level, a.sel = h->d_sel, a.key = h->d_key, a.pin = h->d_pin, a.off = h->d_off, a.mem = h->d_mem, a.cls = h->d_cls;
    a.n_blk = h->n_blk, a.n_wav = h->n_wav, a.n_seg = h->n_seg, a.n_one = h->n_one;
    a.b_wav = h->n_blk;
    a.b_seg = a.b_wav + (h->n_wav + PICK_THREADS / PICK_WAVE - 1) / (PICK_THREADS / PICK_WAVE);
    a.b_one = a.b_seg + (h->n_seg + PICK_THREADS / PICK_SEG - 1) / (PICK_THREADS / PICK_SEG);
    a.S = h->S, a.T = n_frames, a.K = h->K, a.decay = (double)h->decay, a.stick = (double)h->stick;
    const unsigned blocks = (unsigned)(a.b_one + (h->n_one + PICK_THREADS - 1) / PICK_THREADS);
    hipLaunchKernelGGL(k_pick_rank, dim3(blocks), dim3(PICK_THREADS), 0, st, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev_last, st));
    h->last_stream = st;
    h->have_last = true;
    return 0;
}

static int pick_call_ok(const nnn_pick *h, const void *d_in, const void *d_talk, const void *d_dominant, const void *d_level, int n_frames)
{
    if (!h) return fail("null picker");
    if (!d_in) return fail("nnn_pick_select: null input");
    if (!d_talk) return fail("nnn_pick_select: null talk rows");
    if (n_frames < 1) return fail("nnn_pick_select: n_frames = %d", n_frames);
    if ((long long)n_frames * h->S > 0x7fffffffll) return fail("nnn_pick_select: %d frames of %d streams are more than a call holds", n_frames, h->S);
    if ((uintptr_t)d_dominant & 3) return fail("nnn_pick_select: the dominant rows are not aligned to their 4-byte values");
    if ((uintptr_t)d_level & 7) return fail("nnn_pick_select: the level rows are not aligned to their 8-byte values");
    return 0;
}

extern "C" int nnn_pick_select_device(nnn_pick *h, const float *d_in, const uint8_t *d_open, const uint8_t *d_live, uint8_t *d_talk, int32_t *d_dominant,
                                      double *d_level, int n_frames, size_t stream_stride, size_t frame_stride, void *hip_stream)
{
    if (int rc = pick_call_ok(h, d_in, d_talk, d_dominant, d_level, n_frames)) return rc;
    if (frame_stride < (size_t)FRAME) return fail("nnn_pick_select: frame_stride = %zu is below a frame's %d elements", frame_stride, FRAME);
    if ((uintptr_t)d_in & 3) return fail("nnn_pick_select: the audio is not aligned to its 4-byte samples");
    return pick_enqueue(h, PCM_F32, d_in, d_open, d_live, d_talk, d_dominant, d_level, n_frames, 1, stream_stride, frame_stride, hip_stream);
}

extern "C" int nnn_pick_select_pcm_device(nnn_pick *h, const void *d_in, const uint8_t *d_open, const uint8_t *d_live, uint8_t *d_talk,
                                          int32_t *d_dominant, double *d_level, int n_frames, const nnn_pcm_layout *layout, void *hip_stream)
{
    if (int rc = pick_call_ok(h, d_in, d_talk, d_dominant, d_level, n_frames)) return rc;
    if (!layout) return fail("nnn_pick_select: null layout");
    const int fmt = layout->format, C = layout->channels;
    if (fmt != PCM_F32 && fmt != PCM_I16 && fmt != PCM_F32_UNIT) return fail("nnn_pick_select: bad format %d", fmt);
    if (C < 1 || h->S % C) return fail("nnn_pick_select: channels = %d does not divide the %d streams", C, h->S);
    if (layout->discard_first) return fail("nnn_pick_select: discard_first must be 0");
    if (layout->frame_stride < (size_t)FRAME * C) return fail("nnn_pick_select: frame_stride = %zu is below a frame's %d elements", layout->frame_stride, FRAME * C);
    if ((uintptr_t)d_in & (fmt == PCM_I16 ? 1 : 3)) return fail("nnn_pick_select: the audio is not aligned to its %d-byte samples", fmt == PCM_I16 ? 2 : 4);
    return pick_enqueue(h, fmt, d_in, d_open, d_live, d_talk, d_dominant, d_level, n_frames, C, layout->group_stride, layout->frame_stride, hip_stream);
}

template <class T> static int pick_room(nnn_pick *h, T *&q, size_t &cap, size_t bytes)
{
    if (bytes <= cap) return 0;
    NNN_RT_LOCK;
    if (int rc = pick_drain(h)) return rc;
    HIPCHK(hipFree(q));
    q = nullptr, cap = 0;
    HIPCHK(hipMalloc((void **)&q, bytes));
    cap = bytes;
    return 0;
}

extern "C" int nnn_pick_select_host(nnn_pick *h, const float *in, const uint8_t *open, const uint8_t *live, uint8_t *talk, int32_t *dominant,
                                    double *level, int n_frames)
{
    if (int rc = pick_call_ok(h, in, talk, nullptr, nullptr, n_frames)) return rc;
    HIPCHK(hipSetDevice(h->device));
    const size_t S = (size_t)h->S, rows = (size_t)n_frames * S, per = (size_t)n_frames * FRAME;
    if (int rc = pick_room(h, h->h_in, h->h_in_cap, rows * FRAME * sizeof(float))) return rc;
    if (int rc = pick_room(h, h->h_talk, h->h_talk_cap, rows)) return rc;
    if (open)
        if (int rc = pick_room(h, h->h_open, h->h_open_cap, rows)) return rc;
    if (live)
        if (int rc = pick_room(h, h->h_live, h->h_live_cap, S)) return rc;
    if (dominant)
        if (int rc = pick_room(h, h->h_dom, h->h_dom_cap, rows * sizeof(int32_t))) return rc;
    if (level)
        if (int rc = pick_room(h, h->h_level, h->h_level_cap, rows * sizeof(double))) return rc;
    hipStream_t st = h->own_stream;
    if (h->have_last && h->last_stream != st) HIPCHK(hipStreamWaitEvent(st, h->ev_last, 0));   // (the staging may be an earlier call's until then)
    HIPCHK(hipMemcpyAsync(h->h_in, in, rows * FRAME * sizeof(float), hipMemcpyHostToDevice, st));
    if (open) HIPCHK(hipMemcpyAsync(h->h_open, open, rows, hipMemcpyHostToDevice, st));
    if (live) HIPCHK(hipMemcpyAsync(h->h_live, live, S, hipMemcpyHostToDevice, st));
    if (int rc = pick_enqueue(h, PCM_F32, h->h_in, open ? h->h_open : nullptr, live ? h->h_live : nullptr, h->h_talk, dominant ? h->h_dom : nullptr,
                              level ? h->h_level : nullptr, n_frames, 1, per, FRAME, st))
        return rc;
    std::vector<uint8_t> tk;
    std::vector<int32_t> dm;
    std::vector<double> lv;
    if (live) tk.resize(rows), dm.resize(dominant ? rows : 0), lv.resize(level ? rows : 0);
    HIPCHK(hipMemcpyAsync(live ? tk.data() : talk, h->h_talk, rows, hipMemcpyDeviceToHost, st));
    if (dominant) HIPCHK(hipMemcpyAsync(live ? dm.data() : dominant, h->h_dom, rows * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (level) HIPCHK(hipMemcpyAsync(live ? lv.data() : level, h->h_level, rows * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (live)
        for (size_t t = 0; t < (size_t)n_frames; t++)
            for (size_t s = 0; s < S; s++)
                if (live[s]) {
                    talk[t * S + s] = tk[t * S + s];
                    if (dominant) dominant[t * S + s] = dm[t * S + s];
                    if (level) level[t * S + s] = lv[t * S + s];
                }
    return 0;
}
