// nnn_mix.hip -- the conference mixer (include/nnn_mix.h): per-room mix-minus behind the VAD gate.
// One call = k_mix_sum (a block per listener tile and frame: the room's audible terms summed in binary64 in the one stated order, every
// listener of the tile handed the total less its own term) and k_mix_carry (a lane per stream: prev = the last frame's gain), on the
// caller's stream.  The member tables (rooms as CSR, listener tiles) are made on the host by the setters.
// Needs fail / HIPCHK / NNN_RT_LOCK (nnn_batch_core.hip), pcm_to_unit and the PCM_* formats (nnn_common.hip), Gate4 / gate_load /
// gate_store (nnn_gate.hip).
#pragma once

#include "../../include/nnn_mix.h"

// ---- the kernels ------------------------------------------------------------------------------------------------------------------------
constexpr int MIX_THREADS = 128;                      // 120 of them own four consecutive samples of the block's frame; all 128 scan members
constexpr int MIX_VEC = GATE_VEC;
constexpr int MIX_REG = NNN_MIX_REG_TALKERS;
constexpr int MIX_AHEAD = 4;                          // audible inputs a thread fetches before it adds the first of them
static_assert(FRAME == NNN_MIX_FRAME && MIX_VEC == 4 && FRAME / MIX_VEC <= MIX_THREADS && NNN_MIX_TILE <= 32 && MIX_THREADS % 32 == 0, "");

struct MixArgs {
    const char *in;                   // element (s, t, i) at (s / C) * gs + t * fs + i * C + s % C, in elements of the side's format
    char *out;
    const unsigned char *talk;        // NULL or [T][S]
    const unsigned char *live;        // NULL or [S]
    int *heard;                       // NULL or [T][S]
    const float *gain, *prev;         // [S]
    const float *ramp;                // [480]: (float)(i + 1) / 480.0f
    const int *off, *mem;             // rooms as CSR: room r's members, ascending, are mem[off[r] .. off[r + 1])
    const int *tile;                  // [nt][3]: room, first position in mem, listeners
    long long igs, ifs, ogs, ofs;
    int S, T, nt, iC, oC;
    int iwide, owide;                 // the side's frames are whole aligned 16-byte words (int16: 8-byte) for every thread: mix_load
};

struct Mix4 { double v[MIX_VEC]; };

// what a scan leaves in LDS: stream and gains of the members it looked at, a bit per member for "live" and for "audible"
struct MixScan {
    int s[MIX_THREADS];
    float hp[MIX_THREADS], hn[MIX_THREADS];
    unsigned flag[MIX_THREADS / 4];                        // a byte per member: bit 0 live, bit 1 audible
    unsigned live[MIX_THREADS / 32], aud[MIX_THREADS / 32]; // the same as a bit per member
};

// a value every thread of the block holds alike, moved to where the compiler knows it (scalar registers, uniform branches)
__device__ __forceinline__ int mix_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float mix_uniform(float v) { return __uint_as_float((unsigned)__builtin_amdgcn_readfirstlane((int)__float_as_uint(v))); }
__device__ __forceinline__ unsigned mix_uniform(unsigned v) { return (unsigned)__builtin_amdgcn_readfirstlane((int)v); }

// Steps 1 and 3 for the members mem[base .. base + cnt), cnt <= MIX_THREADS, a thread each: the serial part of a room-frame -- who is
// live, who is audible -- costs one round of loads for 128 members instead of a chain of dependent loads for each.  `alone`: a room of
// one, whose gains nobody needs.  The flags go to LDS as bytes, eight threads pack them into the bit masks the loops walk (four bytes
// at a time, by a multiplication that moves bit 0 of each byte into one nibble).  Ends in a barrier; the caller puts another one before
// the next scan.
__device__ __forceinline__ void mix_scan(const MixArgs &a, MixScan &L, int base, int cnt, int t, bool alone)
{
    const int tid = (int)threadIdx.x;
    bool live = false, aud = false;
    if (tid < cnt) {
        const int s = a.mem[base + tid];
        live = !a.live || a.live[s];
        float hp = 0.0f, hn = 0.0f;
        if (live && !alone) {
            const float g = a.gain[s];
            hn = !a.talk || a.talk[(size_t)t * a.S + s] ? g : 0.0f;
            hp = t == 0 ? a.prev[s] : !a.talk || a.talk[(size_t)(t - 1) * a.S + s] ? g : 0.0f;
        }
        aud = hp != 0.0f || hn != 0.0f;
        L.s[tid] = s, L.hp[tid] = hp, L.hn[tid] = hn;
    }
    ((unsigned char *)L.flag)[tid] = (unsigned char)((live ? 1 : 0) | (aud ? 2 : 0));
    __syncthreads();
    if (tid < 2 * (MIX_THREADS / 32)) {
        const int kind = tid / (MIX_THREADS / 32), word = tid % (MIX_THREADS / 32);
        unsigned bits = 0;
#pragma unroll
        for (int b = 0; b < 8; b++) bits |= ((((L.flag[word * 8 + b] >> kind) & 0x01010101u) * 0x01020408u) >> 24 & 0xFu) << (4 * b);
        (kind ? L.aud : L.live)[word] = bits;
    }
    __syncthreads();
}

// Four floats / four int16 as one word of the memory system.  Native vector types: through `uint4` the compiler splits the access into
// 4-byte ones (DESIGN.md section 24 saw it in the gate's loads).
typedef unsigned mix_u4 __attribute__((vector_size(16)));
typedef unsigned mix_u2 __attribute__((vector_size(8)));

// The thread's four samples of frame t of stream s as the bits of floats (int16 converted, unit floats not yet scaled).  Where the side
// is "wide" -- one channel, base and strides multiples of four elements, which the host works out once a call -- they are one aligned
// 16-byte word (8 bytes for int16); otherwise the gate's loader goes word by word or element by element.
template <int FMT> __device__ __forceinline__ Gate4 mix_load(const MixArgs &a, int s, int t, int i0)
{
    const long long e = (long long)(s / a.iC) * a.igs + (long long)t * a.ifs + (long long)i0 * a.iC + s % a.iC;
    if (a.iwide) {
        Gate4 r;
        if (FMT == PCM_I16) {
            const mix_u2 w = *(const mix_u2 *)((const short *)a.in + e);
            r.v[0] = __float_as_uint(pk_s16(w[0])), r.v[1] = __float_as_uint(pk_s16(w[0] >> 16));
            r.v[2] = __float_as_uint(pk_s16(w[1])), r.v[3] = __float_as_uint(pk_s16(w[1] >> 16));
        } else {
            const mix_u4 w = *(const mix_u4 *)((const unsigned *)a.in + e);
            r.v[0] = w[0], r.v[1] = w[1], r.v[2] = w[2], r.v[3] = w[3];
        }
        return r;
    }
    return FMT == PCM_I16 ? gate_load<PCM_I16>(a.in, e, a.iC) : gate_load<PCM_F32>(a.in, e, a.iC);
}

// the thread's four outputs of frame t of stream s through the format's writer (the unit scaling is the caller's), the same way
template <int FMT> __device__ __forceinline__ void mix_store(const MixArgs &a, int s, int t, int i0, const Gate4 &y)
{
    const long long e = (long long)(s / a.oC) * a.ogs + (long long)t * a.ofs + (long long)i0 * a.oC + s % a.oC;
    if (a.owide) {
        if (FMT == PCM_I16) {
            unsigned h[MIX_VEC];
#pragma unroll
            for (int q = 0; q < MIX_VEC; q++) h[q] = (unsigned short)pcm_to_i16(__uint_as_float(y.v[q]));
            mix_u2 w;
            w[0] = h[0] | h[1] << 16, w[1] = h[2] | h[3] << 16;
            *(mix_u2 *)((short *)a.out + e) = w;
        } else {
            mix_u4 w;
            w[0] = y.v[0], w[1] = y.v[1], w[2] = y.v[2], w[3] = y.v[3];
            *(mix_u4 *)((unsigned *)a.out + e) = w;
        }
        return;
    }
    if (FMT == PCM_I16) gate_store<PCM_I16>(a.out, e, a.oC, y);
    else gate_store<PCM_F32>(a.out, e, a.oC, y);
}

// steps 2 and 4: the four terms of an audible stream-frame
template <int FMT> __device__ __forceinline__ Mix4 mix_term(const Gate4 &x, float hp, float hn, const float *ramp)
{
#pragma clang fp contract(off)
    Mix4 c;
#pragma unroll
    for (int q = 0; q < MIX_VEC; q++) {
        float v = __uint_as_float(x.v[q]);
        if (FMT == PCM_F32_UNIT) v = v * 32768.0f;
        const float g = hp == hn ? hn : hp + (hn - hp) * ramp[q];
        c.v[q] = (double)v * (double)g;
    }
    return c;
}

// Steps 1 to 7 of the header's rule for one (listener tile, frame).  The room's members are scanned 128 at a time (mix_scan); what
// decides the control flow afterwards -- the audible bits, the streams, the gains -- is block-uniform and handed to the scalar unit,
// so the loops below branch uniformly.  The audible members are walked in ascending stream index, through the set bits of the scan's
// mask: T in that order whatever the tile, so every tile of a room gets the same bits without talking to the others.  The inputs of up
// to MIX_AHEAD audible members are fetched before the first of them is added; the first MIX_REG terms stay in registers (written and read
// through unrolled compares: an array indexed at run time would live in scratch).  Then the tile's listeners, scanned the same way: the
// inaudible ones all get the same (float)T and their inputs are never read; an audible one gets T less its own term, from the registers
// or, beyond MIX_REG, recomputed from a second read of its input (the same operations on the same bits: the same term).  The eight
// threads without samples take part in the scans and the barriers and touch no audio.
template <int IFMT, int OFMT> __global__ void __launch_bounds__(MIX_THREADS) k_mix_sum(MixArgs a)
{
#pragma clang fp contract(off)
    __shared__ MixScan L;
    const int tile = (int)(blockIdx.x % (unsigned)a.nt), t = (int)(blockIdx.x / (unsigned)a.nt);
    const int i0 = (int)threadIdx.x * MIX_VEC;
    const bool active = i0 < FRAME;
    const int room = a.tile[3 * tile], lo = a.tile[3 * tile + 1], n = a.tile[3 * tile + 2];
    const int m0 = a.off[room], m1 = a.off[room + 1];
    float ramp[MIX_VEC] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (active) {
        const float4 rp = *(const float4 *)(a.ramp + i0);
        ramp[0] = rp.x, ramp[1] = rp.y, ramp[2] = rp.z, ramp[3] = rp.w;
    }

    Mix4 total, reg[MIX_REG];
#pragma unroll
    for (int q = 0; q < MIX_VEC; q++) total.v[q] = 0.0;
#pragma unroll
    for (int j = 0; j < MIX_REG; j++)
#pragma unroll
        for (int q = 0; q < MIX_VEC; q++) reg[j].v[q] = 0.0;
    int A = 0, ord = 0;                                             // audible members so far; those ahead of the tile's first listener
    if (m1 - m0 > 1)                                                // (a room of one: +0.0, nothing read)
        for (int base = m0; base < m1; base += MIX_THREADS) {
            mix_scan(a, L, base, min(MIX_THREADS, m1 - base), t, false);
            // A room that fits one scan and has a single live member: nobody is there to hear it, so its input is not read either (the
            // term of zeros below gives the +0.0 the rule gives).  Larger rooms would need a pass of their own to know; they read it.
            bool solo = false;
            if (m1 - m0 <= MIX_THREADS) {
                int alive = 0;
                for (int w = 0; w < MIX_THREADS / 32; w++) alive += __builtin_popcount(mix_uniform(L.live[w]));
                solo = alive == 1;
            }
            for (int w = 0; w < MIX_THREADS / 32; w++) {
                unsigned m = mix_uniform(L.aud[w]);
                while (m) {
                    Gate4 x[MIX_AHEAD] = {};
                    float hp[MIX_AHEAD], hn[MIX_AHEAD];
                    int at[MIX_AHEAD], got = 0;
#pragma unroll
                    for (int u = 0; u < MIX_AHEAD; u++) {
                        if (!m) break;
                        const int j = __builtin_ctz(m) + 32 * w;
                        m &= m - 1;
                        hp[u] = mix_uniform(L.hp[j]), hn[u] = mix_uniform(L.hn[j]), at[u] = base + j, got = u + 1;
                        if (active && !solo) x[u] = mix_load<IFMT>(a, mix_uniform(L.s[j]), t, i0);
                    }
#pragma unroll
                    for (int u = 0; u < MIX_AHEAD; u++) {
                        if (u >= got) break;
                        if (at[u] < lo) ord++;
                        const Mix4 c = mix_term<IFMT>(x[u], hp[u], hn[u], ramp);
#pragma unroll
                        for (int q = 0; q < MIX_VEC; q++) total.v[q] = total.v[q] + c.v[q];
#pragma unroll
                        for (int j = 0; j < MIX_REG; j++)
                            if (A == j) reg[j] = c;
                        A++;
                    }
                }
            }
            __syncthreads();
        }

    Gate4 yt;                                                       // what every inaudible listener gets
#pragma unroll
    for (int q = 0; q < MIX_VEC; q++) {
        float y = (float)total.v[q];
        if (OFMT == PCM_F32_UNIT) y = pcm_to_unit(y);
        yt.v[q] = __float_as_uint(y);
    }
    mix_scan(a, L, lo, n, t, m1 - m0 == 1);
    const unsigned lives = mix_uniform(L.live[0]), auds = mix_uniform(L.aud[0]);
    for (int j = 0; j < n; j++) {
        if (!(lives >> j & 1)) continue;
        const int s = mix_uniform(L.s[j]);
        const bool aud = auds >> j & 1;
        Gate4 y = yt;
        if (aud) {
            Mix4 c = reg[0];                                        // (A == 1: not used, +0.0 whatever the sample)
            if (A == 2) c = ord == 0 ? reg[1] : reg[0];             // the other one's term
            else if (ord < MIX_REG) {
#pragma unroll
                for (int k = 1; k < MIX_REG; k++)
                    if (ord == k) c = reg[k];
            } else {
                Gate4 x = {};
                if (active) x = mix_load<IFMT>(a, s, t, i0);
                c = mix_term<IFMT>(x, mix_uniform(L.hp[j]), mix_uniform(L.hn[j]), ramp);
            }
#pragma unroll
            for (int q = 0; q < MIX_VEC; q++) {
                float v = A == 1 ? 0.0f : A == 2 ? (float)c.v[q] : (float)(total.v[q] - c.v[q]);
                if (OFMT == PCM_F32_UNIT) v = pcm_to_unit(v);
                y.v[q] = __float_as_uint(v);
            }
            ord++;
        }
        if (active) mix_store<OFMT>(a, s, t, i0, y);
        if (a.heard && threadIdx.x == 0) a.heard[(size_t)t * a.S + s] = A - (aud ? 1 : 0);
    }
}

// step 8, lane = stream: prev = h_(last frame) of the live streams.  A kernel of its own: the blocks of frame 0 read prev while the
// value to store is a later frame's, so it cannot be written in place inside k_mix_sum.
__global__ void __launch_bounds__(256) k_mix_carry(const unsigned char *talk, const unsigned char *live, const float *gain, float *prev, int S, int T)
{
    const int s = (int)(blockIdx.x * 256 + threadIdx.x);
    if (s >= S || (live && !live[s])) return;
    prev[s] = !talk || talk[(size_t)(T - 1) * S + s] ? gain[s] : 0.0f;
}

// prev of the flagged streams to its reset value
__global__ void __launch_bounds__(256) k_mix_clear(const unsigned char *flag, float *prev, int S)
{
    const int s = (int)(blockIdx.x * 256 + threadIdx.x);
    if (s < S && flag[s]) prev[s] = 0.0f;
}

// ---- the host side ------------------------------------------------------------------------------------------------------------------------
struct nnn_mix {
    int S = 0, device = 0, nt = 0;
    std::vector<int32_t> room;                      // as the host set them; the tables are made from them
    std::vector<float> gain;
    // page-locked staging of what the setters upload: off [S + 1], mem [S], tile [3 S] (ints), then gain [S], then flag [S]
    int *stage = nullptr;
    int *d_off = nullptr, *d_mem = nullptr, *d_tile = nullptr;
    float *d_gain = nullptr, *d_prev = nullptr, *d_ramp = nullptr;
    unsigned char *d_flag = nullptr;                // [S]: the streams a reset names
    hipStream_t own_stream = nullptr;
    hipEvent_t ev_last = nullptr;                   // end of the most recent call, on the stream it was made on
    hipStream_t last_stream = nullptr;
    bool have_last = false;
    // device buffers of the host entry point (made on first use, grow only)
    float *h_in = nullptr, *h_out = nullptr;
    unsigned char *h_talk = nullptr, *h_live = nullptr;
    int32_t *h_heard = nullptr;
    size_t h_in_cap = 0, h_out_cap = 0, h_talk_cap = 0, h_live_cap = 0, h_heard_cap = 0;   // bytes
};

extern "C" void nnn_mix_destroy(nnn_mix *h)
{
    if (!h) return;
    NNN_RT_LOCK;
    hipSetDevice(h->device);
    if (h->have_last) hipEventSynchronize(h->ev_last);
    hipFree(h->d_off); hipFree(h->d_mem); hipFree(h->d_tile); hipFree(h->d_gain); hipFree(h->d_prev); hipFree(h->d_ramp); hipFree(h->d_flag);
    hipFree(h->h_in); hipFree(h->h_out); hipFree(h->h_talk); hipFree(h->h_live); hipFree(h->h_heard);
    if (h->stage) hipHostFree(h->stage);
    if (h->own_stream) hipStreamDestroy(h->own_stream);
    if (h->ev_last) hipEventDestroy(h->ev_last);
    delete h;
}

// everything enqueued so far is done
static int mix_drain(nnn_mix *h)
{
    HIPCHK(hipSetDevice(h->device));
    if (h->have_last) HIPCHK(hipEventSynchronize(h->ev_last));
    return 0;
}

// The member tables from the host's rooms, and the gains, to the device; the caller holds the lock and has drained the object.  A room's
// members are its streams in ascending index (the streams are walked in that order); the rooms themselves are numbered by their first
// member, so no table depends on the labels.
static int mix_upload(nnn_mix *h)
{
    const size_t S = (size_t)h->S;
    int *off = h->stage, *mem = off + S + 1, *tile = mem + S;
    float *gain = (float *)(tile + 3 * S);
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
    int nt = 0;
    for (size_t r = 0; r < R; r++)
        for (int lo = off[r]; lo < off[r + 1]; lo += NNN_MIX_TILE, nt++)
            tile[3 * nt] = (int)r, tile[3 * nt + 1] = lo, tile[3 * nt + 2] = std::min(NNN_MIX_TILE, off[r + 1] - lo);
    for (size_t s = 0; s < S; s++) gain[s] = h->gain[s];
    h->nt = nt;
    HIPCHK(hipMemcpy(h->d_off, off, (R + 1) * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_mem, mem, S * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_tile, tile, (size_t)nt * 3 * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_gain, gain, S * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

extern "C" nnn_mix *nnn_mix_create(int n_streams, int device)
{
    if (n_streams < 1 || n_streams > 0x0fffffff) { fail("nnn_mix_create: n_streams = %d", n_streams); return nullptr; }
    NNN_RT_LOCK;
    if (hipSetDevice(device) != hipSuccess) { fail("nnn_mix_create: no such HIP device"); return nullptr; }
    nnn_mix *h = new nnn_mix();
    h->S = n_streams, h->device = device;
    h->room.assign((size_t)n_streams, -1);
    h->gain.assign((size_t)n_streams, 1.0f);
    const size_t S = (size_t)n_streams;
    bool ok = true;
    auto dev = [&](auto **q, size_t bytes) { ok = ok && hipMalloc((void **)q, bytes) == hipSuccess && hipMemset(*q, 0, bytes) == hipSuccess; };
    dev(&h->d_off, (S + 1) * sizeof(int)), dev(&h->d_mem, S * sizeof(int)), dev(&h->d_tile, 3 * S * sizeof(int));
    dev(&h->d_gain, S * sizeof(float)), dev(&h->d_prev, S * sizeof(float)), dev(&h->d_ramp, FRAME * sizeof(float));
    dev(&h->d_flag, S);
    ok = ok && hipHostMalloc((void **)&h->stage, (5 * S + 1) * sizeof(int) + S * sizeof(float) + S, hipHostMallocDefault) == hipSuccess;
    ok = ok && hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&h->ev_last, hipEventDisableTiming) == hipSuccess;
    if (ok) {
        float ramp[FRAME];
        for (int i = 0; i < FRAME; i++) ramp[i] = (float)(i + 1) / 480.0f;
        ok = hipMemcpy(h->d_ramp, ramp, sizeof(ramp), hipMemcpyHostToDevice) == hipSuccess;
    }
    ok = ok && hipDeviceSynchronize() == hipSuccess;   // (the memsets above are on the legacy stream; the calls are on non-blocking ones)
    ok = ok && mix_upload(h) == 0;
    if (!ok) {
        nnn_mix_destroy(h);
        fail("nnn_mix_create: allocation failed (about 30 bytes for each of %d streams)", n_streams);
        return nullptr;
    }
    return h;
}

// an index list of a call: inside the object, and no stream twice where `once` asks for that
static int mix_streams(const nnn_mix *h, const int *idx, int n, bool once, const char *who)
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

extern "C" int nnn_mix_set_rooms(nnn_mix *h, const int *idx, int n, const int32_t *room)
{
    const char *who = "nnn_mix_set_rooms";
    if (!h) return fail("null mixer");
    if (int rc = mix_streams(h, idx, n, true, who)) return rc;
    if (n == 0) return 0;
    if (!room) return fail("%s: null rooms", who);
    for (int i = 0; i < n; i++)
        if (room[i] < -1 || room[i] >= h->S) return fail("%s: entry %d: room %d outside [-1, %d)", who, i, (int)room[i], h->S);
    NNN_RT_LOCK;
    if (int rc = mix_drain(h)) return rc;
    for (int i = 0; i < n; i++) h->room[(size_t)(idx ? idx[i] : i)] = room[i];
    return mix_upload(h);
}

extern "C" int nnn_mix_get_rooms(nnn_mix *h, const int *idx, int n, int32_t *room)
{
    if (!h) return fail("null mixer");
    if (int rc = mix_streams(h, idx, n, false, "nnn_mix_get_rooms")) return rc;
    if (n == 0) return 0;
    if (!room) return fail("nnn_mix_get_rooms: null rooms");
    for (int i = 0; i < n; i++) room[i] = h->room[(size_t)(idx ? idx[i] : i)];
    return 0;
}

extern "C" int nnn_mix_set_gains(nnn_mix *h, const int *idx, int n, const float *gain)
{
    const char *who = "nnn_mix_set_gains";
    if (!h) return fail("null mixer");
    if (int rc = mix_streams(h, idx, n, true, who)) return rc;
    if (n == 0) return 0;
    if (!gain) return fail("%s: null gains", who);
    for (int i = 0; i < n; i++)
        if (!(gain[i] >= 0.0f && gain[i] <= (float)NNN_MIX_MAX_GAIN)) return fail("%s: entry %d: gain %g outside [0, %d]", who, i, (double)gain[i], NNN_MIX_MAX_GAIN);
    NNN_RT_LOCK;
    if (int rc = mix_drain(h)) return rc;
    for (int i = 0; i < n; i++) h->gain[(size_t)(idx ? idx[i] : i)] = gain[i];
    return mix_upload(h);
}

extern "C" int nnn_mix_get_gains(nnn_mix *h, const int *idx, int n, float *gain)
{
    if (!h) return fail("null mixer");
    if (int rc = mix_streams(h, idx, n, false, "nnn_mix_get_gains")) return rc;
    if (n == 0) return 0;
    if (!gain) return fail("nnn_mix_get_gains: null gains");
    for (int i = 0; i < n; i++) gain[i] = h->gain[(size_t)(idx ? idx[i] : i)];
    return 0;
}

extern "C" int nnn_mix_reset(nnn_mix *h, const int *idx, int n)
{
    if (!h) return fail("null mixer");
    if (!idx) n = h->S;
    if (int rc = mix_streams(h, idx, n, false, "nnn_mix_reset")) return rc;
    if (n == 0) return 0;
    NNN_RT_LOCK;
    if (int rc = mix_drain(h)) return rc;
    unsigned char *flag = (unsigned char *)(h->stage + 5 * (size_t)h->S + 1) + (size_t)h->S * sizeof(float);
    memset(flag, 0, (size_t)h->S);
    for (int i = 0; i < n; i++) flag[(size_t)(idx ? idx[i] : i)] = 1;
    HIPCHK(hipMemcpy(h->d_flag, flag, (size_t)h->S, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_mix_clear, dim3((unsigned)((h->S + 255) / 256)), dim3(256), 0, h->own_stream, (const unsigned char *)h->d_flag, h->d_prev, h->S);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->own_stream));
    return 0;
}

template <int IFMT> static void mix_launch(int ofmt, dim3 grid, hipStream_t st, const MixArgs &a)
{
    if (ofmt == PCM_I16) hipLaunchKernelGGL((k_mix_sum<IFMT, PCM_I16>), grid, dim3(MIX_THREADS), 0, st, a);
    else if (ofmt == PCM_F32_UNIT) hipLaunchKernelGGL((k_mix_sum<IFMT, PCM_F32_UNIT>), grid, dim3(MIX_THREADS), 0, st, a);
    else hipLaunchKernelGGL((k_mix_sum<IFMT, PCM_F32>), grid, dim3(MIX_THREADS), 0, st, a);
}

// one call on the unified addressing of each side; everything is validated by now
static int mix_enqueue(nnn_mix *h, const void *d_in, void *d_out, const uint8_t *d_talk, const uint8_t *d_live, int32_t *d_heard, int n_frames, int ifmt,
                       int iC, size_t igs, size_t ifs, int ofmt, int oC, size_t ogs, size_t ofs, void *hip_stream)
{
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : h->own_stream;
    if (h->have_last && h->last_stream != st) HIPCHK(hipStreamWaitEvent(st, h->ev_last, 0));   // (prev is the previous call's until then)
    MixArgs a = {};
    a.in = (const char *)d_in, a.out = (char *)d_out, a.talk = d_talk, a.live = d_live, a.heard = d_heard, a.gain = h->d_gain, a.prev = h->d_prev;
    a.ramp = h->d_ramp, a.off = h->d_off, a.mem = h->d_mem, a.tile = h->d_tile;
    a.igs = (long long)igs, a.ifs = (long long)ifs, a.ogs = (long long)ogs, a.ofs = (long long)ofs;
    a.S = h->S, a.T = n_frames, a.nt = h->nt, a.iC = iC, a.oC = oC;
    auto wide = [](const void *p, int fmt, int C, size_t gs, size_t fs) { return C == 1 && gs % 4 == 0 && fs % 4 == 0 && ((uintptr_t)p & (fmt == PCM_I16 ? 7 : 15)) == 0; };
    a.iwide = wide(d_in, ifmt, iC, igs, ifs), a.owide = wide(d_out, ofmt, oC, ogs, ofs);
    const dim3 grid((unsigned)((long long)h->nt * n_frames));
    if (ifmt == PCM_I16) mix_launch<PCM_I16>(ofmt, grid, st, a);
    else if (ifmt == PCM_F32_UNIT) mix_launch<PCM_F32_UNIT>(ofmt, grid, st, a);
    else mix_launch<PCM_F32>(ofmt, grid, st, a);
    hipLaunchKernelGGL(k_mix_carry, dim3((unsigned)((h->S + 255) / 256)), dim3(256), 0, st, d_talk, d_live, (const float *)h->d_gain, h->d_prev, h->S, n_frames);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev_last, st));
    h->last_stream = st;
    h->have_last = true;
    return 0;
}

static int mix_call_ok(const nnn_mix *h, const void *d_in, const void *d_out, int n_frames)
{
    if (!h) return fail("null mixer");
    if (!d_in || !d_out) return fail("nnn_mix_apply: null %s", d_in ? "output" : "input");
    if (n_frames < 1) return fail("nnn_mix_apply: n_frames = %d", n_frames);
    if ((long long)n_frames * h->S > 0x7fffffffll) return fail("nnn_mix_apply: %d frames of %d streams are more than a call holds", n_frames, h->S);
    if (d_in == d_out) return fail("nnn_mix_apply: the output overlaps the input (an output needs every member's input: no in-place call)");
    return 0;
}

extern "C" int nnn_mix_apply_device(nnn_mix *h, const float *d_in, float *d_out, const uint8_t *d_talk, const uint8_t *d_live, int32_t *d_heard,
                                    int n_frames, size_t in_stream_stride, size_t in_frame_stride, size_t out_stream_stride, size_t out_frame_stride,
                                    void *hip_stream)
{
    if (int rc = mix_call_ok(h, d_in, d_out, n_frames)) return rc;
    if (in_frame_stride < (size_t)FRAME) return fail("nnn_mix_apply: input frame_stride = %zu is below a frame's %d elements", in_frame_stride, FRAME);
    if (out_frame_stride < (size_t)FRAME) return fail("nnn_mix_apply: output frame_stride = %zu is below a frame's %d elements", out_frame_stride, FRAME);
    if (((uintptr_t)d_in | (uintptr_t)d_out | (uintptr_t)d_heard) & 3) return fail("nnn_mix_apply: the audio is not aligned to its 4-byte samples");
    return mix_enqueue(h, d_in, d_out, d_talk, d_live, d_heard, n_frames, PCM_F32, 1, in_stream_stride, in_frame_stride, PCM_F32, 1, out_stream_stride,
                       out_frame_stride, hip_stream);
}

static int mix_layout_ok(const nnn_mix *h, const nnn_pcm_layout *L, const void *p, const char *side)
{
    if (!L) return fail("nnn_mix_apply: null %s layout", side);
    const int fmt = L->format, C = L->channels;
    if (fmt != PCM_F32 && fmt != PCM_I16 && fmt != PCM_F32_UNIT) return fail("nnn_mix_apply: bad %s format %d", side, fmt);
    if (C < 1 || h->S % C) return fail("nnn_mix_apply: %s channels = %d does not divide the %d streams", side, C, h->S);
    if (L->discard_first) return fail("nnn_mix_apply: discard_first must be 0");
    if (L->frame_stride < (size_t)FRAME * C) return fail("nnn_mix_apply: %s frame_stride = %zu is below a frame's %d elements", side, L->frame_stride, FRAME * C);
    if ((uintptr_t)p & (fmt == PCM_I16 ? 1 : 3)) return fail("nnn_mix_apply: the %s is not aligned to its %d-byte samples", side, fmt == PCM_I16 ? 2 : 4);
    return 0;
}

extern "C" int nnn_mix_apply_pcm_device(nnn_mix *h, const void *d_in, void *d_out, const uint8_t *d_talk, const uint8_t *d_live, int32_t *d_heard,
                                        int n_frames, const nnn_pcm_layout *in_layout, const nnn_pcm_layout *out_layout, void *hip_stream)
{
    if (int rc = mix_call_ok(h, d_in, d_out, n_frames)) return rc;
    if (int rc = mix_layout_ok(h, in_layout, d_in, "input")) return rc;
    if (int rc = mix_layout_ok(h, out_layout, d_out, "output")) return rc;
    if ((uintptr_t)d_heard & 3) return fail("nnn_mix_apply: the heard rows are not aligned to their 4-byte values");
    return mix_enqueue(h, d_in, d_out, d_talk, d_live, d_heard, n_frames, in_layout->format, in_layout->channels, in_layout->group_stride,
                       in_layout->frame_stride, out_layout->format, out_layout->channels, out_layout->group_stride, out_layout->frame_stride, hip_stream);
}

template <class T> static int mix_room(nnn_mix *h, T *&q, size_t &cap, size_t bytes)
{
    if (bytes <= cap) return 0;
    NNN_RT_LOCK;
    if (int rc = mix_drain(h)) return rc;
    HIPCHK(hipFree(q));
    q = nullptr, cap = 0;
    HIPCHK(hipMalloc((void **)&q, bytes));
    cap = bytes;
    return 0;
}

extern "C" int nnn_mix_apply_host(nnn_mix *h, const float *in, float *out, const uint8_t *talk, const uint8_t *live, int32_t *heard, int n_frames)
{
    if (int rc = mix_call_ok(h, in, out, n_frames)) return rc;
    HIPCHK(hipSetDevice(h->device));
    const size_t S = (size_t)h->S, rows = (size_t)n_frames * S, per = (size_t)n_frames * FRAME;
    if (int rc = mix_room(h, h->h_in, h->h_in_cap, rows * FRAME * sizeof(float))) return rc;
    if (int rc = mix_room(h, h->h_out, h->h_out_cap, rows * FRAME * sizeof(float))) return rc;
    if (talk)
        if (int rc = mix_room(h, h->h_talk, h->h_talk_cap, rows)) return rc;
    if (live)
        if (int rc = mix_room(h, h->h_live, h->h_live_cap, S)) return rc;
    if (heard)
        if (int rc = mix_room(h, h->h_heard, h->h_heard_cap, rows * sizeof(int32_t))) return rc;
    hipStream_t st = h->own_stream;
    if (h->have_last && h->last_stream != st) HIPCHK(hipStreamWaitEvent(st, h->ev_last, 0));   // (the staging may be an earlier call's until then)
    HIPCHK(hipMemcpyAsync(h->h_in, in, rows * FRAME * sizeof(float), hipMemcpyHostToDevice, st));
    if (talk) HIPCHK(hipMemcpyAsync(h->h_talk, talk, rows, hipMemcpyHostToDevice, st));
    if (live) HIPCHK(hipMemcpyAsync(h->h_live, live, S, hipMemcpyHostToDevice, st));
    if (int rc = mix_enqueue(h, h->h_in, h->h_out, talk ? h->h_talk : nullptr, live ? h->h_live : nullptr, heard ? h->h_heard : nullptr, n_frames, PCM_F32, 1,
                             per, FRAME, PCM_F32, 1, per, FRAME, st))
        return rc;
    std::vector<int32_t> hd;
    if (!live) {
        HIPCHK(hipMemcpyAsync(out, h->h_out, rows * FRAME * sizeof(float), hipMemcpyDeviceToHost, st));
        if (heard) HIPCHK(hipMemcpyAsync(heard, h->h_heard, rows * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    } else {
        for (size_t s = 0; s < S;) {   // the live streams' rows, a run of neighbours at a time
            if (!live[s]) { s++; continue; }
            size_t e = s;
            while (e < S && live[e]) e++;
            HIPCHK(hipMemcpyAsync(out + s * per, h->h_out + s * per, (e - s) * per * sizeof(float), hipMemcpyDeviceToHost, st));
            s = e;
        }
        if (heard) {
            hd.resize(rows);
            HIPCHK(hipMemcpyAsync(hd.data(), h->h_heard, rows * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        }
    }
    HIPCHK(hipStreamSynchronize(st));
    if (live && heard)
        for (size_t t = 0; t < (size_t)n_frames; t++)
            for (size_t s = 0; s < S; s++)
                if (live[s]) heard[t * S + s] = hd[t * S + s];
    return 0;
}
