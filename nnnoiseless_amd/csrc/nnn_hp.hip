#pragma once
// nnn_hp.hip -- K1, the high-pass stage: k_hp, k_hp2 and everything only they use.  nnn_kernels.hip includes it right after nnn_common.hip;
// it is also the one stage file the library compiles on its own (-DNNN_HP_UNIT, with nnn_common.hip and nothing else), WITH the compiler's
// SLP pairing that the rest of the library is built without (see the note at k_hp2; round 6).
#include "nnn_common.hip"

namespace nnn {

// One lane's next HP_CH samples of its own stream, kept in raw form until the recurrence of the previous HP_CH is done (so
// the loads stay in flight behind it).  VEC: mono stream with 16-byte aligned rows, 16 bytes per load.
// (HP_CH = 16 at 168 registers, tried so that the 64 lone waves of a 4096-stream launch would slip in beside the group's other
// kernels: 20 -> 26 us per frame on its own, 70 -> 90 at 65536 streams, and no gain in the pipelined run.)
#ifndef NNN_HP_CH
#define NNN_HP_CH 32
#endif
constexpr int HP_CH = NNN_HP_CH;
template <int FMT, bool VEC> struct HpChunk {
    static constexpr int NV = FMT == PCM_I16 ? HP_CH / 8 : HP_CH / 4;
    uint4 v[VEC ? NV : 1];
    unsigned w[VEC ? 1 : HP_CH];
    __device__ __forceinline__ void load(const char *p, int sstride)
    {
        if (VEC) {
#pragma unroll
            for (int q = 0; q < NV; q++) v[q] = ld_global_u4(p + 16 * q);
        } else {
#pragma unroll
            for (int j = 0; j < HP_CH; j++)
                w[j] = FMT == PCM_I16 ? (unsigned)(int)ld_global<short>(p + (long long)j * sstride)
                                      : ld_global<unsigned>(p + (long long)j * sstride);
        }
    }
    __device__ __forceinline__ void get(float (&x)[HP_CH]) const
    {
        if (VEC && FMT == PCM_I16) {
#pragma unroll
            for (int q = 0; q < NV; q++) {
                const unsigned u[4] = {v[q].x, v[q].y, v[q].z, v[q].w};
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    x[8 * q + 2 * e] = (float)(short)(u[e] & 0xffffu);
                    x[8 * q + 2 * e + 1] = (float)((int)u[e] >> 16);
                }
            }
        } else if (VEC) {
#pragma unroll
            for (int q = 0; q < NV; q++) {
                x[4 * q] = __uint_as_float(v[q].x); x[4 * q + 1] = __uint_as_float(v[q].y);
                x[4 * q + 2] = __uint_as_float(v[q].z); x[4 * q + 3] = __uint_as_float(v[q].w);
            }
        } else {
#pragma unroll
            for (int j = 0; j < HP_CH; j++) x[j] = FMT == PCM_I16 ? (float)(int)w[j] : __uint_as_float(w[j]);
        }
        if (FMT == PCM_F32_UNIT) {
#pragma unroll
            for (int j = 0; j < HP_CH; j++) x[j] *= 32768.0f;
        }
    }
};

// ---------------------------------------------------------------------------------------------
// K1  hp_filter: high-pass biquad (f64 arithmetic, f32 state) + append to the history ring
//     (ref: src/features.rs:97-104, src/util.rs:95-107), and the 2:1 decimation of pitch_downsample
//     (ref: src/pitch.rs:455-458) done incrementally: decimated sample d = ((s[2d-1] + s[2d+1])/2 + s[2d])/2
//     depends only on absolute samples, so each frame adds 240 values to a persistent ring instead of
//     recomputing all 864; only the reference's special first element is per frame.  The first 960 values of the
//     ring are mirrored behind its end: every frame's 864-value window is then one contiguous run for its reader.
//     lane = stream; the 480-step recurrence is inherently serial per stream and a lone wave is bound by
//     instruction issue, so each lane moves its own stream's samples with 16-byte accesses (a full 128-byte
//     line per 32 samples) instead of transposing tiles through LDS for coalescing.  One launch covers the `g`
//     consecutive frames of a group: the biquad state stays in registers from frame to frame.
// ---------------------------------------------------------------------------------------------
struct HpState { float m0, m1, prev; };

// The history ring is stored in rows: a lane's own 32 results are 128 contiguous bytes of ITS stream, so storing them directly
// makes every store instruction touch 64 cache lines with 16 bytes each -- measured (same box, stores left out) at 5 % of the whole
// pipeline's throughput at 4096 streams, more than the kernel's share of anything.  The results of a chunk therefore cross LDS
// (row stride 33 floats: conflict-free both ways) and leave as 8 stores of 8 streams x 128 contiguous bytes.
constexpr int HP_LD = HP_CH + 1;

// HP_CH steps of the biquad (ref: src/util.rs:95-107, coefficients :68-71): y = x + m0; m0 = f32(m1 + (b0 x - a0 y)); m1 = f32(b1 x - a1 y), in
// f64 with the state rounded to f32 each step.  b0 = -2 and b1 = 1: their products are exact, so b0 x - a0 y is ONE rounding of
// -2 x - fl(a0 y) -- what fma(x, -2, -fl(a0 y)) returns -- and b1 x is x.  Twelve f64 instructions per step on a chain of six.
__device__ __forceinline__ void hp_recurrence(const float (&xs)[HP_CH], float (&ys)[HP_CH], float &m0, float &m1)
{
    const double a0 = (double)-1.99599f, a1 = (double)0.99600f;
#pragma unroll
    for (int j = 0; j < HP_CH; j++) {
        const double x64 = (double)xs[j];
        const double y64 = x64 + (double)m0;
        m0 = (float)((double)m1 + fma(x64, -2.0, -(a0 * y64)));
        m1 = (float)(x64 - a1 * y64);
        ys[j] = (float)y64;
    }
}

// A held stream in a tile that still has live ones runs along on zeros: nothing of the caller's buffer enters its (dead) state.
// MUTE is an instantiation of the high-pass KERNELS (k_hp<true>, k_hp2<.., true>), which the launch plan picks for calls made while some
// stream is held; it also carries the kernels' whole-tile returns.  A batch that holds nothing runs the instructions it ran before there
// was a mask: the recurrence is a serial chain bound by issue, and a one-frame tick is three such latency-bound launches, where even the
// compiled-in presence of a never-taken mask check moved the code enough to measure (1 us of 110).  The kernels of the tick -- these,
// k_pitch and k_back -- therefore take the mask as a template flag (HELD there), the others as a run-time null pointer.
// The filter's state goes to zero with them: the stream's history is exact zeros from its first held chunk on (digital silence, the
// cheapest thing every later kernel knows), not the biquad's tail dying away through ever smaller values -- which keeps the coarse pitch
// search of the stream's whole block off its certified path for as long as it lasts (measured: scattered held streams +10 % per call).
__device__ __forceinline__ void hp_mute(float (&xs)[HP_CH], float &m0, float &m1, bool held)
{
#pragma unroll
    for (int j = 0; j < HP_CH; j++) xs[j] = held ? 0.0f : xs[j];
    m0 = held ? 0.0f : m0;
    m1 = held ? 0.0f : m1;
}

template <int FMT, bool VEC, bool MUTE>
__device__ __forceinline__ void hp_frame(const Buffers &b, const char *sp_in, long long sp_group_stride, int slot, int ch, int tile, int lane, HpState &st, float *Ly,
                                         bool held)
{
    const int elem = pcm_elem_bytes(FMT), sstride = ch * elem;
    const int s = tile * TILE + lane;
    // padding lanes of the last tile re-read the last real stream: their state is never looked at
    const int sc = s < b.S ? s : b.S - 1, grp = sc / ch;
    const char *in = sp_in + (long long)grp * sp_group_stride + (long long)(sc - grp * ch) * elem;
    // (two chunks in flight -- chunk c + 2 requested when chunk c leaves its registers -- was measured in round 4 for the lone waves of a
    // one-frame call: 378 registers, the launch 27 -> 34 us.  One chunk ahead it stays.)
    HpChunk<FMT, VEC> nxt;
    nxt.load(in, sstride);
    float m0 = st.m0, m1 = st.m1, prev = st.prev;
    NNN_STAMP(b, 24);
    const int nslot = b.nslot, hstr = hist_stride(nslot);
    float *ring = NNN_TI(b.dec, dec_len(nslot), tile, lane);
    float *h = b.hist + (size_t)s * hstr;
    {   // x_lp[0] = (x[1] / 2 + x[0]) / 2 on the oldest two samples of this frame's 1728-sample history: kept beside
        // the ring, per slot (the ring position it replaces is still a regular value for the previous frame)
        const int rb = ring_base(slot, nslot);
        const float x0 = h[rb], x1 = h[rb + 1];   // (rb + 1 = the ring's length reads the copy of sample 0 kept there)
        NNN_TI(b.xlp0, nslot, tile, lane)[(size_t)slot * TILE] = (x1 / 2.0f + x0) / 2.0f;
    }
    float *dec = ring + (size_t)(240 * slot) * TILE;
    const bool mirror = slot < DEC_MIRROR;
    float4 *hw = (float4 *)(h + slot * FRAME);   // the stride * 4 and FRAME * 4 are multiples of 16
    // Software pipeline over HP_CH-sample chunks.  Loads and stores share one in-order counter (vmcnt), so waiting for
    // chunk c's samples also waits for every store issued before: the stores of chunk c - 1 are therefore issued right
    // after that wait, and both they and the loads of chunk c + 1 travel behind the ~0.7 us recurrence of chunk c.
    float ys[HP_CH], dvs[HP_CH / 2];
    for (int c = 0; c <= FRAME / HP_CH; c++) {
        float xs[HP_CH];
        if (c < FRAME / HP_CH) {
            nxt.get(xs);
            if (MUTE) hp_mute(xs, m0, m1, held);
        }
        if (c > 0) {
#pragma unroll
            for (int t = 0; t < HP_CH / 2; t++) dec[(size_t)(HP_CH / 2 * (c - 1) + t) * TILE] = dvs[t];
            if (mirror) {
#pragma unroll
                for (int t = 0; t < HP_CH / 2; t++) dec[(size_t)(dec_ring_len(nslot) + HP_CH / 2 * (c - 1) + t) * TILE] = dvs[t];
            }
            if (HP_CH == 32) {
                wave_lds_sync();   // (the previous chunk's rows have been read)
#pragma unroll
                for (int j = 0; j < HP_CH; j++) Ly[lane * HP_LD + j] = ys[j];
                wave_lds_sync();
#pragma unroll
                for (int it = 0; it < 8; it++) {
                    const int r = 8 * it + (lane >> 3);
                    const float *y = Ly + r * HP_LD + 4 * (lane & 7);
                    float4 *hr = (float4 *)(b.hist + (size_t)(tile * TILE + r) * hstr + slot * FRAME + (c - 1) * HP_CH) + (lane & 7);
                    *hr = make_float4(y[0], y[1], y[2], y[3]);
                }
            } else {
#pragma unroll
                for (int q = 0; q < HP_CH / 4; q++) hw[HP_CH / 4 * (c - 1) + q] = make_float4(ys[4 * q], ys[4 * q + 1], ys[4 * q + 2], ys[4 * q + 3]);
            }
            if (slot == 0 && c == 1) h[ring_len(nslot)] = ys[0];   // the ring's first sample again behind its end (8-byte reads across the wrap)
        }
        if (c == FRAME / HP_CH) break;
        if (c + 1 < FRAME / HP_CH) nxt.load(in + (long long)(c + 1) * HP_CH * sstride, sstride);
        hp_recurrence(xs, ys, m0, m1);
#pragma unroll
        for (int t = 0; t < HP_CH / 2; t++) {
            const float a = t == 0 ? prev : ys[2 * t - 1], m = ys[2 * t], n = ys[2 * t + 1];
            dvs[t] = ((a + n) / 2.0f + m) / 2.0f;
        }
        prev = ys[HP_CH - 1];
    }
    st.m0 = m0; st.m1 = m1; st.prev = prev;
    NNN_STAMP(b, 25);
}

// `fill` > 0: this launch is the first of a call of `fill` frames whose table nobody has filled -- a launch of its own for that costs
// a one-frame call 6 of its 150 us -- so block 0 writes it (for the kernels behind this one, which start when this one is done) and
// every block takes its own frames' entries from the call's parameters `v0`; the group's first frame is entry `t0` of the call.
template <int FMT, bool VEC, bool MUTE>
__device__ __forceinline__ void hp_group(const Buffers &b, const StepParams *sp, int g, int tile, int lane, float *Ly, const StepParams &v0, int fill)
{
    float *hp = NNN_TI(b.hp_mem, 2, tile, lane);
    float *hl = NNN_TI(b.hp_last, 1, tile, lane);
    HpState st{hp[0], hp[TILE], hl[0]};
    const bool held = MUTE && !live_stream(b, tile, lane);
    for (int f = 0; f < g; f++) {
        // (what a frame needs of its table entry: where its input starts and which ring slot takes it)
        const char *in = fill > 0 ? v0.in + (long long)f * v0.frame_stride : sp[f].in;
        const int slot = fill > 0 ? (v0.slot + f) % b.nslot : sp[f].slot;
        hp_frame<FMT, VEC, MUTE>(b, in, fill > 0 ? v0.group_stride : sp[f].group_stride, slot, fill > 0 ? v0.channels : sp[f].channels, tile, lane, st, Ly, held);
    }
    hp[0] = st.m0;
    hp[TILE] = st.m1;
    hl[0] = st.prev;
}

// The first 16 LPC_HEAD_BLK steps of lag K's sum -- i + K < 624: rows older than the frame being filtered -- for k_hp2's head waves
// (lane = stream on the tile-interleaved ring, like k_lpc); k_pitch's pk_autocorr carries on from there in the same order.
constexpr int LPC_HEAD_BLK = 38;
static_assert(16 * LPC_HEAD_BLK + 4 <= XLP - 240, "");
template <int K>
__device__ __forceinline__ float lpc_head_chain(const float *base, float x0)
{
    constexpr int CH = 16;
    float cur[CH + 4], nxt[CH];
#pragma unroll
    for (int i = 0; i < CH + 4; i++) cur[i] = base[(size_t)i * TILE];
    cur[0] = x0;
    float c = 0.0f;
#pragma nounroll
    for (int ch = 0; ch < LPC_HEAD_BLK; ch++) {
        const float *nb = base + (size_t)((ch + 1 < LPC_HEAD_BLK ? ch + 1 : ch) * CH + 4) * TILE;
#pragma unroll
        for (int i = 0; i < CH; i++) nxt[i] = nb[(size_t)i * TILE];
#pragma unroll
        for (int j = 0; j < CH; j++) c += cur[j] * cur[j + K];
#pragma unroll
        for (int i = 0; i < 4; i++) cur[i] = cur[CH + i];
#pragma unroll
        for (int i = 0; i < CH; i++) cur[4 + i] = nxt[i];
    }
    return c;
}

// The same frame on TWO waves (k_hp2, launches that leave most of the GPU empty: a one-frame call of 4096 streams is 64 lone waves).  The
// recurrence issues 12 f64 instructions per step whatever else the wave does, and everything else -- the results' trip through LDS, 40
// stores per chunk, the decimation -- used to stand between one chunk's recurrence and the next (0.5 of every 1.3 us).  Here wave 0
// runs loads and recurrence only and leaves each chunk's results in one of two LDS buffers; wave 1 (another SIMD) takes them from there
// behind one block barrier per chunk and does the rest while wave 0 is a chunk further.  Same arithmetic, same bits.
template <int FMT, bool VEC, bool MUTE>
__device__ __forceinline__ void hp_chain_frame(const Buffers &b, const char *sp_in, long long sp_group_stride, int ch, int tile, int lane, float &m0, float &m1, float *Ly2, int &k,
                                               bool held)
{
    const int elem = pcm_elem_bytes(FMT), sstride = ch * elem;
    const int s = tile * TILE + lane;
    const int sc = s < b.S ? s : b.S - 1, grp = sc / ch;
    const char *in = sp_in + (long long)grp * sp_group_stride + (long long)(sc - grp * ch) * elem;
    HpChunk<FMT, VEC> nxt;
    nxt.load(in, sstride);
    for (int c = 0; c < FRAME / HP_CH; c++, k++) {
        float xs[HP_CH], ys[HP_CH];
        nxt.get(xs);
        if (MUTE) hp_mute(xs, m0, m1, held);
        if (c + 1 < FRAME / HP_CH) nxt.load(in + (long long)(c + 1) * HP_CH * sstride, sstride);
        hp_recurrence(xs, ys, m0, m1);
        float *L = Ly2 + (k & 1) * (TILE * HP_LD) + lane * HP_LD;
#pragma unroll
        for (int j = 0; j < HP_CH; j++) L[j] = ys[j];
        __syncthreads();   // chunk k is in its buffer (and wave 1 is done with chunk k - 1: this buffer's turn again at k + 2)
    }
}
__device__ __forceinline__ void hp_store_frame(const Buffers &b, int slot, int tile, int lane, float &prev, const float *Ly2, int &k)
{
    const int s = tile * TILE + lane;
    const int nslot = b.nslot, hstr = hist_stride(nslot);
    float *ring = NNN_TI(b.dec, dec_len(nslot), tile, lane);
    float *h = b.hist + (size_t)s * hstr;
    {   // x_lp[0], as in hp_frame
        const int rb = ring_base(slot, nslot);
        const float x0 = h[rb], x1 = h[rb + 1];
        NNN_TI(b.xlp0, nslot, tile, lane)[(size_t)slot * TILE] = (x1 / 2.0f + x0) / 2.0f;
    }
    float *dec = ring + (size_t)(240 * slot) * TILE;
    const bool mirror = slot < DEC_MIRROR;
    for (int c = 0; c < FRAME / HP_CH; c++, k++) {
        __syncthreads();
        const float *L = Ly2 + (k & 1) * (TILE * HP_LD);
#pragma unroll
        for (int it = 0; it < 8; it++) {
            const int r = 8 * it + (lane >> 3);
            const float *y = L + r * HP_LD + 4 * (lane & 7);
            float4 *hr = (float4 *)(b.hist + (size_t)(tile * TILE + r) * hstr + slot * FRAME + c * HP_CH) + (lane & 7);
            *hr = make_float4(y[0], y[1], y[2], y[3]);
        }
        float ys[HP_CH];
#pragma unroll
        for (int j = 0; j < HP_CH; j++) ys[j] = L[lane * HP_LD + j];
#pragma unroll
        for (int t = 0; t < HP_CH / 2; t++) {
            const float a = t == 0 ? prev : ys[2 * t - 1], m = ys[2 * t], n = ys[2 * t + 1];
            const float dv = ((a + n) / 2.0f + m) / 2.0f;
            dec[(size_t)(HP_CH / 2 * c + t) * TILE] = dv;
            if (mirror) dec[(size_t)(dec_ring_len(nslot) + HP_CH / 2 * c + t) * TILE] = dv;
        }
        prev = ys[HP_CH - 1];
        if (slot == 0 && c == 0) h[ring_len(nslot)] = ys[0];
    }
}
template <int FMT, bool VEC, bool MUTE>
__device__ __forceinline__ void hp_chain_group(const Buffers &b, const StepParams *sp, int g, int tile, int lane, float *Ly2, const StepParams &v0, int fill)
{
    float *hp = NNN_TI(b.hp_mem, 2, tile, lane);
    float m0 = hp[0], m1 = hp[TILE];
    int k = 0;
    const bool held = MUTE && !live_stream(b, tile, lane);
    for (int f = 0; f < g; f++) {
        const char *in = fill > 0 ? v0.in + (long long)f * v0.frame_stride : sp[f].in;
        hp_chain_frame<FMT, VEC, MUTE>(b, in, fill > 0 ? v0.group_stride : sp[f].group_stride, fill > 0 ? v0.channels : sp[f].channels, tile, lane, m0, m1, Ly2, k, held);
    }
    hp[0] = m0;
    hp[TILE] = m1;
}
// `head` (a one-frame launch whose LPC analysis runs inside k_pitch): blocks NT .. are not the high-pass at all -- each of their waves takes
// one (tile, lag) of the five autocorrelation sums through the rows of the frame's window that are older than the frame (608 of the 860
// steps: they end before the first decimated value this launch produces), while the recurrence above runs its 20 us; k_pitch then
// starts every sum there instead of at zero: 11 -> 3.5 us of its critical path.
// TPB tiles per block (waves 0 .. TPB - 1 the recurrences, waves TPB .. the helpers; TPB <= 2: every wave a SIMD of its own -- with four
// tiles a helper shares the SIMD of a recurrence and the kernel takes twice as long).  Groups run two tiles per block: half as many
// compute units carry a wave that takes most of its SIMD's issue slots from the pipelined call's other kernels (4096 x 48 +1 %, 8192 x 48
// +2 %; keeping k_pitch's blocks off those units altogether by padding the block's LDS: measured, no gain).
// The two high-pass kernels are compiled in a translation unit of their own (nnn_hp.hip) WITH the compiler's SLP pairing, the rest of the
// library without it (round 6): the recurrence is one wave's serial chain of f64 instructions, bound by that wave's own issue rate, and
// where the loads, address arithmetic and stores land between the chain's instructions decides its pace -- with the pairing pass on the
// same source is 14 % faster per frame on small launches (k_hp2 21.5 against 25.0 us per frame at 4096 streams, 26 against 29 us in a
// one-frame tick), while k_pitch, the transforms and the synthesis are 2-5 % faster without it.  Same instructions on the same values either
// way.  NNN_HP_EXTERN: this unit only declares them; NNN_HP_UNIT: this unit is nnn_hp.hip on its own and emits them.  A build that
// defines neither (the tests' interpreter, scripts/build_variant.sh, the stamp builds) holds everything in one unit, as before.
// the instantiations the library launches, written once: declared (NNN_HP_EXTERN) or emitted (NNN_HP_UNIT) with the same list
#define NNN_HP_INSTANCES(DECL)                                                                                            \
    DECL void k_hp2<1, false>(Buffers b, const StepParams *sp, int g, StepParams v0, int fill, int head);                 \
    DECL void k_hp2<2, false>(Buffers b, const StepParams *sp, int g, StepParams v0, int fill, int head);                 \
    DECL void k_hp2<1, true>(Buffers b, const StepParams *sp, int g, StepParams v0, int fill, int head);                  \
    DECL void k_hp2<2, true>(Buffers b, const StepParams *sp, int g, StepParams v0, int fill, int head);                  \
    DECL void k_hp<false>(Buffers b, const StepParams *sp, int g, StepParams v0, int fill);                               \
    DECL void k_hp<true>(Buffers b, const StepParams *sp, int g, StepParams v0, int fill);
#ifdef NNN_HP_EXTERN
template <int TPB, bool MUTE> __global__ void k_hp2(Buffers b, const StepParams *sp, int g, StepParams v0, int fill, int head);
template <bool MUTE> __global__ void k_hp(Buffers b, const StepParams *sp, int g, StepParams v0, int fill);
NNN_HP_INSTANCES(extern template __global__)
#else
template <int TPB, bool MUTE>
__global__ void __launch_bounds__(128 * TPB) k_hp2(Buffers b, const StepParams *sp, int g, StepParams v0, int fill, int head)
{
    static_assert(HP_CH == 32, "");
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int role = wave / TPB, nblk = (b.NT + TPB - 1) / TPB;
    if ((int)blockIdx.x >= nblk) {
        const int item = 2 * TPB * ((int)blockIdx.x - nblk) + wave;
        if (!head || item >= 5 * b.NT) return;
        const int tile = item / 5, lag = item - 5 * tile, nslot = b.nslot;
        if (MUTE && live_word(b, tile) == 0ull) return;   // (every stream of the tile held: its pitch blocks, which would take these sums, return too)
        const int slot = fill > 0 ? v0.slot : sp->slot;
        const float *h = b.hist + (size_t)(tile * TILE + lane) * hist_stride(nslot);
        const int rb = ring_base(slot, nslot);
        const float x0 = (h[rb + 1] / 2.0f + h[rb]) / 2.0f;   // x_lp[0] is special (ref: src/pitch.rs:458); see hp_frame
        const float *base = b.dec + ((size_t)tile * dec_len(nslot) + (size_t)dec_base(slot, nslot)) * TILE + lane;
        float c;
        if (lag == 0) c = lpc_head_chain<0>(base, x0);
        else if (lag == 1) c = lpc_head_chain<1>(base, x0);
        else if (lag == 2) c = lpc_head_chain<2>(base, x0);
        else if (lag == 3) c = lpc_head_chain<3>(base, x0);
        else c = lpc_head_chain<4>(base, x0);
        b.lpc_head[(size_t)item * TILE + lane] = c;
        return;
    }
    const int tile = (int)blockIdx.x * TPB + (wave - role * TPB);
    __shared__ float Ly2s[TPB][2 * TILE * HP_LD];
    float *Ly2 = Ly2s[wave - role * TPB];
    // (the parameter table is tile 0's to fill whether or not its streams take part)
    if (role == 1 && fill > 0 && tile == 0)
        for (int t = lane; t < fill; t += 64) ((StepParams *)sp)[t] = step_params_at(v0, t, b.nslot);
    if (MUTE) {   // a block none of whose tiles has a live stream (nnn_batch_hold_streams) returns at once
        bool any = false;
#pragma unroll
        for (int u = 0; u < TPB; u++) {
            const int tu = (int)blockIdx.x * TPB + u;
            any = any || (tu < b.NT && live_word(b, tu) != 0ull);
        }
        if (!any) return;
    }
    if (tile >= b.NT || (MUTE && live_word(b, tile) == 0ull)) {   // (a ragged last block, a held tile beside a live one: the spare waves only keep the barrier count)
        for (int i = 0; i < g * (FRAME / HP_CH); i++) __syncthreads();
        return;
    }
    if (role == 1) {
        float *hl = NNN_TI(b.hp_last, 1, tile, lane);
        float prev = hl[0];
        int k = 0;
        for (int f = 0; f < g; f++) hp_store_frame(b, fill > 0 ? (v0.slot + f) % b.nslot : sp[f].slot, tile, lane, prev, Ly2, k);
        hl[0] = prev;
        return;
    }
    const int fmt = fill > 0 ? v0.fmt : sp->fmt;
    wf_setprio_high();
    const StepParams &lay = fill > 0 ? v0 : *sp;
    const bool vec = lay.channels == 1 && ((((size_t)lay.in) | (size_t)lay.group_stride | (size_t)lay.frame_stride) & 15) == 0;
    if (fmt == PCM_F32) { if (vec) hp_chain_group<PCM_F32, true, MUTE>(b, sp, g, tile, lane, Ly2, v0, fill); else hp_chain_group<PCM_F32, false, MUTE>(b, sp, g, tile, lane, Ly2, v0, fill); }
    else if (fmt == PCM_I16) { if (vec) hp_chain_group<PCM_I16, true, MUTE>(b, sp, g, tile, lane, Ly2, v0, fill); else hp_chain_group<PCM_I16, false, MUTE>(b, sp, g, tile, lane, Ly2, v0, fill); }
    else { if (vec) hp_chain_group<PCM_F32_UNIT, true, MUTE>(b, sp, g, tile, lane, Ly2, v0, fill); else hp_chain_group<PCM_F32_UNIT, false, MUTE>(b, sp, g, tile, lane, Ly2, v0, fill); }
}

template <bool MUTE>
__global__ void __launch_bounds__(64, HP_CH <= 16 ? 3 : 1) k_hp(Buffers b, const StepParams *sp, int g, StepParams v0, int fill)
{
    const int lane = threadIdx.x, tile = blockIdx.x;
    if (fill > 0 && tile == 0)
        for (int t = lane; t < fill; t += 64) ((StepParams *)sp)[t] = step_params_at(v0, t, b.nslot);
    if (MUTE && live_word(b, tile) == 0ull) return;   // (every stream of the tile held, nnn_batch_hold_streams)
    const int fmt = fill > 0 ? v0.fmt : sp->fmt;
    wf_setprio_high();   // a lone wave on a serial chain that shares its SIMD with another kernel's wave (+1 % at 4096 streams)
    const StepParams &lay = fill > 0 ? v0 : *sp;
    const bool vec = lay.channels == 1 && ((((size_t)lay.in) | (size_t)lay.group_stride | (size_t)lay.frame_stride) & 15) == 0;
    __shared__ float Ly[TILE * HP_LD];
    if (fmt == PCM_F32) { if (vec) hp_group<PCM_F32, true, MUTE>(b, sp, g, tile, lane, Ly, v0, fill); else hp_group<PCM_F32, false, MUTE>(b, sp, g, tile, lane, Ly, v0, fill); }
    else if (fmt == PCM_I16) { if (vec) hp_group<PCM_I16, true, MUTE>(b, sp, g, tile, lane, Ly, v0, fill); else hp_group<PCM_I16, false, MUTE>(b, sp, g, tile, lane, Ly, v0, fill); }
    else { if (vec) hp_group<PCM_F32_UNIT, true, MUTE>(b, sp, g, tile, lane, Ly, v0, fill); else hp_group<PCM_F32_UNIT, false, MUTE>(b, sp, g, tile, lane, Ly, v0, fill); }
}

#ifdef NNN_HP_UNIT
NNN_HP_INSTANCES(template __global__)
#endif
#endif   // NNN_HP_EXTERN

}  // namespace nnn
