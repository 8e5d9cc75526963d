#pragma once
// nnn_rnn_wf.hip -- K10w, the layer-pipelined RNN: k_rnn_wf, its LDS layout (wf_lds) and everything only it uses.  Not a translation unit:
// nnn_kernels.hip includes it between k_rnn (nnn_rnn.hip, whose GEMM and shared layer pieces it uses) and the synthesis.

namespace nnn {

// ---------------------------------------------------------------------------------------------
// K10w rnn, layer-pipelined ("wavefront"): the same computation as k_rnn for models of the built-in shape class (at most 2 / 2 /
//     3 / 6 neuron blocks of 16 in the input dense, vad, noise and denoise layers), 16 stream rows per block, 12 waves.
//     The chain of a frame -- dense, three GRUs of two phases each, output dense -- is eleven dependent phases of ~1-2 us of
//     mostly latency; here the layers of DIFFERENT frames run side by side, each on its own waves: in tick t the vad GRU works
//     on frame t, the noise GRU on frame t - 1, the denoise GRU on frame t - 2, the output layer on frame t - 3, the input
//     dense and the feature stage on frame t + 1, and a tick is two phases (everybody's first GEMM phase; everybody's second).
//     A group of g frames takes g + 4 ticks instead of 11 g phases.
//     Every layer reads its inputs from its own LDS matrix, written by its producers one to three ticks earlier into the
//     slot of that frame (noise: 2 slots, denoise: 3), so nothing is overwritten before its last reader has passed; all
//     matrices use the column coordinates of the packed weights (k_rnn's single input matrix), each holding the window its
//     layer reads.  Roles (every phase of every layer is a latency chain, so no wave carries two of the long ones): waves 0..5
//     denoise neuron block w, the first two also an input dense unit each in the second phase (their shortest); waves 6..8
//     noise block w - 6 and, between them, the feature fan-out; waves 9, 10 vad block w - 9 plus an output dense unit each;
//     wave 11 the feature stage (lane = (row, part)) and the vad output.  Measured per tick at 65 536 streams
//     (scripts/gpu_stamps_rnn.sh): first phase 3.7-3.9 us on every role, second 1.5-2.6 us (round 2a: 5.8 + 3.4, both set by
//     the features wave and the vad waves, which then also carried the input dense layer and the fan-out).
// ---------------------------------------------------------------------------------------------
constexpr int WF_ROWS = 16, WF_WAVES = 12, WF_FS_W = 72;   // feature staging: the input dense layer's two k-steps wide + 8

struct WfGru {   // what a GRU unit keeps from its first phase to its second
    f32x4 acc[3][2];
    float zz[4], sold[4];
};
// The recurrent weight fragments of a wave's GRU unit (and its biases) stay in its registers for the whole launch; the input
// fragments -- too many to keep beside them at three waves per SIMD -- are requested at the head of the first phase and
// travel behind the recurrent GEMM.  Recurrent GEMMs of the shape class have <= 3 k-steps.
constexpr int WF_KS_REC = 3;
struct WfWeights {
    Frags<2, WF_KS_REC> zr;
    Frags<1, WF_KS_REC> h;
    float bias[3];
};
__device__ __forceinline__ void wf_load_weights(WfWeights &w, const LayerDesc &L, const uint4 *__restrict__ Wq, const float *__restrict__ fpar,
                                                int nbi, int lane)
{
    const uint4 *Brec = Wq + L.rec.wofs + (size_t)nbi * 3 * L.rec.ksteps * 64;
    load_frags<2, 0, WF_KS_REC>(w.zr, L.rec, Brec, lane);
    load_frags<1, 2, WF_KS_REC>(w.h, L.rec, Brec, lane);
    const int neuron = nbi * 16 + (lane & 15);
#pragma unroll
    for (int g = 0; g < 3; g++) w.bias[g] = neuron < L.n ? fpar[L.bias + g * L.n + neuron] : 0.0f;
}

// first phase of GRU layer L for neuron block nbi: z, r, input part of the candidate; r * state -> RS (ref: src/rnn.rs:292-318)
__device__ __forceinline__ void wf_gru_a(const LayerDesc &L, const unsigned short *Ain, int in_w, const unsigned short *SP, unsigned short *RS,
                                         int sw, const uint4 *__restrict__ Wq, const WfWeights &w, const float *tab, int nbi, int lane, WfGru &u)
{
    const float scale = 1.0f / 256.0f;
    const int neuron = nbi * 16 + (lane & 15);
    const bool nvalid = neuron < L.n;
    const uint4 *Bin = Wq + L.in.wofs + (size_t)nbi * 3 * L.in.ksteps * 64;
    const uint4 *Brec = Wq + L.rec.wofs + (size_t)nbi * 3 * L.rec.ksteps * 64;
    Frags<3> f_in;
    load_frags<3, 0>(f_in, L.in, Bin, lane);
#pragma unroll
    for (int g = 0; g < 3; g++) u.acc[g][0] = f32x4{w.bias[g], w.bias[g], w.bias[g], w.bias[g]};
    const int ps = WF_ROWS * sw;
    gemm_acc<2, 1, 0, WF_KS_REC>(u.acc, SP, ps, sw, 0, L.rec, Brec, lane, w.zr);
    gemm_acc<3, 1, 0>(u.acc, Ain, WF_ROWS * in_w, in_w, 0, L.in, Bin, lane, f_in);
    const int kcols = 32 * L.rec.ksteps;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int row = 4 * (lane >> 4) + q;
        const float so = nvalid ? load_split(SP, ps, row * sw + neuron) : 0.0f;   // the three planes hold the state exactly
        u.sold[q] = so;
        u.zz[q] = sigmoid_approx(scale * u.acc[0][0][q], tab);
        const float rs = so * sigmoid_approx(scale * u.acc[1][0][q], tab);
        if (neuron < kcols) store_split(RS, ps, row * sw + neuron, rs);
        if (nbi == L.nb - 1 && neuron + 16 < kcols) store_split(RS, ps, row * sw + neuron + 16, 0.0f);
    }
}

// second phase: recurrent part of the candidate on r * state, state update (ref: src/rnn.rs:319-326); sink(row, neuron, new state)
template <class Sink>
__device__ __forceinline__ void wf_gru_b(const LayerDesc &L, const unsigned short *RS, int sw, const uint4 *__restrict__ Wq, const WfWeights &w,
                                         const float *tab, const int *live, int nbi, int lane, WfGru &u, Sink &&sink)
{
    const float scale = 1.0f / 256.0f;
    const int neuron = nbi * 16 + (lane & 15);
    const uint4 *Brec = Wq + L.rec.wofs + (size_t)nbi * 3 * L.rec.ksteps * 64;
    gemm_acc<1, 1, 2, WF_KS_REC>(u.acc, RS, WF_ROWS * sw, sw, 0, L.rec, Brec, lane, w.h);
    if (neuron < L.n) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int row = 4 * (lane >> 4) + q;
            const float hh = activate(L.act, scale * u.acc[2][0][q], tab);
            const float z = u.zz[q], so = u.sold[q];
            float snew = z * so + (1.0f - z) * hh;
            snew = live[row] ? snew : so;   // silent frames leave the state alone (ref: src/denoise.rs:100)
            sink(row, neuron, snew);
        }
    }
}

// The feature stage of one frame on all 64 lanes of the features wave: lane = (row, part), row = lane & 15, part = lane >> 4.
// Same arithmetic as features_row (which one lane per row runs start to finish); the four parts of a row share the new
// cepstrum through LDS (`cnb`), split the 7 pair distances the new ring row takes part in and the 42 outputs.  The frame's
// inputs (written by k_fft_xp / k_pitch2, in HBM) are requested a tick ahead: WfFeatIn.
// (they live in the registers of the features wave's otherwise unused weight set: one register allocation serves all roles)
struct WfFeatIn {
    float mine[7];
    int pitch, silent;
};
__device__ __forceinline__ void wf_features_load(WfWeights &w, const Buffers &b, int f, int tile, int r0, int lane)
{
    const int row = lane & 15, part = lane >> 4, trow = r0 + row;
    const float *cg = NNN_TIF(b, cn, 28, f, tile, trow);
    unsigned m[7];
#pragma unroll
    for (int i = 0; i < 7; i++) m[i] = __float_as_uint(cg[(size_t)(7 * part + i) * TILE]);
    w.zr.f[0][0] = make_uint4(m[0], m[1], m[2], m[3]);
    w.zr.f[0][1] = make_uint4(m[4], m[5], m[6], (unsigned)NNN_TIF(b, pitch, 1, f, tile, trow)[0]);
    w.h.f[0][0].x = (unsigned)NNN_TIF(b, silence, 1, f, tile, trow)[0];
}
__device__ __forceinline__ WfFeatIn wf_features_in(const WfWeights &w)
{
    WfFeatIn in;
    const uint4 a = w.zr.f[0][0], c = w.zr.f[0][1];
    in.mine[0] = __uint_as_float(a.x); in.mine[1] = __uint_as_float(a.y); in.mine[2] = __uint_as_float(a.z); in.mine[3] = __uint_as_float(a.w);
    in.mine[4] = __uint_as_float(c.x); in.mine[5] = __uint_as_float(c.y); in.mine[6] = __uint_as_float(c.z);
    in.pitch = (int)c.w;
    in.silent = (int)w.h.f[0][0].x;
    return in;
}
// outputs kb + part of the feature stage, all of one kind (compile-time, so every address below is a base + a constant):
// KIND 0: ceps + ring[-1] + ring[-2]; 1: the value itself; 2: ceps - ring[-2]; 3: ceps - 2 ring[-1] + ring[-2] -- each as
// (v0 + a) + c with features_row's a and c, zeros included.  src_b / rb: first input of the kind / first ring band, for part 0.
template <int KIND, int KB, int SRC_B, int RB, bool HALF>
__device__ __forceinline__ void wf_feature_outputs(const Buffers &b, int f, int tile, int trow, int part, bool silent, const float *cnb_l,
                                                   const float *r1_l, const float *r2_l, unsigned short *fs_l)
{
    constexpr int rm = WF_ROWS;
    if (HALF && part >= 2) return;   // (the kind's last two outputs)
    const float v0 = cnb_l[SRC_B * rm];
    const float v1 = (KIND == 0 || KIND == 3) ? r1_l[RB * rm] : 0.0f;
    const float v2 = (KIND == 0 || KIND == 2 || KIND == 3) ? r2_l[RB * rm] : 0.0f;
    const float a = KIND == 0 ? v1 : (KIND == 3 ? -(2.0f * v1) : 0.0f);
    const float c = (KIND == 0 || KIND == 3) ? v2 : (KIND == 2 ? -v2 : 0.0f);
    float v = (v0 + a) + c;
    v = silent ? 0.0f : v;
    if (b.taps) NNN_TIF(b, feat, NFEAT, f, tile, trow)[(size_t)(KB + part) * TILE] = v;
    store_split(fs_l, rm * WF_FS_W, KB, v);
}

__device__ __forceinline__ void wf_features(const Buffers &b, const WfFeatIn &in, int f, int tile, int r0, int lane, float *crs, float *dc,
                                            float *cnb, unsigned short *FS, int *live_f, int &mem_id)
{
    constexpr int rm = WF_ROWS;
    const int row = lane & 15, part = lane >> 4, trow = r0 + row;
    const int pitch = in.pitch;
    const bool silent = in.silent != 0;
    NNN_STAMPW(b, 8, f == 3);
#pragma unroll
    for (int i = 0; i < 7; i++) cnb[(7 * part + i) * rm + row] = in.mine[i];
    wave_lds_sync();
    if (part == 0) live_f[row] = silent ? 0 : 1;
    const int c0 = mem_id, c1 = mem_id < 1 ? CEPS_MEM + mem_id - 1 : mem_id - 1;
    const int c2 = mem_id < 2 ? CEPS_MEM + mem_id - 2 : mem_id - 2;
    NNN_STAMPW(b, 9, f == 3);
    if (!silent) {   // "if there's no audio, avoid messing up the state" (ref: src/features.rs:160-166)
        float *cm = NNN_TI(b.ceps_mem, CEPS_MEM * NB, tile, trow);
        for (int k = part; k < NB; k += 4) {
            const float v = cnb[k * rm + row];
            cm[(size_t)(c0 * NB + k) * TILE] = v;
            crs[(c0 * NB + k) * rm + row] = v;
        }
        mem_id = mem_id + 1 == CEPS_MEM ? 0 : mem_id + 1;
        NNN_STAMPW(b, 10, f == 3);
        // the 7 distances the new row takes part in, each summed over the 22 bands in order (ref: src/features.rs:203-208);
        // they read the new row from cnb and the others from the ring (rows j != c0 are not being written).  A lane takes
        // partners part and part + 4 together (the fourth part's second one is a shadow of its first, not stored): one read of
        // the new row serves both sums and the two chains hide each other's latency.
        const int ia = part, ib = part + 4 < CEPS_MEM - 1 ? part + 4 : part;
        const int ja = ia < c0 ? ia : ia + 1, jb = ib < c0 ? ib : ib + 1;
        const float *ra = crs + (ja * NB) * rm + row, *rb = crs + (jb * NB) * rm + row, *nw = cnb + row;
        float da = 0.0f, db = 0.0f;
#pragma unroll
        for (int k = 0; k < NB; k++) {
            const float x = nw[k * rm];
            const float ea = x - ra[k * rm], eb = x - rb[k * rm];
            da += ea * ea;
            db += eb * eb;
        }
        dc[pair_index(ja < c0 ? ja : c0, ja < c0 ? c0 : ja) * rm + row] = da;
        if (part + 4 < CEPS_MEM - 1) dc[pair_index(jb < c0 ? jb : c0, jb < c0 ? c0 : jb) * rm + row] = db;
    }
    NNN_STAMPW(b, 11, f == 3);
    wave_lds_sync();
    // outputs 0..39, four at a time (one per part) and one kind at a time: the operations of features_row in its order on the
    // new cepstrum and the two ring rows before it
    {
        const float *cnb_l = cnb + part * rm + row;
        const float *r1_l = crs + (c1 * NB + part) * rm + row, *r2_l = crs + (c2 * NB + part) * rm + row;
        unsigned short *fs_l = FS + row * WF_FS_W + part;
        wf_feature_outputs<0, 0, 0, 0, false>(b, f, tile, trow, part, silent, cnb_l, r1_l, r2_l, fs_l);
        wf_feature_outputs<0, 4, 4, 4, true>(b, f, tile, trow, part, silent, cnb_l, r1_l, r2_l, fs_l);
        wf_feature_outputs<1, 6, 6, 0, false>(b, f, tile, trow, part, silent, cnb_l, r1_l, r2_l, fs_l);
        wf_feature_outputs<1, 10, 10, 0, false>(b, f, tile, trow, part, silent, cnb_l, r1_l, r2_l, fs_l);
        wf_feature_outputs<1, 14, 14, 0, false>(b, f, tile, trow, part, silent, cnb_l, r1_l, r2_l, fs_l);
        wf_feature_outputs<1, 18, 18, 0, false>(b, f, tile, trow, part, silent, cnb_l, r1_l, r2_l, fs_l);
        wf_feature_outputs<2, NB, 0, 0, false>(b, f, tile, trow, part, silent, cnb_l, r1_l, r2_l, fs_l);
        wf_feature_outputs<2, NB + 4, 4, 4, true>(b, f, tile, trow, part, silent, cnb_l, r1_l, r2_l, fs_l);
        wf_feature_outputs<3, NB + 6, 0, 0, false>(b, f, tile, trow, part, silent, cnb_l, r1_l, r2_l, fs_l);
        wf_feature_outputs<3, NB + 10, 4, 4, true>(b, f, tile, trow, part, silent, cnb_l, r1_l, r2_l, fs_l);
        wf_feature_outputs<1, NB + 12, NB, 0, false>(b, f, tile, trow, part, silent, cnb_l, r1_l, r2_l, fs_l);       // cn[22 + ..]: the correlation DCT
        wf_feature_outputs<1, NB + 16, NB + 4, 0, true>(b, f, tile, trow, part, silent, cnb_l, r1_l, r2_l, fs_l);
    }
    NNN_STAMPW(b, 12, f == 3);
    if (part < 2) {   // k = 40 (pitch) on part 0, k = 41 (spectral variability) on part 1
        float v = part == 0 ? 0.01f * ((float)pitch - 300.0f) : spectral_variability(dc, row, rm);
        v = silent ? 0.0f : v;
        if (b.taps) NNN_TIF(b, feat, NFEAT, f, tile, trow)[(size_t)(40 + part) * TILE] = v;
        store_split(FS, rm * WF_FS_W, row * WF_FS_W + 40 + part, v);
    }
    NNN_STAMPW(b, 13, f == 3);
}

// dense unit nbi of layer L on the 16 rows of the block; sink(row, neuron, value).  Its weights are requested by wf_dense_load,
// placed ahead of other work of the phase so that they travel behind it.
template <int KS> struct WfDenseW {
    Frags<1, KS> fr;
    float bias;
};
template <int KS>
__device__ __forceinline__ void wf_dense_load(WfDenseW<KS> &w, const LayerDesc &L, const uint4 *__restrict__ Wq, const float *__restrict__ fpar,
                                              int nbi, int lane)
{
    load_frags<1, 0, KS>(w.fr, L.in, Wq + L.in.wofs + (size_t)nbi * L.in.ksteps * 64, lane);
    const int neuron = nbi * 16 + (lane & 15);
    w.bias = neuron < L.n ? fpar[L.bias + neuron] : 0.0f;
}
template <bool QUAD = false, int KS, class Sink>   // (QUAD: as dense_layer's)
__device__ __forceinline__ void wf_dense(const LayerDesc &L, const unsigned short *Ain, int in_w, const uint4 *__restrict__ Wq, const WfDenseW<KS> &w,
                                         const float *tab, int nbi, int lane, Sink &&sink)
{
    const int neuron = nbi * 16 + (lane & 15);
    const uint4 *Bnb = Wq + L.in.wofs + (size_t)nbi * L.in.ksteps * 64;
    f32x4 acc[3][2];
    acc[0][0] = f32x4{w.bias, w.bias, w.bias, w.bias};
    gemm_acc<1, 1, 0, KS>(acc, Ain, WF_ROWS * in_w, in_w, 0, L.in, Bnb, lane, w.fr);
    if (neuron < L.n) {
        if constexpr (QUAD) {
            float v[4];
#pragma unroll
            for (int q = 0; q < 4; q++) v[q] = activate(L.act, acc[0][0][q] * (1.0f / 256.0f), tab);
            sink(4 * (lane >> 4), neuron, v);
        } else {
#pragma unroll
            for (int q = 0; q < 4; q++) sink(4 * (lane >> 4) + q, neuron, activate(L.act, acc[0][0][q] * (1.0f / 256.0f), tab));
        }
    }
}

#ifndef NNN_WF_MINWAVES
#define NNN_WF_MINWAVES 3   // waves per SIMD the register allocation must allow (12 waves = 3 per SIMD at <= 168 registers)
#endif
struct WfPlan {   // LDS strides (bf16 elements) of the per-layer matrices, set by the host from the model
    int w_v, w_n, w_dn;         // input windows: vad [cD ..], noise [cV ..], denoise [0 ..]
    int sw_v, sw_n, sw_dn;      // state / r * state matrices
};

__host__ __device__ constexpr WfPlan wf_plan_of(const RnnPlan &pl)
{
    return WfPlan{32 * pl.vad.in.ksteps + 8, 32 * pl.noise.in.ksteps + 8, 32 * pl.dn.in.ksteps + 8,
                  rnn_state_w(pl.vad), rnn_state_w(pl.noise), rnn_state_w(pl.dn)};
}
// byte offsets into k_rnn_wf's dynamic LDS: tanh table (256 floats); live flags [8][16] (frame f at slot f mod 8: written a tick before the
// first reader, read until three ticks after); 3 bf16 planes each of the vad input, the noise input (2 frame slots), the denoise input (3),
// the three state and the three r * state matrices and the feature staging; the cepstral ring [8 * 22][16], its pair distances [28][16] and
// the features wave's own cepstrum + pitch-correlation DCT [28][16].  The kernel takes its pointers from it, the host the total.
struct WfLds { int tab, live, Xv, Xn, Xdn, SPv, SPn, SPdn, RSv, RSn, RSdn, FS, crs, dc, cnb, total; };
__host__ __device__ constexpr WfLds wf_lds(const WfPlan &w)
{
    constexpr int plane3 = 3 * WF_ROWS * 2;   // bytes per column of a three-plane matrix
    WfLds o{};
    int at = 0;
    o.tab = lds_take(at, 256 * 4);
    o.live = lds_take(at, 8 * WF_ROWS * 4);
    o.Xv = lds_take(at, plane3 * w.w_v);
    o.Xn = lds_take(at, 2 * plane3 * w.w_n);
    o.Xdn = lds_take(at, 3 * plane3 * w.w_dn);
    o.SPv = lds_take(at, plane3 * w.sw_v);
    o.SPn = lds_take(at, plane3 * w.sw_n);
    o.SPdn = lds_take(at, plane3 * w.sw_dn);
    o.RSv = lds_take(at, plane3 * w.sw_v);
    o.RSn = lds_take(at, plane3 * w.sw_n);
    o.RSdn = lds_take(at, plane3 * w.sw_dn);
    o.FS = lds_take(at, plane3 * WF_FS_W);
    o.crs = lds_take(at, CEPS_MEM * NB * WF_ROWS * 4);
    o.dc = lds_take(at, 28 * WF_ROWS * 4);
    o.cnb = lds_take(at, 28 * WF_ROWS * 4);
    o.total = at;
    return o;
}
static_assert(wf_lds(wf_plan_of(BkShapeBuiltin::plan())).total == 127744, "k_rnn_wf's LDS for the built-in shape class");
// SH: a shape class with a compile-time packing plan (SH::plan(), e.g. BkShapeBuiltin of nnn_layout.h: every model of the built-in
// layer sizes) or WfShapeAny (the plan comes with the launch).  With a compile-time plan only the six activation kinds are taken from
// the launch's plan: every stride, column and fragment offset is a constant -- the run-time form keeps some fifty of them in scalar
// registers, more than the wave has, and pays for it in v_readlane / v_writelane spill traffic inside the tick loop (round 5: a sixth
// of the loop's vector instructions).  Same arithmetic either way.
struct WfShapeAny { static constexpr bool fixed = false; };
template <class SH> struct WfFixed { static constexpr bool value = true; };
template <> struct WfFixed<WfShapeAny> { static constexpr bool value = false; };
template <class SH>
__global__ void __launch_bounds__(64 * WF_WAVES, NNN_WF_MINWAVES) k_rnn_wf(Buffers b, RnnPlan pl_rt, WfPlan wp_rt, const uint4 *__restrict__ Wq,
                                                            const float *__restrict__ fpar, int tile0, int g)
{
    RnnPlan pl = pl_rt;
    WfPlan wp = wp_rt;
    if constexpr (WfFixed<SH>::value) {
        constexpr RnnPlan p0 = SH::plan();
        constexpr WfPlan w0 = wf_plan_of(p0);
        pl = p0;
        pl.dense.act = pl_rt.dense.act; pl.vad.act = pl_rt.vad.act; pl.noise.act = pl_rt.noise.act; pl.dn.act = pl_rt.dn.act;
        pl.out.act = pl_rt.out.act; pl.act_vo = pl_rt.act_vo;
        wp = w0;
    }
    HIP_DYNAMIC_SHARED(float, lds_raw)
    constexpr int rm = WF_ROWS;
    const int wave0 = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane0 = threadIdx.x & 63;
    int wave = wave0, lane = lane0;
    int tile, r0;                                            // r0: first row of the tile handled here
    if (!rnn_block_rows(b, tile0, rm, tile, r0)) return;
    if (!live_any(b, tile, r0, rm)) return;   // (... or all held, nnn_batch_hold_streams; held rows beside live ones: see k_rnn)
    const bool rowl = lane0 < rm;
    const int trow = r0 + (rowl ? lane0 : 0);
    NNN_STAMP(b, 50);
    // ---- LDS
    const WfLds o = wf_lds(wp);
    // (a float base with offsets in floats, and below the zeroed span as a pointer difference, where k_rnn and k_back take a byte base
    // and the span from the offsets: either of those here and the compiler orders k_rnn_wf<BkShapeBuiltin>'s instructions differently,
    // and the headline kernel is kept instruction for instruction what it was)
    auto planes = [&](int at) { return (unsigned short *)(lds_raw + at / 4); };   // (every offset is a whole number of 16-byte units)
    float *tab = lds_raw + o.tab / 4;
    int *live = (int *)(lds_raw + o.live / 4);
    unsigned short *Xv = planes(o.Xv), *Xn = planes(o.Xn), *Xdn = planes(o.Xdn);
    unsigned short *SPv = planes(o.SPv), *SPn = planes(o.SPn), *SPdn = planes(o.SPdn);
    unsigned short *RSv = planes(o.RSv), *RSn = planes(o.RSn), *RSdn = planes(o.RSdn);
    unsigned short *FS = planes(o.FS);
    float *crs = lds_raw + o.crs / 4, *dc = lds_raw + o.dc / 4, *cnb = lds_raw + o.cnb / 4;
    const int cD = pl.dense.out_col, cV = pl.cV, cF = pl.cF;
    float *sv = b.gru_v + ((size_t)tile * TILE * b.gru_v_w + (size_t)r0 * pl.vad.n),
          *sn = b.gru_n + ((size_t)tile * TILE * b.gru_n_w + (size_t)r0 * pl.noise.n),
          *sdn = b.gru_dn + ((size_t)tile * TILE * b.gru_dn_w + (size_t)r0 * pl.dn.n);
    // ---- once per launch: zero every operand plane, activation table, cepstral ring, states, pair distances
    {
        uint4 *z = (uint4 *)Xv;
        const int n16 = (int)(((char *)crs - (char *)Xv) / 16);
        for (int i = (int)threadIdx.x; i < n16; i += 64 * WF_WAVES) z[i] = make_uint4(0u, 0u, 0u, 0u);
        for (int i = (int)threadIdx.x; i < 201; i += 64 * WF_WAVES) tab[i] = b.tansig[i];
        const float *cm = NNN_TI(b.ceps_mem, CEPS_MEM * NB, tile, trow);
        constexpr int PER = (CEPS_MEM * NB + WF_WAVES - 1) / WF_WAVES;
        float stg[PER];
#pragma unroll
        for (int i = 0; i < PER; i++) {
            const int r = wave + i * WF_WAVES;
            stg[i] = (rowl && r < CEPS_MEM * NB) ? cm[(size_t)r * TILE] : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < PER; i++) {
            const int r = wave + i * WF_WAVES;
            if (rowl && r < CEPS_MEM * NB) crs[r * rm + lane] = stg[i];
        }
    }
    lds_barrier();
    constexpr int T = 64 * WF_WAVES;
    gru_state_io<T>(pl.vad, rm, sv, SPv, wp.sw_v, true);
    gru_state_io<T>(pl.noise, rm, sn, SPn, wp.sw_n, true);
    gru_state_io<T>(pl.dn, rm, sdn, SPdn, wp.sw_dn, true);
    if (rowl)
        for (int p = wave; p < 28; p += WF_WAVES) dc[p * rm + lane] = pair_dist(crs, p, lane, rm);
    int mem_id = wave == WF_WAVES - 1 ? NNN_TI(b.mem_id, 1, tile, r0 + (lane & 15))[0] : 0;   // every part of a row keeps a copy
    // this wave's GRU unit: its weights stay in registers for all ticks
    const int W_N = 6, W_V = 9, W_F = 11;   // first wave of the noise / vad roles; the features wave
    WfWeights wts;
    if (wave < W_N) wf_load_weights(wts, pl.dn, Wq, fpar, wave < pl.dn.nb ? wave : 0, lane);
    else if (wave < W_V) wf_load_weights(wts, pl.noise, Wq, fpar, wave - W_N < pl.noise.nb ? wave - W_N : 0, lane);
    else if (wave < W_F) wf_load_weights(wts, pl.vad, Wq, fpar, wave - W_V < pl.vad.nb ? wave - W_V : 0, lane);
    else wf_load_weights(wts, pl.vad, Wq, fpar, 0, lane);   // (the features wave keeps its prefetched inputs there)
    lds_barrier();
    NNN_STAMP(b, 51);
    WfGru ua;   // the GRU unit of this wave (denoise / noise / vad by role), first phase -> second phase
    if (wave == WF_WAVES - 1 && g > 0) wf_features_load(wts, b, 0, tile, r0, lane);
    // the features wave is all vector ALU on one wave while the GRU waves wait on matrix results: let it issue first
    if (wave0 == WF_WAVES - 1) wf_setprio_high();
    for (int t = -1; t < g + 3; t++) {
        lane = launder_v(lane0);   // keep the tick loop's addresses inside the loop (see launder_v)
        wave = launder_s(wave0);
        const int fv = t, fn = t - 1, fd = t - 2, fo = t - 3, ff = t + 1;   // the frame each layer works on in this tick
        const bool on_v = fv >= 0 && fv < g, on_n = fn >= 0 && fn < g, on_d = fd >= 0 && fd < g, on_o = fo >= 0 && fo < g,
                   on_f = ff >= 0 && ff < g;
        unsigned short *Xn_n = Xn + (fn & 1) * 3 * rm * wp.w_n;               // noise input of frame fn
        unsigned short *Xdn_d = Xdn + ((fd + 3) % 3) * 3 * rm * wp.w_dn;      // denoise input of frame fd
        // role stamps of a mid-group tick: slots 30 + 5 role + {0: tick start, 1: first phase done, 2: past barrier, 3: second phase done, 4: past barrier}
        const int srole = wave0 == 0 ? 0 : (wave0 == 6 ? 1 : (wave0 == 9 ? 2 : (wave0 == 11 ? 3 : -1)));
        NNN_STAMPW(b, 30 + 5 * srole, t == 2 && srole >= 0);
        // ---------------- first phase
        if (wave < W_N) {
            if (on_d && wave < pl.dn.nb) wf_gru_a(pl.dn, Xdn_d, wp.w_dn, SPdn, RSdn, wp.sw_dn, Wq, wts, tab, wave, lane, ua);
        } else if (wave < W_V) {
            if (on_n && wave - W_N < pl.noise.nb) wf_gru_a(pl.noise, Xn_n - cV, wp.w_n, SPn, RSn, wp.sw_n, Wq, wts, tab, wave - W_N, lane, ua);
        } else if (wave < W_F) {
            WfDenseW<3> dw;   // the output layer reads the denoise state: <= 96 columns in this shape class
            const bool mine_o = on_o && wave - W_V < pl.out.nb;   // (the output layer has 22 neurons: two units, one per vad wave)
            if (on_v && wave - W_V < pl.vad.nb) wf_gru_a(pl.vad, Xv - cD, wp.w_v, SPv, RSv, wp.sw_v, Wq, wts, tab, wave - W_V, lane, ua);
            if (mine_o) {   // gains of frame fo and their smoothing
                const int *lv = live + 16 * (fo & 7);
                wf_dense_load(dw, pl.out, Wq, fpar, wave - W_V, lane);
                wf_dense<true>(pl.out, SPdn, wp.sw_dn, Wq, dw, tab, wave - W_V, lane, [&](int lrow, int band, const float (&v)[4]) {
                    if (b.link) {   // (nnn_batch_set_channel_link: one gain per band for the channels of a link group)
                        rnn_gain_out4(b, fo, tile, r0 + lrow, band, lv + lrow, v);
                    } else {
#pragma unroll
                        for (int q = 0; q < 4; q++) rnn_gain_out(b, fo, tile, r0 + lrow + q, band, lv[lrow + q] != 0, v[q]);
                    }
                });
            }
        } else {
            if (on_f) wf_features(b, wf_features_in(wts), ff, tile, r0, lane, crs, dc, cnb, FS, live + 16 * (ff & 7), mem_id);
            if (ff + 1 >= 0 && ff + 1 < g) wf_features_load(wts, b, ff + 1, tile, r0, lane);   // the next tick's inputs start travelling
        }
        NNN_STAMPW(b, 31 + 5 * srole, t == 2 && srole >= 0);
#if defined(NNN_STAMPS) && NNN_WFSTAMP_PHASE == 1
        NNN_STAMPW(b, 14 + wave0, t == 2);   // every wave's end of the first phase (scripts/gpu_stamps_rnn.sh)
#endif
        lds_barrier();
        NNN_STAMPW(b, 32 + 5 * srole, t == 2 && srole >= 0);
        // ---------------- second phase
        if (wave < W_N) {
            // the denoise units' second phase is the shortest of all: the first waves also take the input dense layer of
            // frame ff (ref: src/rnn.rs:353-355) on the features staged in the first phase; two k-steps (42 features)
            WfDenseW<2> dw;
            const bool mine_d = on_f && wave < pl.dense.nb;
            if (on_d && wave < pl.dn.nb)
                wf_gru_b(pl.dn, RSdn, wp.sw_dn, Wq, wts, tab, live + 16 * (fd & 7), wave, lane, ua,
                         [&](int row, int n, float v) { store_split(SPdn, rm * wp.sw_dn, row * wp.sw_dn + n, v); });
            if (mine_d) {
                unsigned short *Xnn = Xn + (ff & 1) * 3 * rm * wp.w_n;
                wf_dense_load(dw, pl.dense, Wq, fpar, wave, lane);
                wf_dense(pl.dense, FS - cF, WF_FS_W, Wq, dw, tab, wave, lane, [&](int row, int n, float v) {
                    store_split(Xv, rm * wp.w_v, row * wp.w_v + n, v);                      // vad window starts at cD
                    store_split(Xnn, rm * wp.w_n, row * wp.w_n + (cD - cV) + n, v);
                });
            }
        } else if (wave < W_V) {
            if (on_n && wave - W_N < pl.noise.nb) {
                unsigned short *Xd = Xdn + (fn % 3) * 3 * rm * wp.w_dn;   // the denoise layer's input of the same frame
                wf_gru_b(pl.noise, RSn, wp.sw_n, Wq, wts, tab, live + 16 * (fn & 7), wave - W_N, lane, ua, [&](int row, int n, float v) {
                    store_split(SPn, rm * wp.sw_n, row * wp.sw_n + n, v);
                    store_split(Xd, rm * wp.w_dn, row * wp.w_dn + n, v);
                });
            }
            if (on_f) {
                // feature fan-out, dealt over the noise waves: the staged features of frame ff -> the noise and denoise inputs
                // of that frame (48 columns)
                unsigned short *Xnn = Xn + (ff & 1) * 3 * rm * wp.w_n, *Xd = Xdn + (ff % 3) * 3 * rm * wp.w_dn;
                for (int i = 64 * (wave - W_N) + lane; i < 3 * rm * 6; i += 64 * (W_V - W_N)) {
                    const int plx = i / (rm * 6), rem = i - plx * rm * 6, row = rem / 6, c8 = rem - row * 6;
                    const uint4 v = *(const uint4 *)(FS + (size_t)plx * rm * WF_FS_W + row * WF_FS_W + 8 * c8);
                    *(uint4 *)(Xnn + (size_t)plx * rm * wp.w_n + row * wp.w_n + (cF - cV) + 8 * c8) = v;
                    *(uint4 *)(Xd + (size_t)plx * rm * wp.w_dn + row * wp.w_dn + cF + 8 * c8) = v;
                }
            }
        } else if (wave < W_F) {
            if (on_v && wave - W_V < pl.vad.nb) {
                unsigned short *Xnn = Xn + (fv & 1) * 3 * rm * wp.w_n, *Xd = Xdn + (fv % 3) * 3 * rm * wp.w_dn;
                wf_gru_b(pl.vad, RSv, wp.sw_v, Wq, wts, tab, live + 16 * (fv & 7), wave - W_V, lane, ua, [&](int row, int n, float v) {
                    store_split(SPv, rm * wp.sw_v, row * wp.sw_v + n, v);
                    store_split(Xnn, rm * wp.w_n, row * wp.w_n + n, v);               // noise window starts at cV
                    store_split(Xd, rm * wp.w_dn, row * wp.w_dn + cV + n, v);
                });
            }
        } else {
            if (on_n && rowl) {
                // vad output of frame fn, from the copy of that frame's vad state in the noise layer's input (columns 0.. of its window;
                // not rewritten before tick fn + 2)
                const unsigned short *Xv1 = Xn + (fn & 1) * 3 * rm * wp.w_n;
                NNN_TIF(b, vad, 1, fn, tile, trow)[0] = rnn_vad_out(pl, fpar, Xv1, rm * wp.w_n, wp.w_n, 0, lane, live + 16 * (fn & 7), tab);
            }
        }
        NNN_STAMPW(b, 33 + 5 * srole, t == 2 && srole >= 0);
#if defined(NNN_STAMPS) && NNN_WFSTAMP_PHASE == 2
        NNN_STAMPW(b, 14 + wave0, t == 2);   // ... or of the second
#endif
        lds_barrier();
        NNN_STAMPW(b, 34 + 5 * srole, t == 2 && srole >= 0);
    }
    // ---- states back to HBM
    gru_state_io<T>(pl.vad, rm, sv, SPv, wp.sw_v, false);
    gru_state_io<T>(pl.noise, rm, sn, SPn, wp.sw_n, false);
    gru_state_io<T>(pl.dn, rm, sdn, SPdn, wp.sw_dn, false);
    if (wave0 == WF_WAVES - 1 && rowl) NNN_TI(b.mem_id, 1, tile, trow)[0] = mem_id;   // (part 0 of every row)
    NNN_STAMP(b, 52);
}

}  // namespace nnn
