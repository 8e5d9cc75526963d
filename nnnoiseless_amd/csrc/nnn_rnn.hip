#pragma once
// nnn_rnn.hip -- K10, the network: activations, bf16 split planes, the MFMA GEMM pieces, the layer pieces the three RNN kernels share (the
// block prologue, state load and store, gain and VAD output), the GRU and dense layers and k_rnn (layers one after the other) with its
// LDS layout.  Not a translation unit: nnn_kernels.hip includes it between the feature stage and k_rnn_wf; k_rnn_wf (nnn_rnn_wf.hip) and
// k_back (nnn_back.hip) use these pieces.

namespace nnn {

// ---------------------------------------------------------------------------------------------
// K10 rnn: dense + 3 GRUs + 2 dense, i8-origin weights, activations via the 201-entry tanh table.
//     ref: src/rnn.rs:251-272, 292-327, 343-379, 402-410; src/util.rs:29-53.
//     Batched GEMMs on the matrix cores: a tile's activations live in LDS as [stream][column] matrices in three bf16 planes
//     (x = hi + mid + lo exactly), the weights are small integers (exact in bf16) packed on the host in MFMA B-fragment order,
//     so v_mfma_f32_16x16x32_bf16 accumulates exact products.  Two kernels share these pieces: k_rnn (layers one after the
//     other, any model the format allows) and k_rnn_wf (layers of different frames side by side, the built-in shape class).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float tansig_approx(float x, const float *tab)
{
    // ref: src/util.rs:29-45, written without branches so that a lane's many evaluations overlap (the table
    // read is a dependent LDS access).  Same arithmetic for |x| < 8; the saturation tests (which also catch
    // NaN exactly like the reference's reversed comparisons) select the result at the end.
    const float ax = fabsf(x);
    float fi = floorf(0.5f + 25.0f * ax);
    fi = fminf(fi, 200.0f);   // only reached when the result is discarded (|x| >= 8 or NaN)
    const float xr = ax - 0.04f * fi;
    const float y0 = tab[(int)fi];
    const float dy = 1.0f - y0 * y0;
    const float y = y0 + xr * dy * (1.0f - y0 * xr);
    const float r = x < 0.0f ? -y : y;
    return !(x < 8.0f) ? 1.0f : (!(x > -8.0f) ? -1.0f : r);
}
__device__ __forceinline__ float sigmoid_approx(float x, const float *tab) { return 0.5f + 0.5f * tansig_approx(0.5f * x, tab); }
__device__ __forceinline__ float activate(int act, float x, const float *tab)
{
    if (act == 0) return tansig_approx(x, tab);
    if (act == 1) return sigmoid_approx(x, tab);
    return fmaxf(x, 0.0f);
}

constexpr int RNN_WAVES = 8;

__device__ __forceinline__ unsigned short bf16_rn(float x)   // round to nearest even
{
    unsigned u = __float_as_uint(x);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}
__device__ __forceinline__ float bf16_f32(unsigned short h) { return __uint_as_float((unsigned)h << 16); }

// x = hi + mid + lo exactly (8 + 8 + 8 significand bits), one bf16 plane each.  Truncation, not rounding: hi is the top
// half of x's word, the remainder x - hi is exact and has <= 16 significant bits, its top half is mid, and what is left
// has <= 8 bits and is a bf16 as it stands.
__device__ __forceinline__ void store_split(unsigned short *P, int plane_stride, int idx, float x)
{
    const unsigned uh = __float_as_uint(x) & 0xFFFF0000u;
    const float r1 = x - __uint_as_float(uh);
    const unsigned um = __float_as_uint(r1) & 0xFFFF0000u;
    const float r2 = r1 - __uint_as_float(um);
    P[idx] = (unsigned short)(uh >> 16);
    P[idx + plane_stride] = (unsigned short)(um >> 16);
    P[idx + 2 * plane_stride] = (unsigned short)(__float_as_uint(r2) >> 16);
}
__device__ __forceinline__ float load_split(const unsigned short *P, int plane_stride, int idx)
{
    return (bf16_f32(P[idx]) + bf16_f32(P[idx + plane_stride])) + bf16_f32(P[idx + 2 * plane_stride]);
}

// operand planes in the products: all three (two -- activations truncated to 16 significand bits -- were measured in round 4,
// profiles/r4_experiments_ab.txt B)
constexpr int GPL = 3;
// Weight fragments of one GEMM group: all k-steps (up to KSMAX) are requested together so that a layer pays
// one trip to the Infinity Cache / HBM instead of one per k-step.
constexpr int KSMAX = 4;
template <int NG, int KS = KSMAX> struct Frags { uint4 f[KS][NG]; };

template <int NG, int G0, int KS = KSMAX>
__device__ __forceinline__ void load_frags(Frags<NG, KS> &fr, const GemmDesc &g, const uint4 *__restrict__ Bnb, int lane)
{
#pragma unroll
    for (int ks = 0; ks < KS; ks++)
#pragma unroll
        for (int gi = 0; gi < NG; gi++)
            fr.f[ks][gi] = ks < g.ksteps ? Bnb[((G0 + gi) * g.ksteps + ks) * 64 + lane] : make_uint4(0u, 0u, 0u, 0u);
}

// acc[G0 + g][mb] += A[16 (mb0 + mb) .. +15][kbase ..] * B(gate G0 + g), g < NG, mb < MB, over all k-steps and
// the three activation planes.  Bnb points at this neuron block's fragments ([gate][k-step][lane]).
// (k_back's bk_gemm / bk_frags_load stay a form of their own, as do the four feature stages: each a parallelisation chosen by measurement)
template <int NG, int MB, int G0, int KS = KSMAX>
__device__ __forceinline__ void gemm_acc(f32x4 (&acc)[3][2], const unsigned short *A, int plane_stride, int row_w, int mb0,
                                         const GemmDesc &g, const uint4 *__restrict__ Bnb, int lane, const Frags<NG, KS> &fr)
{
    const unsigned short *a0 = A + (size_t)(mb0 * 16 + (lane & 15)) * row_w + g.kbase + 8 * (lane >> 4);
    const size_t mb_stride = (size_t)16 * row_w;
    // Software pipeline over (k-step, stream block): the three plane fragments of the next step are read from
    // LDS before the current step's 3*NG MFMAs issue, so LDS latency hides behind matrix work.
    const int steps = g.ksteps * MB;
    uint4 cur[3], nxt[3];
#pragma unroll
    for (int pl = 0; pl < GPL; pl++) cur[pl] = *(const uint4 *)(a0 + (size_t)pl * plane_stride);
    for (int ks = 0; ks < g.ksteps; ks++) {
        uint4 bfr[NG];
        if (ks < KS) {
#pragma unroll
            for (int gi = 0; gi < NG; gi++) {
                bfr[gi] = fr.f[0][gi];
#pragma unroll
                for (int u = 1; u < KS; u++) bfr[gi] = (ks == u) ? fr.f[u][gi] : bfr[gi];
            }
        } else {   // more k-steps than the fragment set holds: fetch as we go
#pragma unroll
            for (int gi = 0; gi < NG; gi++) bfr[gi] = Bnb[((G0 + gi) * g.ksteps + ks) * 64 + lane];
        }
#pragma unroll
        for (int mb = 0; mb < MB; mb++) {
            const int step = ks * MB + mb;
            if (step + 1 < steps) {
                const int ks1 = (mb + 1 < MB) ? ks : ks + 1, mb1 = (mb + 1 < MB) ? mb + 1 : 0;
                const unsigned short *ap = a0 + mb1 * mb_stride + ks1 * 32;
#pragma unroll
                for (int pl = 0; pl < GPL; pl++) nxt[pl] = *(const uint4 *)(ap + (size_t)pl * plane_stride);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int pl = 0; pl < GPL; pl++)
#pragma unroll
                for (int gi = 0; gi < NG; gi++) acc[G0 + gi][mb] = mfma_16x16x32_bf16(cur[pl], bfr[gi], acc[G0 + gi][mb]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int pl = 0; pl < GPL; pl++) cur[pl] = nxt[pl];
        }
    }
}

// ---- pieces the three RNN kernels share (k_rnn, k_rnn_wf, k_back): the same operations in the same order, so that they give the same bits

// carving a kernel's dynamic LDS: the byte offset of the next `bytes` (whole 16-byte units)
__host__ __device__ constexpr int lds_take(int &at, int bytes) { const int r = at; at += (bytes + 15) & ~15; return r; }

// The block's tile and the first of its `rm` rows in it (blocks dealt over the XCDs by xcd_tile_block; tile0: first tile of this model's
// run).  False: every stream of the block is padding -- the last tile of a batch that is not a multiple of 64 -- and it has nothing to do.
__device__ __forceinline__ bool rnn_block_rows(const Buffers &b, int tile0, int rm, int &tile, int &r0)
{
    const int per = TILE / rm;
    int sub;
    xcd_tile_block((int)blockIdx.x, (tile0 & 7) ? 1 : (int)gridDim.x / per, per, tile, sub);
    tile += tile0;
    r0 = sub * rm;
    return tile * TILE + r0 < b.S;
}

// a layer's state: its stream-major array in HBM (the `rm` rows of this block) <-> its LDS planes, all THREADS threads of the block
template <int THREADS>
__device__ __forceinline__ void gru_state_io(const LayerDesc &L, int rm, float *state, unsigned short *SP, int sw, bool load)
{
    const int n = rm * L.n;
    for (int e = (int)threadIdx.x; e < n; e += THREADS) {
        const int row = e / L.n, col = e - row * L.n;
        if (load) store_split(SP, rm * sw, row * sw + col, state[e]);
        else state[e] = load_split(SP, rm * sw, row * sw + col);
    }
}

// vad output, 1 x nv, lane = stream (ref: src/rnn.rs:359): the vad state of row `lane` sits at column c0 of matrix X (plane stride ps, row
// stride w); `live`: the rows' live flags of that frame
__device__ __forceinline__ float rnn_vad_out(const RnnPlan &pl, const float *__restrict__ fpar, const unsigned short *X, int ps, int w, int c0,
                                             int lane, const int *live, const float *tab)
{
    float acc = fpar[pl.vo_b];
    for (int k = 0; k < pl.vad.n; k++) acc = fmaf(fpar[pl.vo_w + k], load_split(X, ps, lane * w + c0 + k), acc);
    return live[lane] ? activate(pl.act_vo, acc * (1.0f / 256.0f), tab) : 0.0f;
}

// gain `v` of (row, band) of frame f (ref: src/rnn.rs:378) and its smoothing g = max(g, 0.6 lastg) (ref: src/denoise.rs:106-109); a silent
// frame (`lv` false) has gains 0 and leaves lastg alone.  A batch with gain floors (nnn_batch_set_gain_floor; b.gfloor is null without):
// the raw gain of a non-silent frame is fmaxf(v, the stream's floor of the band) before the tap, the smoothing and k_synth see it
__device__ __forceinline__ void rnn_gain_out(const Buffers &b, int f, int tile, int row, int band, bool lv, float v)
{
    if (b.gfloor) v = fmaxf(v, NNN_TI(b.gfloor, NB, tile, row)[(size_t)band * TILE]);
    const float gr = lv ? v : 0.0f;
    NNN_TIF(b, g_raw, NB, f, tile, row)[(size_t)band * TILE] = gr;
    float gs = 0.0f;
    if (lv) {
        float *lg = NNN_TI(b.lastg, NB, tile, row) + (size_t)band * TILE;
        gs = fmaxf(gr, 0.6f * *lg);
        *lg = gs;
    }
    NNN_TIF(b, g, NB, f, tile, row)[(size_t)band * TILE] = gs;
}

// Channel link (nnn_batch_set_channel_link; `link` is Buffers::link, not 0): the network's gains `v` of one band for the four rows 4 k ..
// 4 k + 3 of a tile -- what a lane of the output layer's 16x16 accumulator holds -- become one common gain per link group.  Rows are batch
// indices modulo 4 (tiles and blocks start at multiples of 16), so the pairs (0, 1) and (2, 3) are the 2-channel groups and the four rows
// the 4-channel group.  A row takes part while its frame is not silent (`nonsilent`, the kernel's per-row flags) and its stream is live
// (bit q of `live4`); a row that does not keeps its own value and gives none, and a group with one member left keeps that member's value.
// Max and min of finite values are exact and order-free: the host's max / min over the same members gives the same bits.
__device__ __forceinline__ void link_quad(int link, const int *nonsilent, unsigned live4, const float (&v)[4], float (&out)[4])
{
    const bool mn = link < 0;
    const float idle = mn ? INFINITY : -INFINITY;
    bool m[4];
    float x[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        m[q] = nonsilent[q] != 0 && ((live4 >> q) & 1u) != 0u;
        x[q] = m[q] ? v[q] : idle;
    }
    const float p01 = mn ? fminf(x[0], x[1]) : fmaxf(x[0], x[1]), p23 = mn ? fminf(x[2], x[3]) : fmaxf(x[2], x[3]);
    const float all = mn ? fminf(p01, p23) : fmaxf(p01, p23);
    const bool four = link == 4 || link == -4;
#pragma unroll
    for (int q = 0; q < 4; q++) out[q] = m[q] ? (four ? all : (q < 2 ? p01 : p23)) : v[q];
}
// rnn_gain_out for the four rows row0 .. row0 + 3 (row0 a multiple of 4) of a linked batch: link first, then each stream's own floor
__device__ __forceinline__ void rnn_gain_out4(const Buffers &b, int f, int tile, int row0, int band, const int *nonsilent, const float (&v)[4])
{
    float lk[4];
    link_quad(b.link, nonsilent, (unsigned)(live_word(b, tile) >> row0) & 15u, v, lk);
#pragma unroll
    for (int q = 0; q < 4; q++) rnn_gain_out(b, f, tile, row0 + q, band, nonsilent[q] != 0, lk[q]);
}

struct RnnLds {
    const float *tab;
    int *live;            // rows whose frame is not silent (this frame)
    unsigned short *IN;   // input operand matrix [rm][in_w], 3 planes
    unsigned short *RS;   // r * state of the layer in progress [rm][rec_w], 3 planes
    int in_ps, rs_ps;     // plane strides (elements)
    int rm;               // stream rows of this block: 32 or 16
};

// One GRU layer (ref: src/rnn.rs:292-327) as three GEMM groups on the matrix cores.  A wave owns one
// (neuron block, MB stream blocks) unit: z, r and the input part of the candidate accumulate together,
// r * state goes through LDS (every candidate needs all of it), then the recurrent part of the candidate and the state
// update.  The state itself lives in the layer's own LDS planes `SP` (row stride `sw`; three bf16 planes hold an f32
// exactly) for all frames of the launch: recurrent operand of the GEMMs, read back by the owning wave for the update, and
// rewritten by it -- a layer costs two barriers, and no state travels to HBM and back between frames.
// `idle` runs on waves without a unit while the others are in the first GEMM phase (the next frame's features).
// KS: the k-steps whose weight fragments are requested up front and held in registers (24 registers per k-step; a GEMM of more k-steps
// fetches the rest as it goes, see gemm_acc).  k_vad, whose layer has one k-step in the built-in shape class, asks for one.
template <int MB, int KS = KSMAX, class Idle>
__device__ __forceinline__ void gru_layer(const Buffers &b, const LayerDesc &L, const RnnPlan &pl, const RnnLds &lds, unsigned short *SP,
                                          int sw, const uint4 *__restrict__ Wq, const float *__restrict__ fpar,
                                          int wave, int lane, Idle &&idle)
{
    const float scale = 1.0f / 256.0f;
    const int groups = (lds.rm >> 4) / MB, units = L.nb * groups;
    const bool mine = wave < units;
    const int nbi = mine ? wave / groups : 0, mb0 = (wave % groups) * MB;
    const int neuron = nbi * 16 + (lane & 15);
    const bool nvalid = mine && neuron < L.n;
    const int sp_ps = lds.rm * sw;
    const uint4 *Bin = Wq + L.in.wofs + (size_t)nbi * 3 * L.in.ksteps * 64;
    const uint4 *Brec = Wq + L.rec.wofs + (size_t)nbi * 3 * L.rec.ksteps * 64;
    // all weight fragments of this layer start travelling now
    Frags<3, KS> f_in;
    Frags<2, KS> f_zr;
    Frags<1, KS> f_h;
    load_frags<3, 0, KS>(f_in, L.in, Bin, lane);
    load_frags<2, 0, KS>(f_zr, L.rec, Brec, lane);
    load_frags<1, 2, KS>(f_h, L.rec, Brec, lane);
    float bias[3];
#pragma unroll
    for (int g = 0; g < 3; g++) bias[g] = (neuron < L.n) ? fpar[L.bias + g * L.n + neuron] : 0.0f;
    NNN_STAMP(b, 16);
    f32x4 acc[3][2];
    float zz[2][4], sold[2][4];
    if (mine) {
#pragma unroll
        for (int g = 0; g < 3; g++) {
#pragma unroll
            for (int mb = 0; mb < MB; mb++) acc[g][mb] = f32x4{bias[g], bias[g], bias[g], bias[g]};
        }
        gemm_acc<2, MB, 0, KS>(acc, SP, sp_ps, sw, mb0, L.rec, Brec, lane, f_zr);   // (recurrent part first: the order k_rnn_wf uses)
        gemm_acc<3, MB, 0, KS>(acc, lds.IN, lds.in_ps, pl.in_w, mb0, L.in, Bin, lane, f_in);
        // r * state: the columns of this neuron block, plus (last block) the padding up to the GEMM's k range, as zeros
        const int kcols = 32 * L.rec.ksteps;
#pragma unroll
        for (int mb = 0; mb < MB; mb++)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int row = (mb0 + mb) * 16 + 4 * (lane >> 4) + q;
                const float so = nvalid ? load_split(SP, sp_ps, row * sw + neuron) : 0.0f;   // the three planes hold the state exactly
                sold[mb][q] = so;
                zz[mb][q] = sigmoid_approx(scale * acc[0][mb][q], lds.tab);
                const float rs = so * sigmoid_approx(scale * acc[1][mb][q], lds.tab);
                if (neuron < kcols) store_split(lds.RS, lds.rs_ps, row * pl.rec_w + neuron, rs);
                if (nbi == L.nb - 1 && neuron + 16 < kcols) store_split(lds.RS, lds.rs_ps, row * pl.rec_w + neuron + 16, 0.0f);
            }
        NNN_STAMP(b, 22);
    } else {
        idle();
    }
    lds_barrier();   // r * state complete; every wave is done reading the old state planes
    NNN_STAMP(b, 18);
    if (mine) {
        gemm_acc<1, MB, 2, KS>(acc, lds.RS, lds.rs_ps, pl.rec_w, mb0, L.rec, Brec, lane, f_h);
        NNN_STAMP(b, 23);
        if (nvalid) {
#pragma unroll
            for (int mb = 0; mb < MB; mb++)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int row = (mb0 + mb) * 16 + 4 * (lane >> 4) + q;
                    const float hh = activate(L.act, scale * acc[2][mb][q], lds.tab);
                    const float z = zz[mb][q], so = sold[mb][q];
                    float snew = z * so + (1.0f - z) * hh;
                    snew = lds.live[row] ? snew : so;   // silent frames leave the state alone (ref: src/denoise.rs:100)
                    store_split(lds.IN, lds.in_ps, row * pl.in_w + L.out_col + neuron, snew);
                    store_split(SP, sp_ps, row * sw + neuron, snew);
                }
        }
        NNN_STAMP(b, 26);
    }
    lds_barrier();
}

// dense layer on the matrix cores: act(W x + b) for every (neuron block, 16-stream block) unit, units dealt round-robin to
// the block's waves (a layer wider than the waves are many takes several rounds); `sink(row, neuron, value)` per output.  QUAD: the four
// rows a lane holds of its neuron in one call, `sink(first row, neuron, values[4])` (the channel link's form of the gains sink, link_quad)
template <bool QUAD = false, class Sink>
__device__ __forceinline__ void dense_layer(const LayerDesc &L, const RnnPlan &pl, const RnnLds &lds, const uint4 *__restrict__ Wq,
                                            const float *__restrict__ fpar, int wave, int lane, Sink &&sink)
{
    const int mbt = lds.rm >> 4, units = L.nb * mbt;
    for (int unit = wave; unit < units; unit += RNN_WAVES) {
        const int nbi = unit / mbt, mb0 = unit % mbt;
        const int neuron = nbi * 16 + (lane & 15);
        const uint4 *Bnb = Wq + L.in.wofs + (size_t)nbi * L.in.ksteps * 64;
        Frags<1> fr;
        load_frags<1, 0>(fr, L.in, Bnb, lane);
        const float bv = neuron < L.n ? fpar[L.bias + neuron] : 0.0f;
        f32x4 acc[3][2];
        acc[0][0] = f32x4{bv, bv, bv, bv};
        gemm_acc<1, 1, 0>(acc, lds.IN, lds.in_ps, pl.in_w, mb0, L.in, Bnb, lane, fr);
        if (neuron < L.n) {
            if constexpr (QUAD) {
                float v[4];
#pragma unroll
                for (int q = 0; q < 4; q++) v[q] = activate(L.act, acc[0][0][q] * (1.0f / 256.0f), lds.tab);
                sink(mb0 * 16 + 4 * (lane >> 4), neuron, v);
            } else {
#pragma unroll
                for (int q = 0; q < 4; q++)
                    sink(mb0 * 16 + 4 * (lane >> 4) + q, neuron, activate(L.act, acc[0][0][q] * (1.0f / 256.0f), lds.tab));
            }
        }
    }
}

// pair index of rows i < j among the 8 ring rows, in spectral_variability's order
__device__ __forceinline__ int pair_index(int i, int j) { return i * (15 - i) / 2 + (j - i - 1); }

// The feature stage of one frame for one row (lane = stream), start to finish without leaving the lane: cepstral-ring
// update, delta features, spectral variability (ref: src/features.rs:170-219).  The ring (`crs`) and the 28 pairwise
// cepstral distances (`dc`) stay in LDS for all frames of the launch: a new cepstrum changes only the 7 distances it
// takes part in, the other 21 are the same sums over the same rows as the reference recomputes.  Writes the 42 features as
// three bf16 planes into the staging `FS` (row stride FS_W) and the row's live flag for that frame.
constexpr int FS_W = 56;   // 48 feature columns + 8: 16-byte rows, odd multiple of 16 bytes
__device__ __forceinline__ void features_row(const Buffers &b, int f, int tile, int trow, int ll, int rm, float *crs, float *dc,
                                             unsigned short *FS, int fs_w, int *live_next, int &mem_id)
{
    const float *cg = NNN_TIF(b, cn, 28, f, tile, trow);
    float cn[28];
#pragma unroll
    for (int i = 0; i < 28; i++) cn[i] = cg[(size_t)i * TILE];
    const int pitch = NNN_TIF(b, pitch, 1, f, tile, trow)[0];
    const bool silent = NNN_TIF(b, silence, 1, f, tile, trow)[0] != 0;
    float fr[NFEAT];
    if (silent) {   // "if there's no audio, avoid messing up the state" (ref: src/features.rs:160-166)
#pragma unroll
        for (int i = 0; i < NFEAT; i++) fr[i] = 0.0f;
    } else {
        float *cm = NNN_TI(b.ceps_mem, CEPS_MEM * NB, tile, trow);
        const int c0 = mem_id, c1 = mem_id < 1 ? CEPS_MEM + mem_id - 1 : mem_id - 1;
        const int c2 = mem_id < 2 ? CEPS_MEM + mem_id - 2 : mem_id - 2;
#pragma unroll
        for (int k = 0; k < NB; k++) {
            cm[(size_t)(c0 * NB + k) * TILE] = cn[k];
            crs[(c0 * NB + k) * rm + ll] = cn[k];
        }
        mem_id = mem_id + 1 == CEPS_MEM ? 0 : mem_id + 1;
#pragma unroll
        for (int i = 0; i < NB; i++) fr[i] = cn[i];
#pragma unroll
        for (int i = 0; i < 6; i++) {
            const float v1 = crs[(c1 * NB + i) * rm + ll], v2 = crs[(c2 * NB + i) * rm + ll];
            const float v0 = cn[i];
            fr[i] = v0 + v1 + v2;
            fr[NB + i] = v0 - v2;
            fr[NB + 6 + i] = v0 - 2.0f * v1 + v2;
            fr[NB + 12 + i] = cn[NB + i];
        }
        fr[40] = 0.01f * ((float)pitch - 300.0f);
        // the 7 distances the new row takes part in, each summed over the 22 bands in order (ref: src/features.rs:203-208)
        for (int j = 0; j < CEPS_MEM; j++) {
            if (j == c0) continue;
            float dist = 0.0f;
#pragma unroll
            for (int k = 0; k < NB; k++) {
                const float d = cn[k] - crs[(j * NB + k) * rm + ll];
                dist += d * d;
            }
            dc[pair_index(j < c0 ? j : c0, j < c0 ? c0 : j) * rm + ll] = dist;
        }
        fr[41] = spectral_variability(dc, ll, rm);
    }
    live_next[ll] = silent ? 0 : 1;
    if (b.taps) {
        float *fo = NNN_TIF(b, feat, NFEAT, f, tile, trow);
#pragma unroll
        for (int k = 0; k < NFEAT; k++) fo[(size_t)k * TILE] = fr[k];
    }
#pragma unroll
    for (int k = 0; k < NFEAT; k++) store_split(FS, rm * fs_w, ll * fs_w + k, fr[k]);
}

// ---------------------------------------------------------------------------------------------
// K10 rnn: the feature stage's recurrent part and the network (ref: src/rnn.rs:343-379) for the `g` frames of a group in
//     one launch.  `rm` stream rows (32 or 16 of a 64-stream tile) per block, 8 waves; GEMMs on the matrix cores with
//     exact products (bf16 weights, activations as three bf16 planes).  Across the frames of the launch the GRU states stay in
//     registers and LDS, the cepstral ring and its pair distances in LDS; the last wave prepares frame f + 1's features
//     while the others are inside frame f's GRU GEMMs (when the layer shapes leave it without a unit).
// ---------------------------------------------------------------------------------------------
// byte offsets into k_rnn's dynamic LDS at `rows` stream rows per block: tanh table (256 floats), live flags of this frame and the next
// (2 x 64 ints); 3 bf16 planes each of the input matrix, the r * state matrix, the three state matrices and the feature staging; the
// cepstral ring [8 * 22][rows] and its pair distances [28][rows].  The kernel takes its pointers from it, the host the total.
struct RnnLdsAt {
    int tab, live, IN, RS, SPv, SPn, SPdn, FS, crs, dc, total;
    int sw_v, sw_n, sw_dn;   // row strides of the state matrices
};
__host__ __device__ constexpr RnnLdsAt rnn_lds(const RnnPlan &pl, int rows)
{
    RnnLdsAt o{};
    o.sw_v = rnn_state_w(pl.vad); o.sw_n = rnn_state_w(pl.noise); o.sw_dn = rnn_state_w(pl.dn);
    int at = 0;
    o.tab = lds_take(at, 256 * 4);
    o.live = lds_take(at, 2 * 64 * 4);
    o.IN = lds_take(at, 3 * rows * pl.in_w * 2);
    o.RS = lds_take(at, 3 * rows * pl.rec_w * 2);
    o.SPv = lds_take(at, 3 * rows * o.sw_v * 2);
    o.SPn = lds_take(at, 3 * rows * o.sw_n * 2);
    o.SPdn = lds_take(at, 3 * rows * o.sw_dn * 2);
    o.FS = lds_take(at, 3 * rows * FS_W * 2);
    o.crs = lds_take(at, CEPS_MEM * NB * rows * 4);
    o.dc = lds_take(at, 28 * rows * 4);
    o.total = at;
    return o;
}
static_assert(rnn_lds(BkShapeBuiltin::plan(), 16).total == 66816 && rnn_lds(BkShapeBuiltin::plan(), 32).total == 132096, "k_rnn's LDS for the built-in shape class");

// LINK: the batch links the channels of its stream groups (nnn_batch_set_channel_link) -- the instantiation whose gains sink takes a lane's
// four rows of a band together (rnn_gain_out4); the launch plan picks it only while a link is on.  A template flag as in k_back, not a
// run-time test of b.link as in k_rnn_wf: this kernel keeps some five hundred scalars in vector lanes, and a run-time test -- around the
// whole sink, around link_quad alone, or carried in the rows' LDS flags -- moved its register allocation from 203 to 205 - 209 registers.
template <bool LINK = false>
__global__ void __launch_bounds__(64 * RNN_WAVES) k_rnn(Buffers b, RnnPlan pl, const uint4 *__restrict__ Wq,
                                                          const float *__restrict__ fpar, int tile0, int rm, int g)
{
    HIP_DYNAMIC_SHARED(float, lds_raw)
    char *ldsb = (char *)lds_raw;
    const int wave0 = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane0 = threadIdx.x & 63;
    int wave = wave0, lane = lane0, tid = threadIdx.x;
    const int mbt = rm >> 4;
    int tile, r0;                                          // r0: first row of the tile handled here
    if (!rnn_block_rows(b, tile0, rm, tile, r0)) return;
    // (... or all held, nnn_batch_hold_streams.  A block with live rows also runs its held rows, whose feature rows k_fft_xp -- which returns
    // by four streams -- may not have written in this call: stale or creation-time zeros.  Rows never mix here -- each GEMM row is its own
    // input row times the shared weights, the live flags are per row -- and a held row's results go to its own dead state.  DESIGN.md section 13.)
    if (!live_any(b, tile, r0, rm)) return;
    const bool rowl = lane < rm;                           // lane = stream phases: this lane has a row
    const int trow = r0 + (rowl ? lane : 0);               // its row in the tile
    // ---- LDS
    const RnnLdsAt o = rnn_lds(pl, rm);
    float *tab = (float *)(ldsb + o.tab);
    int *live = (int *)(ldsb + o.live), *live_next = live + 64;
    unsigned short *IN = (unsigned short *)(ldsb + o.IN), *RS = (unsigned short *)(ldsb + o.RS);
    const int in_ps = rm * pl.in_w, rs_ps = rm * pl.rec_w;
    const int sw_v = o.sw_v, sw_n = o.sw_n, sw_dn = o.sw_dn;
    unsigned short *SPv = (unsigned short *)(ldsb + o.SPv), *SPn = (unsigned short *)(ldsb + o.SPn), *SPdn = (unsigned short *)(ldsb + o.SPdn);
    unsigned short *FS = (unsigned short *)(ldsb + o.FS);
    float *crs = (float *)(ldsb + o.crs);              // cepstral ring [8 * 22][rm]
    float *dc = (float *)(ldsb + o.dc);                // pair distances [28][rm]
    RnnLds lds{tab, live, IN, RS, in_ps, rs_ps, rm};
    float *sv = b.gru_v + ((size_t)tile * TILE * b.gru_v_w + (size_t)r0 * pl.vad.n),
          *sn = b.gru_n + ((size_t)tile * TILE * b.gru_n_w + (size_t)r0 * pl.noise.n),
          *sdn = b.gru_dn + ((size_t)tile * TILE * b.gru_dn_w + (size_t)r0 * pl.dn.n);
    NNN_STAMP(b, 8);
    // stream blocks per wave unit of a GRU: one, or both of a 32-row block's when the layer has more than four neuron blocks
    // (units = neuron blocks x stream-block groups must stay within the 8 waves)
    const int mb_v = pl.vad.nb * mbt <= RNN_WAVES ? 1 : 2;
    const int mb_n = pl.noise.nb * mbt <= RNN_WAVES ? 1 : 2;
    const int mb_dn = pl.dn.nb * mbt <= RNN_WAVES ? 1 : 2;
#define NNN_MB(mb, CALL)            \
    {                               \
        if ((mb) == 2) { CALL(2) }  \
        else { CALL(1) }            \
    }
    // ---- once per launch: zero every operand plane (padding columns must read as 0), activation table, ring, states
    {
        uint4 *z = (uint4 *)IN;
        const int n16 = (o.crs - o.IN) / 16;
        for (int i = tid; i < n16; i += 64 * RNN_WAVES) z[i] = make_uint4(0u, 0u, 0u, 0u);
        for (int i = tid; i < 201; i += 64 * RNN_WAVES) tab[i] = b.tansig[i];
        const float *cm = NNN_TI(b.ceps_mem, CEPS_MEM * NB, tile, trow);
        constexpr int PER = (CEPS_MEM * NB + RNN_WAVES - 1) / RNN_WAVES;   // 22 rows per wave, all in flight
        float stg[PER];
#pragma unroll
        for (int i = 0; i < PER; i++) {
            const int r = wave + i * RNN_WAVES;
            stg[i] = (rowl && r < CEPS_MEM * NB) ? cm[(size_t)r * TILE] : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < PER; i++) {
            const int r = wave + i * RNN_WAVES;
            if (rowl && r < CEPS_MEM * NB) crs[r * rm + lane] = stg[i];
        }
    }
    lds_barrier();
    constexpr int T = 64 * RNN_WAVES;
    gru_state_io<T>(pl.vad, rm, sv, SPv, sw_v, true);
    gru_state_io<T>(pl.noise, rm, sn, SPn, sw_n, true);
    gru_state_io<T>(pl.dn, rm, sdn, SPdn, sw_dn, true);
    if (rowl)
        for (int p = wave; p < 28; p += RNN_WAVES) dc[p * rm + lane] = pair_dist(crs, p, lane, rm);
    int mem_id = (wave == RNN_WAVES - 1 && rowl) ? NNN_TI(b.mem_id, 1, tile, trow)[0] : 0;
    lds_barrier();
    // frame 0's features (the last wave; the others have nothing to do yet)
    if (wave == RNN_WAVES - 1 && rowl) features_row(b, 0, tile, trow, lane, rm, crs, dc, FS, FS_W, live_next, mem_id);
    NNN_STAMP(b, 9);
    for (int f = 0; f < g; f++) {
        // keep the frame loop's addresses inside the loop (see launder_v)
        lane = launder_v(lane0);
        wave = launder_s(wave0);
        tid = 64 * wave + lane;
        lds_barrier();   // features of frame f staged; the previous frame is done with the input matrix
        {   // staged features -> their columns of the input matrix; live flags
            const int n8 = rm * 6;   // 48 columns = 6 x 16 bytes per row and plane
            for (int i = tid; i < 3 * n8; i += 64 * RNN_WAVES) {
                const int plx = i / n8, rem = i - plx * n8, row = rem / 6, c8 = rem - row * 6;
                *(uint4 *)(IN + (size_t)plx * in_ps + row * pl.in_w + pl.cF + 8 * c8) =
                    *(const uint4 *)(FS + (size_t)plx * rm * FS_W + row * FS_W + 8 * c8);
            }
            if (tid < 64) live[tid] = live_next[tid];
        }
        lds_barrier();
        NNN_STAMP(b, 10);
        bool feat_done = (f + 1 >= g);   // wave-uniform: the next frame's features are staged (or there is no next frame)
        auto feat_next = [&]() {
            if (wave == RNN_WAVES - 1 && !feat_done) {
                if (rowl) features_row(b, f + 1, tile, trow, lane, rm, crs, dc, FS, FS_W, live_next, mem_id);
                feat_done = true;
            }
        };
        auto no_idle = []() {};
        // input dense (ref: src/rnn.rs:353-355)
        dense_layer(pl.dense, pl, lds, Wq, fpar, wave, lane, [&](int row, int neuron, float v) {
            store_split(IN, in_ps, row * pl.in_w + pl.dense.out_col + neuron, v);
        });
        lds_barrier();
        NNN_STAMP(b, 11);
#define NNN_GRU_V(M) gru_layer<M>(b, pl.vad, pl, lds, SPv, sw_v, Wq, fpar, wave, lane, no_idle);
#define NNN_GRU_N(M) gru_layer<M>(b, pl.noise, pl, lds, SPn, sw_n, Wq, fpar, wave, lane, feat_next);
#define NNN_GRU_DN(M) gru_layer<M>(b, pl.dn, pl, lds, SPdn, sw_dn, Wq, fpar, wave, lane, feat_next);
        NNN_MB(mb_v, NNN_GRU_V)                                             // ref: src/rnn.rs:356-358
        NNN_STAMP(b, 12);
        if (wave == RNN_WAVES - 1 && rowl) NNN_TIF(b, vad, 1, f, tile, trow)[0] = rnn_vad_out(pl, fpar, IN, in_ps, pl.in_w, pl.cV, lane, live, tab);
        NNN_MB(mb_n, NNN_GRU_N)                                             // ref: src/rnn.rs:361-366
        NNN_STAMP(b, 13);
        NNN_MB(mb_dn, NNN_GRU_DN)                                           // ref: src/rnn.rs:368-377
        NNN_STAMP(b, 14);
        // gains and their smoothing
        if constexpr (LINK)
            dense_layer<true>(pl.out, pl, lds, Wq, fpar, wave, lane,
                              [&](int lrow, int band, const float (&v)[4]) { rnn_gain_out4(b, f, tile, r0 + lrow, band, live + lrow, v); });
        else
            dense_layer(pl.out, pl, lds, Wq, fpar, wave, lane,
                        [&](int lrow, int band, float v) { rnn_gain_out(b, f, tile, r0 + lrow, band, live[lrow] != 0, v); });
        feat_next();   // layer shapes that keep every wave busy: the next frame's features go last
        NNN_STAMP(b, 15);
    }
    // ---- states back to HBM (the last layer's update is behind its closing barrier)
    gru_state_io<T>(pl.vad, rm, sv, SPv, sw_v, false);
    gru_state_io<T>(pl.noise, rm, sn, SPn, sw_n, false);
    gru_state_io<T>(pl.dn, rm, sdn, SPdn, sw_dn, false);
    if (wave == RNN_WAVES - 1 && rowl) NNN_TI(b.mem_id, 1, tile, trow)[0] = mem_id;
#undef NNN_MB
}

}  // namespace nnn
