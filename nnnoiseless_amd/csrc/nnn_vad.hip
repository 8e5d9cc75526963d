#pragma once
// nnn_vad.hip -- k_vad, the network cut off behind the VAD output (nnn_batch_vad_*): input dense, VAD GRU and the
// one-neuron VAD output for the frames of a group, from the feature rows k_features left.  Built from the layer pieces of nnn_rnn.hip
// (dense_layer, gru_layer, rnn_vad_out, gru_state_io) on the model's packed weights as they are: the same operations in the same order
// as k_rnn, hence the same bits.  Not a translation unit: nnn_kernels.hip includes it behind the RNN kernels.

namespace nnn {

// ---------------------------------------------------------------------------------------------
// K14 vad: ref src/rnn.rs:353-359 -- and nothing of 361-378.
//     The VAD branch reads three column ranges of the RNN's input matrix -- the VAD state, the features, the dense output -- and none of
//     the noise state in front of them, so the block's input matrix starts at the VAD state: vad_plan_view is the model's plan with every
//     column moved down by cV and the two row strides cut to what the branch reads.  Only addresses change; weights, fragment
//     offsets, k-steps and biases are the model's.  With the noise and denoise state matrices gone as well, a block of the built-in shape
//     class keeps a whole 64-stream tile in 76.5 KB (k_rnn: 129 KB for 32 rows), and the eight (neuron block, 16-stream block) units of
//     the dense layer and of the GRU are one per wave.  Two blocks per compute unit need four waves per SIMD as well: 128 registers.  The
//     GRU therefore keeps one k-step of weight fragments in registers (gru_layer<MB, 1>: 24 registers where k_rnn holds 96; the built-in
//     class's VAD GRU has one k-step per GEMM, a wider layer fetches the others as it goes) and the kernel is bound to four waves
//     (99 VGPRs, no spill; with k_rnn's four k-steps it took 169, two waves per SIMD, one block per compute unit whatever the LDS).
// ---------------------------------------------------------------------------------------------
__host__ __device__ constexpr RnnPlan vad_plan_view(const RnnPlan &pl)
{
    RnnPlan v = pl;
    const int c0 = pl.cV;
    v.cV = 0;
    v.cF = pl.cF - c0;
    v.dense.in.kbase = pl.dense.in.kbase - c0;
    v.dense.out_col = pl.dense.out_col - c0;
    v.vad.in.kbase = pl.vad.in.kbase - c0;
    v.vad.out_col = pl.vad.out_col - c0;
    const int wd = v.dense.in.kbase + 32 * v.dense.in.ksteps, wv = v.vad.in.kbase + 32 * v.vad.in.ksteps;
    const int width = wd > wv ? wd : wv;
    v.in_w = (width + 15) / 16 * 16 + 8;   // (16 bytes mod 32, as rnn_plan_for's)
    v.rec_w = rnn_state_w(pl.vad);         // r * state of the VAD GRU alone
    return v;
}
// byte offsets into k_vad's dynamic LDS at `rows` stream rows per block: tanh table, the live flags of two frames, 3 bf16 planes each of the
// input matrix, the r * state matrix and the VAD state.  `pv`: the plan view.
struct VadLdsAt {
    int tab, live, IN, RS, SPv, total;
    int sw_v;
};
__host__ __device__ constexpr VadLdsAt vad_lds(const RnnPlan &pv, int rows)
{
    VadLdsAt o{};
    o.sw_v = rnn_state_w(pv.vad);
    int at = 0;
    o.tab = lds_take(at, 256 * 4);
    o.live = lds_take(at, 2 * 64 * 4);
    o.IN = lds_take(at, 3 * rows * pv.in_w * 2);
    o.RS = lds_take(at, 3 * rows * pv.rec_w * 2);
    o.SPv = lds_take(at, 3 * rows * o.sw_v * 2);
    o.total = at;
    return o;
}
static_assert(vad_plan_view(BkShapeBuiltin::plan()).in_w == 120 && vad_lds(vad_plan_view(BkShapeBuiltin::plan()), 64).total == 78336,
              "k_vad's LDS for the built-in shape class: two blocks of 64 rows per compute unit");
// Stream-block pairing of the GRU's wave units at `rows` rows per block (gru_layer<MB>): 1 or 2; 0 = the layer's units do not fit
// the eight waves at this many rows.
__host__ __device__ constexpr int vad_gru_mb(const RnnPlan &pl, int rows)
{
    const int mbt = rows >> 4;
    if (pl.vad.nb * mbt <= RNN_WAVES) return 1;
    return (mbt % 2 == 0 && pl.vad.nb * (mbt / 2) <= RNN_WAVES) ? 2 : 0;
}

// `rm` stream rows (64, 32 or 16 of a tile) per block, 8 waves; blocks dealt as k_rnn's (rnn_block_rows).  A frame is four barriers:
//   features of frame f in the input matrix | dense | GRU phase one | GRU phase two | VAD output (wave 7) beside frame f + 1's features
//   going from registers into the input matrix (waves 0 .. 6)
// Frame f + 1's feature rows and silence flags are requested from memory at the top of frame f and arrive behind its GEMMs.  The live flags
// are kept for two frames: frame f's are read by the VAD output while frame f + 1's are written.
// `sp`: the group's parameter table; sp[f].vad is the caller's row of frame f (or null).  Written for live streams only: never for the
// padding behind the batch's last stream, never for a held stream; the scratch `vad` row (the tap) is written for every row, like k_rnn's.
constexpr int VAD_LOADERS = 64 * (RNN_WAVES - 1);                           // threads that carry feature values: waves 0 .. 6
constexpr int VAD_FPT = (NFEAT * TILE + VAD_LOADERS - 1) / VAD_LOADERS;     // values per loader thread at 64 rows: 6
__global__ void __launch_bounds__(64 * RNN_WAVES, 4) k_vad(Buffers b, const StepParams *__restrict__ sp, RnnPlan pl, const uint4 *__restrict__ Wq,
                                                          const float *__restrict__ fpar, int tile0, int rm, int mb, int g)
{
    HIP_DYNAMIC_SHARED(float, lds_raw)
    char *ldsb = (char *)lds_raw;
    const int wave0 = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane0 = threadIdx.x & 63;
    int wave = wave0, lane = lane0, tid = threadIdx.x;
    int tile, r0;
    if (!rnn_block_rows(b, tile0, rm, tile, r0)) return;
    if (!live_any(b, tile, r0, rm)) return;   // (a block with live rows also runs its held rows, each on its own dead state: see k_rnn)
    const bool rowl = lane < rm;
    const int trow = r0 + (rowl ? lane : 0);
    const int s = tile * TILE + trow;
    const bool writes = rowl && s < b.S && live_stream(b, tile, trow);   // this lane's stream has a row in the caller's buffer
    const RnnPlan pv = vad_plan_view(pl);
    const VadLdsAt o = vad_lds(pv, rm);
    float *tab = (float *)(ldsb + o.tab);
    int *live2 = (int *)(ldsb + o.live);
    unsigned short *IN = (unsigned short *)(ldsb + o.IN), *RS = (unsigned short *)(ldsb + o.RS), *SPv = (unsigned short *)(ldsb + o.SPv);
    const int in_ps = rm * pv.in_w, rs_ps = rm * pv.rec_w, sw_v = o.sw_v;
    float *sv = b.gru_v + ((size_t)tile * TILE * b.gru_v_w + (size_t)r0 * pl.vad.n);
    // ---- once per launch: zero every operand plane (padding columns must read as 0), the activation table, the state
    {
        uint4 *z = (uint4 *)IN;
        const int n16 = (o.total - o.IN) / 16;
        for (int i = tid; i < n16; i += 64 * RNN_WAVES) z[i] = make_uint4(0u, 0u, 0u, 0u);
        for (int i = tid; i < 201; i += 64 * RNN_WAVES) tab[i] = b.tansig[i];
    }
    lds_barrier();
    gru_state_io<64 * RNN_WAVES>(pl.vad, rm, sv, SPv, sw_v, true);
    // feature e of the block's rm x 42 values: column e / rm of row e % rm (consecutive lanes on consecutive streams of the tile-interleaved rows)
    const int nfe = NFEAT * rm, rsh = rm == 64 ? 6 : (rm == 32 ? 5 : 4);
    float fv[VAD_FPT];
    int sil = 0;
    auto fetch = [&](int f) {
        if (wave < RNN_WAVES - 1) {
            const float *fg = NNN_TIF(b, feat, NFEAT, f, tile, r0);
#pragma unroll
            for (int i = 0; i < VAD_FPT; i++) {
                const int e = tid + VAD_LOADERS * i, k = e >> rsh, row = e & (rm - 1);
                fv[i] = e < nfe ? fg[(size_t)k * TILE + row] : 0.0f;
            }
        } else {
            sil = NNN_TIF(b, silence, 1, f, tile, trow)[0];
        }
    };
    auto stage = [&](int f) {   // ... into the input matrix at cF (columns 42 .. 47 stay zero) and the frame's live flags
        if (wave < RNN_WAVES - 1) {
#pragma unroll
            for (int i = 0; i < VAD_FPT; i++) {
                const int e = tid + VAD_LOADERS * i, k = e >> rsh, row = e & (rm - 1);
                if (e < nfe) store_split(IN, in_ps, row * pv.in_w + pv.cF + k, fv[i]);
            }
        } else if (rowl) {
            live2[(f & 1) * 64 + lane] = sil != 0 ? 0 : 1;
        }
    };
    fetch(0);
    stage(0);
    auto no_idle = []() {};
    for (int f = 0; f < g; f++) {
        // keep the frame loop's addresses inside the loop (see launder_v)
        lane = launder_v(lane0);
        wave = launder_s(wave0);
        tid = 64 * wave + lane;
        lds_barrier();   // features and live flags of frame f in place (first frame: the state planes too)
        RnnLds lds{tab, live2 + (f & 1) * 64, IN, RS, in_ps, rs_ps, rm};
        if (f + 1 < g) fetch(f + 1);
        // input dense (ref: src/rnn.rs:353-355)
        dense_layer(pv.dense, pv, lds, Wq, fpar, wave, lane, [&](int row, int neuron, float v) {
            store_split(IN, in_ps, row * pv.in_w + pv.dense.out_col + neuron, v);
        });
        lds_barrier();
        // vad GRU (ref: src/rnn.rs:356-358)
        if (mb == 2) gru_layer<2, 1>(b, pv.vad, pv, lds, SPv, sw_v, Wq, fpar, wave, lane, no_idle);
        else gru_layer<1, 1>(b, pv.vad, pv, lds, SPv, sw_v, Wq, fpar, wave, lane, no_idle);
        // vad output (ref: src/rnn.rs:359) on the last wave; the others lay the next frame's features out (the dense layer, their only reader, is done)
        if (wave == RNN_WAVES - 1) {
            if (rowl) {
                const float v = rnn_vad_out(pl, fpar, IN, in_ps, pv.in_w, pv.cV, lane, lds.live, tab);
                NNN_TIF(b, vad, 1, f, tile, trow)[0] = v;
                float *row = sp[f].vad;
                if (writes && row) row[s] = v;
            }
        }
        if (f + 1 < g) stage(f + 1);
    }
    // ---- the state back to HBM (the last update is behind the GRU's closing barrier)
    gru_state_io<64 * RNN_WAVES>(pl.vad, rm, sv, SPv, sw_v, false);
}

}  // namespace nnn
