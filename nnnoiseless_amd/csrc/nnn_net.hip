#pragma once
// nnn_net.hip -- k_net, the network alone (nnn_batch_network_*): RnnState::compute for the frames of a call on the
// caller's feature rows, raw gains and VAD out to the caller's rows, and nothing else of the frame.  Built from the layer pieces of
// nnn_rnn.hip (dense_layer, gru_layer, rnn_vad_out, gru_state_io, rnn_block_rows) on the model's plan and packed weights as they are: the
// same layer calls in the same order as k_rnn, hence the same bits.  Not a translation unit: nnn_kernels.hip includes it behind nnn_vad.hip.

namespace nnn {

// the caller's row buffers of a network call (device memory, dense, no rows for the padding streams behind the batch's last one)
struct NetIo {
    const float *features;   // [n_frames][n_streams][42]
    const int *silence;      // [n_frames][n_streams], may be null: no frame is silent
    float *gains;            // [n_frames][n_streams][22]
    float *vad;              // [n_frames][n_streams], may be null
};

// ---------------------------------------------------------------------------------------------
// K15 net: ref src/rnn.rs:343-379 -- k_rnn without features_row, the cepstral ring, the pair distances and mem_id in front, and without
//     the lastg smoothing and the scratch stores behind.  Its LDS is k_rnn's minus the staging planes, the ring and the distances
//     (1152 bytes per row): a frame's feature rows wait in registers instead (three values per thread at 32 rows).
//     The GRUs keep two k-steps of weight fragments in registers (gru_layer<MB, NET_KS>: 48 registers where k_rnn holds 96; further k-steps
//     are fetched as the GEMM goes, gemm_acc's existing path, same values) and the kernel is bound to four waves per SIMD: 114 VGPRs, no
//     spill (163 and two waves per SIMD with k_rnn's four), so that two 16-row blocks share a compute unit -- measured, DESIGN.md section 16.
// ---------------------------------------------------------------------------------------------
// byte offsets into k_net's dynamic LDS at `rows` stream rows per block: tanh table, the live flags (k_rnn's 2 x 64 ints, so that the
// layouts differ by whole arrays only; this kernel uses the first 64), 3 bf16 planes each of the input matrix, the r * state matrix and the
// three state matrices.
struct NetLdsAt {
    int tab, live, IN, RS, SPv, SPn, SPdn, total;
    int sw_v, sw_n, sw_dn;   // row strides of the state matrices
};
__host__ __device__ constexpr NetLdsAt net_lds(const RnnPlan &pl, int rows)
{
    NetLdsAt o{};
    o.sw_v = rnn_state_w(pl.vad); o.sw_n = rnn_state_w(pl.noise); o.sw_dn = rnn_state_w(pl.dn);
    int at = 0;
    o.tab = lds_take(at, 256 * 4);
    o.live = lds_take(at, 2 * 64 * 4);
    o.IN = lds_take(at, 3 * rows * pl.in_w * 2);
    o.RS = lds_take(at, 3 * rows * pl.rec_w * 2);
    o.SPv = lds_take(at, 3 * rows * o.sw_v * 2);
    o.SPn = lds_take(at, 3 * rows * o.sw_n * 2);
    o.SPdn = lds_take(at, 3 * rows * o.sw_dn * 2);
    o.total = at;
    return o;
}
static_assert(net_lds(BkShapeBuiltin::plan(), 16).total == 48384 && net_lds(BkShapeBuiltin::plan(), 32).total == 95232 &&
                  rnn_lds(BkShapeBuiltin::plan(), 32).total - net_lds(BkShapeBuiltin::plan(), 32).total == 32 * 1152,
              "k_net's LDS for the built-in shape class: k_rnn's minus 1152 bytes per row");
// (the second 64 live ints are 256 bytes per block that nothing reads: the price of that identity, and no block fewer per compute unit)

// `rm` stream rows (32 or 16 of a tile) per block, 8 waves, blocks dealt as k_rnn's.  A frame:
//   barrier | frame f's features from registers into the input matrix, its live flags | barrier | frame f + 1's rows requested |
//   the layers as k_rnn runs them; the VAD value (last wave) and the gains (the output layer's sink) straight to the caller's rows
// Frame f + 1's features stay in registers until frame f is done with the input matrix: all three GRUs read the feature columns.
// The rows of a block for one frame are one run of rm * 42 floats in the caller's buffer: consecutive lanes on consecutive floats.
// Rows without a place in the caller's buffers -- the padding behind the batch's last stream, held streams -- are never loaded or
// stored: they run on zeros as silent rows (their state stays put) and their results are dropped.
constexpr int NET_T = 64 * RNN_WAVES;
constexpr int NET_KS = 2;                                   // k-steps of weight fragments a GRU keeps in registers
constexpr int NET_FPT = (NFEAT * 32 + NET_T - 1) / NET_T;   // feature values per thread at 32 rows: 3
__global__ void __launch_bounds__(NET_T, 4) k_net(Buffers b, NetIo io, RnnPlan pl, const uint4 *__restrict__ Wq, const float *__restrict__ fpar,
                                                int tile0, int rm, int g)
{
    HIP_DYNAMIC_SHARED(float, lds_raw)
    char *ldsb = (char *)lds_raw;
    const int wave0 = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane0 = threadIdx.x & 63;
    int wave = wave0, lane = lane0, tid = threadIdx.x;
    const int mbt = rm >> 4;
    int tile, r0;
    if (!rnn_block_rows(b, tile0, rm, tile, r0)) return;   // every row is padding
    if (!live_any(b, tile, r0, rm)) return;                // ... or held
    const bool rowl = lane < rm;
    const size_t S = (size_t)b.S, s0 = (size_t)tile * TILE + r0;   // s0 < S (rnn_block_rows)
    const int nrow = S - s0 < (size_t)rm ? (int)(S - s0) : rm;     // rows of this block inside the batch
    const unsigned long long lw = live_word(b, tile) >> r0;        // bit r: row r is live
    const bool writes = rowl && lane < nrow && ((lw >> lane) & 1ull) != 0ull;   // this lane's stream has a row in the caller's buffers
    // ---- LDS
    const NetLdsAt o = net_lds(pl, rm);
    float *tab = (float *)(ldsb + o.tab);
    int *live = (int *)(ldsb + o.live);
    unsigned short *IN = (unsigned short *)(ldsb + o.IN), *RS = (unsigned short *)(ldsb + o.RS);
    const int in_ps = rm * pl.in_w, rs_ps = rm * pl.rec_w;
    const int sw_v = o.sw_v, sw_n = o.sw_n, sw_dn = o.sw_dn;
    unsigned short *SPv = (unsigned short *)(ldsb + o.SPv), *SPn = (unsigned short *)(ldsb + o.SPn), *SPdn = (unsigned short *)(ldsb + o.SPdn);
    RnnLds lds{tab, live, IN, RS, in_ps, rs_ps, rm};
    float *sv = b.gru_v + ((size_t)tile * TILE * b.gru_v_w + (size_t)r0 * pl.vad.n),
          *sn = b.gru_n + ((size_t)tile * TILE * b.gru_n_w + (size_t)r0 * pl.noise.n),
          *sdn = b.gru_dn + ((size_t)tile * TILE * b.gru_dn_w + (size_t)r0 * pl.dn.n);
    const int mb_v = pl.vad.nb * mbt <= RNN_WAVES ? 1 : 2;
    const int mb_n = pl.noise.nb * mbt <= RNN_WAVES ? 1 : 2;
    const int mb_dn = pl.dn.nb * mbt <= RNN_WAVES ? 1 : 2;
#define NNN_MB(mb, CALL)            \
    {                               \
        if ((mb) == 2) { CALL(2) }  \
        else { CALL(1) }            \
    }
    // ---- once per launch: zero every operand plane (padding columns must read as 0), the activation table, the states
    {
        uint4 *z = (uint4 *)IN;
        const int n16 = (o.total - o.IN) / 16;
        for (int i = tid; i < n16; i += NET_T) z[i] = make_uint4(0u, 0u, 0u, 0u);
        for (int i = tid; i < 201; i += NET_T) tab[i] = b.tansig[i];
    }
    lds_barrier();
    gru_state_io<NET_T>(pl.vad, rm, sv, SPv, sw_v, true);
    gru_state_io<NET_T>(pl.noise, rm, sn, SPn, sw_n, true);
    gru_state_io<NET_T>(pl.dn, rm, sdn, SPdn, sw_dn, true);
    // value e of the block's run of rm * 42 floats: feature e % 42 of row e / 42
    const int nfe = NFEAT * rm, nfe_in = NFEAT * nrow;
    float fv[NET_FPT];
    int sil = 0;
    auto fetch = [&](int f) {
        const float *fg = io.features + ((size_t)f * S + s0) * NFEAT;
#pragma unroll
        for (int i = 0; i < NET_FPT; i++) {
            const int e = tid + NET_T * i, row = e / NFEAT;
            fv[i] = (e < nfe_in && ((lw >> row) & 1ull) != 0ull) ? fg[e] : 0.0f;
        }
        if (wave == RNN_WAVES - 1) sil = (writes && io.silence) ? io.silence[(size_t)f * S + s0 + lane] : 0;
    };
    auto stage = [&]() {   // ... into the input matrix at cF (columns 42 .. 47 stay zero) and the frame's live flags
#pragma unroll
        for (int i = 0; i < NET_FPT; i++) {
            const int e = tid + NET_T * i, row = e / NFEAT, k = e - row * NFEAT;
            if (e < nfe) store_split(IN, in_ps, row * pl.in_w + pl.cF + k, fv[i]);
        }
        if (wave == RNN_WAVES - 1 && rowl) live[lane] = (writes && sil == 0) ? 1 : 0;
    };
    fetch(0);
    auto no_idle = []() {};
    for (int f = 0; f < g; f++) {
        // keep the frame loop's addresses inside the loop (see launder_v)
        lane = launder_v(lane0);
        wave = launder_s(wave0);
        tid = 64 * wave + lane;
        lds_barrier();   // the previous frame is done with the input matrix and the live flags (first frame: the state planes are in place)
        stage();
        lds_barrier();
        if (f + 1 < g) fetch(f + 1);
        // input dense (ref: src/rnn.rs:353-355)
        dense_layer(pl.dense, pl, lds, Wq, fpar, wave, lane, [&](int row, int neuron, float v) {
            store_split(IN, in_ps, row * pl.in_w + pl.dense.out_col + neuron, v);
        });
        lds_barrier();
#define NNN_NET_V(M) gru_layer<M, NET_KS>(b, pl.vad, pl, lds, SPv, sw_v, Wq, fpar, wave, lane, no_idle);
#define NNN_NET_N(M) gru_layer<M, NET_KS>(b, pl.noise, pl, lds, SPn, sw_n, Wq, fpar, wave, lane, no_idle);
#define NNN_NET_DN(M) gru_layer<M, NET_KS>(b, pl.dn, pl, lds, SPdn, sw_dn, Wq, fpar, wave, lane, no_idle);
        NNN_MB(mb_v, NNN_NET_V)                                             // ref: src/rnn.rs:356-358
        if (wave == RNN_WAVES - 1 && rowl) {                                // ref: src/rnn.rs:359
            const float v = rnn_vad_out(pl, fpar, IN, in_ps, pl.in_w, pl.cV, lane, live, tab);
            if (writes && io.vad) io.vad[(size_t)f * S + s0 + lane] = v;
        }
        NNN_MB(mb_n, NNN_NET_N)                                             // ref: src/rnn.rs:361-366
        NNN_MB(mb_dn, NNN_NET_DN)                                           // ref: src/rnn.rs:368-377
        // the raw gains (ref: src/rnn.rs:378); a silent frame's are +0
        float *gg = io.gains + ((size_t)f * S + s0) * NB;
        dense_layer(pl.out, pl, lds, Wq, fpar, wave, lane, [&](int lrow, int band, float v) {
            if (lrow < nrow && ((lw >> lrow) & 1ull) != 0ull) gg[lrow * NB + band] = live[lrow] ? v : 0.0f;
        });
    }
    // ---- states back to HBM (the last GRU's update is behind its closing barrier)
    gru_state_io<NET_T>(pl.vad, rm, sv, SPv, sw_v, false);
    gru_state_io<NET_T>(pl.noise, rm, sn, SPn, sw_n, false);
    gru_state_io<NET_T>(pl.dn, rm, sdn, SPdn, sw_dn, false);
#undef NNN_NET_V
#undef NNN_NET_N
#undef NNN_NET_DN
#undef NNN_MB
}

}  // namespace nnn
