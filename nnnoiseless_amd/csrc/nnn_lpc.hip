#pragma once
// nnn_lpc.hip -- K2, the LPC analysis ahead of the pitch stage: k_lpc, k_lpc_wide and lpc_finish, which k_pitch shares.  Not a translation
// unit: nnn_kernels.hip includes it between the high-pass stage and the pitch stage.

namespace nnn {

// ---------------------------------------------------------------------------------------------
// K2  lpc: the part of pitch_downsample between the decimation and the FIR -- 5-lag autocorrelation of the 864-value window,
//     lag window, order-4 Levinson recursion, bandwidth expansion and the extra zero (ref: src/pitch.rs:433-446, 460-480,
//     257-292) -- lane = stream on the tile-interleaved decimated ring, one wave per (tile, up to eight consecutive frames).
//     Each of the five sums is a serial chain of 860 steps in the reference's order; inside k_pitch (one block per 16
//     streams) they occupied two waves for 8.7 of the block's 44 us with the other six waiting behind a barrier.  Here every lane
//     carries its own stream's five chains (independent of each other: five-way instruction-level parallelism on full waves), the
//     frames of a group run side by side (nothing here carries over from frame to frame; a wave takes up to four consecutive
//     frames and reads the rows their windows share once), every load is a whole 256-byte row, and the launch rides on the high-pass stream, ahead of the pitch stage.  Output: ac[5], FIR taps[5] per stream-frame.
// ---------------------------------------------------------------------------------------------
constexpr int LPC_CH = 20;    // rows per unrolled chunk: 860 = 43 x 20
constexpr int LPC_CHW = 43;   // k_lpc_wide: 20 chunks.  A lone one-frame launch has the GPU to itself and is paced by the trips to memory it
                              // makes one after the other, not by the rows in flight: 23.5 -> 17 us for a frame of 4096 streams (of which some
                              // 8 us are the launch; 86 rows on four waves per block, with the overflow in AGPRs, measured no better)
static_assert((XLP - 4) % LPC_CH == 0 && (XLP - 4) % LPC_CHW == 0, "");
// lags K0 .. K0 + NK - 1 of the autocorrelation of the 864 rows at base[i * TILE] (row 0 replaced by x0): the reference's
// sequential sum per lag, then its tail (ref: src/pitch.rs:433-446)
template <int K0, int NK, int CH>
__device__ __forceinline__ void lpc_chains(const float *base, float x0, float (&ac)[NK])
{
    float cur[CH + 4], nxt[CH];
#pragma unroll
    for (int i = 0; i < CH + 4; i++) cur[i] = base[(size_t)i * TILE];
    cur[0] = x0;
    float c[NK];
#pragma unroll
    for (int k = 0; k < NK; k++) c[k] = 0.0f;
    constexpr int NCH = (XLP - 4) / CH;
#pragma nounroll
    for (int ch = 0; ch < NCH; ch++) {
        // rows CH (ch + 1) + 4 .. + CH + 3 travel while this chunk is summed (the last chunk re-reads its own rows: in range, unused)
        const float *nb = base + (size_t)((ch + 1 < NCH ? ch + 1 : ch) * CH + 4) * TILE;
#pragma unroll
        for (int i = 0; i < CH; i++) nxt[i] = nb[(size_t)i * TILE];
        // ac[k] += x[i] * x[i + k], i ascending: the reference's sequential sum per lag (pitch_xcorr's unrolling keeps that order)
#pragma unroll
        for (int j = 0; j < CH; j++)
#pragma unroll
            for (int k = 0; k < NK; k++) c[k] += cur[j] * cur[j + K0 + k];
        if (ch + 1 < NCH) {
#pragma unroll
            for (int i = 0; i < 4; i++) cur[i] = cur[CH + i];
#pragma unroll
            for (int i = 0; i < CH; i++) cur[4 + i] = nxt[i];
        }
    }
    // tail d_k = sum_{i = k + 860}^{863} x[i] x[i - k], added after the main sum; cur[] holds the last CH + 4 rows
#pragma unroll
    for (int kk = 0; kk < NK; kk++) {
        constexpr int O = XLP - CH - 4;
        const int k = K0 + kk;
        float d = 0.0f;
#pragma unroll
        for (int i = k + XLP - 4; i < XLP; i++) d += cur[i - O] * cur[i - k - O];
        ac[kk] = c[kk] + d;
    }
}

// lag window, Levinson recursion, bandwidth expansion, extra zero (ref: src/pitch.rs:460-480, 257-292) on a frame's five sums; the
// windowed autocorrelation and the FIR taps go to the frame's ring slot
__device__ __forceinline__ void lpc_finish(const Buffers &b, int tile, int lane, int slot, float (&ac)[5], float *taps = nullptr)
{
    ac[0] *= 1.0001f;
#pragma unroll
    for (int i = 1; i < 5; i++) ac[i] -= ac[i] * (0.008f * (float)i) * (0.008f * (float)i);
    float lpc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (ac[0] != 0.0f) {
        float error = ac[0];
        bool done = false;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (!done) {
                float rr = 0.0f;
#pragma unroll
                for (int j = 0; j < i; j++) rr += lpc[j] * ac[i - j];
                rr += ac[i + 1];
                float r = -rr / error;
                lpc[i] = r;
#pragma unroll
                for (int j = 0; j < (i + 1) / 2; j++) {
                    float t1 = lpc[j], t2 = lpc[i - 1 - j];
                    lpc[j] = t1 + r * t2;
                    lpc[i - 1 - j] = t2 + r * t1;
                }
                error = error - r * r * error;
                if (error < 0.001f * ac[0]) done = true;
            }
        }
    }
    float tmp = 1.0f;
#pragma unroll
    for (int i = 0; i < 4; i++) { tmp *= 0.9f; lpc[i] *= tmp; }
    float l2[5];
    l2[0] = lpc[0] + 0.8f;
    l2[1] = lpc[1] + 0.8f * lpc[0];
    l2[2] = lpc[2] + 0.8f * lpc[1];
    l2[3] = lpc[3] + 0.8f * lpc[2];
    l2[4] = 0.8f * lpc[3];
    float *o = NNN_TI(b.lpc, b.nslot * 10, tile, lane) + (size_t)(slot * 10) * TILE;
#pragma unroll
    for (int i = 0; i < 5; i++) { o[(size_t)i * TILE] = ac[i]; o[(size_t)(5 + i) * TILE] = l2[i]; }
    if (taps) {
#pragma unroll
        for (int i = 0; i < 5; i++) taps[i] = l2[i];
    }
}

// k_lpc's packed form.  One lag sum of a frame pair takes a product: MODE 1 the pair's first frame only, 2 the second only, 3 both;
// H = the half of `p` that holds the product.
template <int MODE, int H>
__device__ __forceinline__ void lpc_add(v2f &a, v2f p)
{
    if (MODE == 3) a = H ? pk_add_by(a, p) : pk_add_bx(a, p);
    else if (MODE == 1) a.x = sadd(a.x, H ? p.y : p.x);
    else a.y = sadd(a.y, H ? p.y : p.x);
}
// the chunk's LPC_CH rows (x[i] in aligned pairs, `first` in row 0's place) against rows i .. i + 4, into the five lag sums: ac[k] +=
// x[i] * x[i + k], i ascending (ref: src/pitch.rs:433-446)
template <int MODE, int NP>
__device__ __forceinline__ void lpc_rows(v2f (&acc)[5], const v2f (&rows)[NP], float first)
{
    v2f cur[LPC_CH / 2 + 2];
#pragma unroll
    for (int i = 0; i < LPC_CH / 2 + 2; i++) cur[i] = rows[i];
    cur[0].x = first;
#pragma unroll
    for (int m = 0; m < LPC_CH / 2; m++) {
        {   // row 2m: (p0, p1) (p2, p3) (p4, -)
            const v2f a = pk_mul_bx(cur[m], cur[m]), b = pk_mul_bx(cur[m], cur[m + 1]), c = pk_mul_bx(cur[m], cur[m + 2]);
            lpc_add<MODE, 0>(acc[0], a); lpc_add<MODE, 1>(acc[1], a); lpc_add<MODE, 0>(acc[2], b); lpc_add<MODE, 1>(acc[3], b); lpc_add<MODE, 0>(acc[4], c);
        }
        {   // row 2m + 1: (-, p0) (p1, p2) (p3, p4)
            const v2f a = pk_mul_by(cur[m], cur[m]), b = pk_mul_by(cur[m], cur[m + 1]), c = pk_mul_by(cur[m], cur[m + 2]);
            lpc_add<MODE, 1>(acc[0], a); lpc_add<MODE, 0>(acc[1], b); lpc_add<MODE, 1>(acc[2], b); lpc_add<MODE, 0>(acc[3], c); lpc_add<MODE, 1>(acc[4], c);
        }
    }
}
template <int MODE, int NP>
__device__ __forceinline__ void lpc_rows(v2f (&acc)[5], const v2f (&rows)[NP]) { lpc_rows<MODE>(acc, rows, rows[0].x); }
template <int NP>
__device__ __forceinline__ float lpc_cur(const v2f (&cur)[NP], int n) { return n & 1 ? cur[n >> 1].y : cur[n >> 1].x; }

// k_lpc: one wave per (tile, LPC_FC consecutive frames).  Consecutive frames' windows overlap by 624 of 864 rows, and frames of a
// tile running as separate waves do not find each other's rows in L2 (the few hundred waves an XCD has in flight read 16 MB of
// rows between two uses of a line: 3.4 KB per stream-frame from HBM).  Here a wave walks the union of its frames' windows once
// -- 864 + 240 per further frame rows -- and every row serves each frame whose window holds it: the same sums in the same order
// per frame, 2.7x fewer rows with eight frames per wave.
#ifndef NNN_LPC_FC_MAX
#define NNN_LPC_FC_MAX 8
#endif
constexpr int LPC_FC = NNN_LPC_FC_MAX;
static_assert(LPC_FC % 2 == 0, "k_lpc sums frames in pairs");
static_assert(240 % LPC_CH == 0, "");
// `fc` <= LPC_FC frames per wave: the host gives small launches fewer (more, shorter waves)
__global__ void __launch_bounds__(64) k_lpc(Buffers b, const StepParams *sp0, int g, int fc)
{
    const int lane = threadIdx.x;
    const int nch = (g + fc - 1) / fc;
    // block -> (tile, chunk of frames).  Workgroup i runs on XCD i mod 8 (observed; a speed matter only): tile t's chunks go to XCD
    // t mod 8, where k_hp's block t wrote the ring.
    int tile, chunk, sub_;
    xcd_tile_block_units((int)blockIdx.x, b.NT, 1, nch, chunk, tile, sub_);
    if (live_word(b, tile) == 0ull) return;   // (every stream of the tile held, nnn_batch_hold_streams: k_hp wrote nothing for it, k_pitch reads nothing)
    const int f0 = chunk * fc, nf = g - f0 < fc ? g - f0 : fc;
    const int nslot = b.nslot, ring = dec_ring_len(nslot);
    int slot[LPC_FC];
    float x0[LPC_FC];   // x_lp[0] of each frame is special (ref: src/pitch.rs:458)
#pragma unroll
    for (int c = 0; c < LPC_FC; c++) {
        slot[c] = sp0[f0 + (c < nf ? c : 0)].slot;
        x0[c] = NNN_TI(b.xlp0, nslot, tile, lane)[(size_t)slot[c] * TILE];
    }
    // union row r of the chunk sits at ring position (base0 + r) mod ring (consecutive frames' windows start 240 apart)
    const float *rows = b.dec + (size_t)tile * dec_len(nslot) * TILE + lane;
    const int base0 = dec_base(slot[0], nslot);
    auto row = [&](int r) {
        int p = base0 + r;
        p = p >= ring ? p - ring : p;
        return rows[(size_t)p * TILE];
    };
    constexpr int NCH = (XLP - 4) / LPC_CH, STEP = 240 / LPC_CH;   // chunks of a window (43), chunks between two windows (12)
    const int J = NCH + STEP * (nf - 1);
    // Rows in aligned register pairs, frames in pairs (acc[q][k] = lag k of frames 2q and 2q + 1): a row's five products are three packed
    // multiplies, and while both frames of a pair hold the row -- 31 of a window's 43 chunks -- one packed add serves both (the product
    // in both halves by operand selection).  Same products, same sums in the same order as lpc_chains above.  (The arithmetic is not what
    // paces this kernel -- the rows are: packed or not, 22.7 us per frame at 65536 streams with four frames per wave; the packed form's
    // registers let a wave take eight: 19.6, profiles/r5_experiments_ab.txt O.)
    constexpr int NP = (LPC_CH + 4) / 2;
    v2f cur[NP], nxt[LPC_CH / 2];
#pragma unroll
    for (int i = 0; i < NP; i++) cur[i] = v2f{row(2 * i), row(2 * i + 1)};
    v2f acc[LPC_FC / 2][5];
#pragma unroll
    for (int q = 0; q < LPC_FC / 2; q++)
#pragma unroll
        for (int k = 0; k < 5; k++) acc[q][k] = v2f{0.0f, 0.0f};
#pragma nounroll
    for (int j = 0; j < J; j++) {
        const int jn = j + 1 < J ? j + 1 : j;
#pragma unroll
        for (int i = 0; i < LPC_CH / 2; i++) nxt[i] = v2f{row(jn * LPC_CH + 4 + 2 * i), row(jn * LPC_CH + 5 + 2 * i)};
#pragma unroll
        for (int q = 0; q < LPC_FC / 2; q++) {
            const int jj0 = j - STEP * 2 * q, jj1 = jj0 - STEP;   // this chunk's place in the two frames' windows
            const bool a0 = 2 * q < nf && jj0 >= 0 && jj0 < NCH, a1 = 2 * q + 1 < nf && jj1 >= 0 && jj1 < NCH;
            if (a0 && a1 && jj1 != 0) lpc_rows<3>(acc[q], cur);
            else {
                // a window's first row is the frame's own x_lp[0] (ref: src/pitch.rs:458): that chunk on its own
                if (a0) lpc_rows<1>(acc[q], cur, jj0 == 0 ? x0[2 * q] : cur[0].x);
                if (a1) lpc_rows<2>(acc[q], cur, jj1 == 0 ? x0[2 * q + 1] : cur[0].x);
            }
#pragma unroll
            for (int h = 0; h < 2; h++)
                if ((h ? a1 : a0) && (h ? jj1 : jj0) == NCH - 1) {
                    // tail d_k = sum_{i = k + 860}^{863} x[i] x[i - k], added after the main sum; cur[] holds rows 840 .. 863 of the window
                    float ac[5];
#pragma unroll
                    for (int k = 0; k < 5; k++) {
                        constexpr int O = XLP - LPC_CH - 4;
                        float d = 0.0f;
#pragma unroll
                        for (int i = k + XLP - 4; i < XLP; i++) d += lpc_cur(cur, i - O) * lpc_cur(cur, i - k - O);
                        ac[k] = (h ? acc[q][k].y : acc[q][k].x) + d;
                    }
                    lpc_finish(b, tile, lane, slot[2 * q + h], ac);
                }
        }
        if (j + 1 < J) {
            cur[0] = cur[LPC_CH / 2];
            cur[1] = cur[LPC_CH / 2 + 1];
#pragma unroll
            for (int i = 0; i < LPC_CH / 2; i++) cur[2 + i] = nxt[i];
        }
    }
}

// k_lpc_wide, for launches too small to fill the GPU (a one-frame call on a few thousand streams is 64 waves walking five 860-step
// chains each): five waves per (tile, frame), one lag each, the five sums meeting in LDS.
__global__ void __launch_bounds__(320) k_lpc_wide(Buffers b, const StepParams *sp0, int g)
{
    __shared__ float acs[5][TILE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int tile, f, sub_;
    xcd_tile_block_units((int)blockIdx.x, b.NT, 1, g, f, tile, sub_);
    if (live_word(b, tile) == 0ull) return;   // (every stream of the tile held, as in k_lpc)
    const int slot = sp0[f].slot;
    const float *base = b.dec + ((size_t)tile * dec_len(b.nslot) + (size_t)dec_base(slot, b.nslot)) * TILE + lane;
    const float x0 = NNN_TI(b.xlp0, b.nslot, tile, lane)[(size_t)slot * TILE];   // x_lp[0] is special (ref: src/pitch.rs:458)
    float a1[1];
    if (wave == 0) lpc_chains<0, 1, LPC_CHW>(base, x0, a1);
    else if (wave == 1) lpc_chains<1, 1, LPC_CHW>(base, x0, a1);
    else if (wave == 2) lpc_chains<2, 1, LPC_CHW>(base, x0, a1);
    else if (wave == 3) lpc_chains<3, 1, LPC_CHW>(base, x0, a1);
    else lpc_chains<4, 1, LPC_CHW>(base, x0, a1);
    acs[wave][lane] = a1[0];
    __syncthreads();
    if (wave != 0) return;
    float ac[5];
#pragma unroll
    for (int k = 0; k < 5; k++) ac[k] = acs[k][lane];
    lpc_finish(b, tile, lane, slot, ac);
}

}  // namespace nnn
