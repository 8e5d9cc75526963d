// nnn_fit.hip -- the network trainer (include/nnn_fit.h): forward pass, loss, back-propagation through time and Adam
// for the reference's 3-GRU network over windows of consecutive training rows, and the quantisation into a .rnn file.
// Needs fail / HIPCHK / NNN_RT_LOCK (nnn_batch_core.hip) and nnn_model_parse (nnn_model.h).
// ref: train/rnn_train.py (network, loss, optimiser), train/dump_rnn.py (quantisation), src/rnn.rs:343-379 (wiring).
//
// A row is (t, s), row index t * S + s; every buffer of the object is dense [T][S][width] at the CALL's S and T, so nothing depends on
// the maxima beyond the size of the allocations.  The three GRUs run one after another over the whole window: a GRU's inputs are
// known for every t once the layers before it are done, so its input-side product is one row-parallel kernel (k_fit_proj) and only
// h U is left for the recurrence (k_fit_gru_fwd / k_fit_gru_bwd, one block per tile of FIT_TILE sequences, U resident in LDS).
// Gradients of the weights are reductions over rows with a fixed split (k_fit_wgrad into partial sums, k_fit_reduce over them in
// order): no floating-point atomics anywhere.
#pragma once

#include "../../include/nnn_fit.h"

constexpr int FIT_NP = NNN_FIT_PARAMS, FIT_TILE = NNN_FIT_TILE;
constexpr int FIT_NF = 42, FIT_ND = 24, FIT_NV = 24, FIT_NN = 48, FIT_NDN = 96, FIT_NG = 22, FIT_VCOL = 86;
constexpr int FIT_RB = 16;        // rows a block of the row-parallel kernels takes
constexpr int FIT_SPLITS = 64;    // the most row ranges a weight gradient is split into
constexpr int FIT_KT = 8;         // rows of a weight matrix one k_fit_wgrad block owns
constexpr int FIT_ROW_FLOATS = 2 * FIT_ND + 2 * FIT_NG + 2 + 8 * (FIT_NV + FIT_NN + FIT_NDN);
static_assert(FIT_ROW_FLOATS * 4 == NNN_FIT_ROW_BYTES, "");
enum { FIT_TANH = 0, FIT_SIGMOID = 1, FIT_RELU = 2, FIT_LINEAR = 3 };   // the .rnn header's codes (src/rnn.rs:138-140), and none

__device__ __forceinline__ float fit_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float fit_act(int a, float x)
{
    return a == FIT_TANH ? tanhf(x) : a == FIT_SIGMOID ? fit_sigmoid(x) : a == FIT_RELU ? fmaxf(x, 0.0f) : x;
}
// the activation's derivative from its VALUE y
__device__ __forceinline__ float fit_dact(int a, float y)
{
    return a == FIT_TANH ? 1.0f - y * y : a == FIT_SIGMOID ? y * (1.0f - y) : a == FIT_RELU ? (y > 0.0f ? 1.0f : 0.0f) : 1.0f;
}

// ---- inputs of a layer ------------------------------------------------------------------------------------------------------------------
// A layer's input is a concatenation of up to three sources that is never materialised: element k of row (t, s) is read from the
// source that holds it.  The caller's rows are one such source, with the caller's strides.
struct FitSeg { const float *p; long long ft, fs; int w; };
enum { FIT_IN_CONCAT = 0, FIT_IN_HPREV = 1, FIT_IN_RH = 2, FIT_IN_ONES = 3 };
struct FitIn {
    FitSeg seg[3];
    int nseg, K, mode;     // HPREV: seg[0] one step earlier (0 at t = 0); RH: that times r; ONES: 1 (the bias's "input")
    const float *r;        // [T][S][K]
};

__device__ __forceinline__ float fit_in(const FitIn &in, int t, int s, int S, int k)
{
    if (in.mode == FIT_IN_ONES) return 1.0f;
    if (in.mode != FIT_IN_CONCAT) {
        if (t == 0) return 0.0f;
        const float hp = in.seg[0].p[(long long)(t - 1) * in.seg[0].ft + (long long)s * in.seg[0].fs + k];
        return in.mode == FIT_IN_RH ? in.r[((long long)t * S + s) * in.K + k] * hp : hp;
    }
    int i = 0;
    while (i + 1 < in.nseg && k >= in.seg[i].w) k -= in.seg[i++].w;
    return in.seg[i].p[(long long)t * in.seg[i].ft + (long long)s * in.seg[i].fs + k];
}

// ---- k_fit_proj: out[row][j] = act(b[j] + sum_k in[row][k] W[k][j]) -------------------------------------------------------------------------
// A block takes FIT_RB rows: their inputs go through LDS once, thread j then owns column j (j, j + blockDim, ...) of all of them, so a
// weight is read once per FIT_RB rows (coalesced over j) and an input is an LDS broadcast.  k ascending, one FMA per term.
struct FitProjArgs {
    FitIn in;
    const float *W, *b;
    float *out;            // [N][ncols]
    int ncols, act, S, N;
};

__global__ void __launch_bounds__(256) k_fit_proj(FitProjArgs a)
{
    __shared__ float X[FIT_RB * 116];
    const int tid = threadIdx.x, bd = blockDim.x, K = a.in.K, row0 = blockIdx.x * FIT_RB;
    for (int i = tid; i < FIT_RB * K; i += bd) {
        const int r = i / K, k = i - r * K, row = row0 + r;
        X[i] = row < a.N ? fit_in(a.in, row / a.S, row % a.S, a.S, k) : 0.0f;
    }
    __syncthreads();
    for (int j = tid; j < a.ncols; j += bd) {
        float acc[FIT_RB];
        const float bj = a.b[j];
#pragma unroll
        for (int r = 0; r < FIT_RB; r++) acc[r] = bj;
        for (int k = 0; k < K; k++) {
            const float w = a.W[(size_t)k * a.ncols + j];
#pragma unroll
            for (int r = 0; r < FIT_RB; r++) acc[r] = fmaf(X[r * K + k], w, acc[r]);
        }
#pragma unroll
        for (int r = 0; r < FIT_RB; r++)
            if (row0 + r < a.N) a.out[(size_t)(row0 + r) * a.ncols + j] = fit_act(a.act, acc[r]);
    }
}

// ---- the recurrence -----------------------------------------------------------------------------------------------------------------------
// One block owns FIT_TILE sequences for the whole window; 2 n threads.  LDS: U [n][3n] (f32, 110.6 KB for the denoise GRU), h of the
// previous and of this step [2][TILE][n], r * h [TILE][n].  A step is two dependent products separated by a block barrier:
//   thread j < 2n: column j of  P[t] + h U(z | r)  for the tile's sequences -> z (kept by thread j < n) or r, r * h into LDS     | barrier
//   thread j < n:  column j of  P[t] + (r * h) U(c) -> c, h' = z h + (1 - z) c into the other h buffer                           | barrier
// A weight U[k][j] is one conflict-free LDS read (consecutive j) for TILE FMAs; h arrives four k at a time as a broadcast.  z, r, c and
// h' of every step are saved for the backward pass.  Padding sequences of a partial tile compute on zeros and store nothing.
struct FitGruArgs {
    const float *U;        // [n][3n]
    float *P;              // [T][S][3n]: forward: x W + b (read); backward: the three pre-activation deltas (written)
    float *Z, *R, *C, *H;  // [T][S][n]
    const float *GH;       // [T][S][n]: dL/dh[t] from the layers above (backward)
    int act, S, T;
};

template <int N> __global__ void __launch_bounds__(2 * N) k_fit_gru_fwd(FitGruArgs a)
{
    HIP_DYNAMIC_SHARED(float, fit_lds)
    constexpr int N3 = 3 * N;
    float *Us = fit_lds, *hb = Us + N * N3, *rh = hb + 2 * FIT_TILE * N;
    const int j = threadIdx.x, s0 = blockIdx.x * FIT_TILE;
    for (int i = j; i < N * N3; i += 2 * N) Us[i] = a.U[i];
    for (int i = j; i < 2 * FIT_TILE * N; i += 2 * N) hb[i] = 0.0f;
    __syncthreads();
    float z[FIT_TILE];
    int cur = 0;
#pragma nounroll
    for (int t = 0; t < a.T; t++) {
        const float *hc = hb + cur * FIT_TILE * N;
        float *hn = hb + (cur ^ 1) * FIT_TILE * N;
        const size_t row0 = (size_t)t * a.S + s0;
        float acc[FIT_TILE];
#pragma unroll
        for (int q = 0; q < FIT_TILE; q++) acc[q] = s0 + q < a.S ? a.P[(row0 + q) * N3 + j] : 0.0f;
        for (int k = 0; k < N; k += 4) {
            const float u0 = Us[k * N3 + j], u1 = Us[(k + 1) * N3 + j], u2 = Us[(k + 2) * N3 + j], u3 = Us[(k + 3) * N3 + j];
#pragma unroll
            for (int q = 0; q < FIT_TILE; q++) {
                const float4 h4 = *(const float4 *)(hc + q * N + k);
                acc[q] = fmaf(h4.w, u3, fmaf(h4.z, u2, fmaf(h4.y, u1, fmaf(h4.x, u0, acc[q]))));
            }
        }
#pragma unroll
        for (int q = 0; q < FIT_TILE; q++) {
            const float g = fit_sigmoid(acc[q]);
            if (j < N) {
                z[q] = g;
                if (s0 + q < a.S) a.Z[(row0 + q) * N + j] = g;
            } else {
                rh[q * N + j - N] = g * hc[q * N + j - N];
                if (s0 + q < a.S) a.R[(row0 + q) * N + j - N] = g;
            }
        }
        __syncthreads();
        if (j < N) {
#pragma unroll
            for (int q = 0; q < FIT_TILE; q++) acc[q] = s0 + q < a.S ? a.P[(row0 + q) * N3 + 2 * N + j] : 0.0f;
            for (int k = 0; k < N; k += 4) {
                const float u0 = Us[k * N3 + 2 * N + j], u1 = Us[(k + 1) * N3 + 2 * N + j], u2 = Us[(k + 2) * N3 + 2 * N + j],
                            u3 = Us[(k + 3) * N3 + 2 * N + j];
#pragma unroll
                for (int q = 0; q < FIT_TILE; q++) {
                    const float4 h4 = *(const float4 *)(rh + q * N + k);
                    acc[q] = fmaf(h4.w, u3, fmaf(h4.z, u2, fmaf(h4.y, u1, fmaf(h4.x, u0, acc[q]))));
                }
            }
#pragma unroll
            for (int q = 0; q < FIT_TILE; q++) {
                const float c = fit_act(a.act, acc[q]);
                const float hv = z[q] * hc[q * N + j] + (1.0f - z[q]) * c;
                hn[q * N + j] = hv;
                if (s0 + q < a.S) {
                    a.C[(row0 + q) * N + j] = c;
                    a.H[(row0 + q) * N + j] = hv;
                }
            }
        }
        __syncthreads();   // h' is there for the next step, and r * h and the old h have been read
        cur ^= 1;
    }
}

// The window in reverse, carrying dL/dh.  LDS: U transposed [3n][n] (thread k reads column k of a row: consecutive k, no conflicts),
// the step's deltas [TILE][3n], and the two halves of the recurrent part of dh for the step before [2][TILE][n].  Per step, with
// dh = GH[t] + (what step t + 1 left for h[t]):
//   thread k < n:   da_c = dh (1 - z) act'(c),  da_z = dh (h_prev - c) z (1 - z)                                                  | barrier
//   thread k < n:   d(rh) = sum_j da_c[j] Uc[k][j];  da_r = d(rh) h_prev r (1 - r);  keeps dh z + d(rh) r                         | barrier
//   thread (k, half): half 0 sums da_z[j] Uz[k][j], half 1 sums da_r[j] Ur[k][j] over j, into LDS                                 | barrier
// and the three deltas of the step go to memory (over P, which the forward pass is done with): nothing else is written.
template <int N> __global__ void __launch_bounds__(2 * N) k_fit_gru_bwd(FitGruArgs a)
{
    HIP_DYNAMIC_SHARED(float, fit_lds)
    constexpr int N3 = 3 * N;
    float *UT = fit_lds, *dA = UT + N * N3, *part = dA + FIT_TILE * N3;
    const int tid = threadIdx.x, s0 = blockIdx.x * FIT_TILE;
    for (int i = tid; i < N * N3; i += 2 * N) {
        const int jj = i / N, k = i - jj * N;
        UT[i] = a.U[k * N3 + jj];
    }
    for (int i = tid; i < 2 * FIT_TILE * N; i += 2 * N) part[i] = 0.0f;
    __syncthreads();
    const int half = tid / N, k = tid - half * N;
    float keep[FIT_TILE], hp[FIT_TILE];
#pragma unroll
    for (int q = 0; q < FIT_TILE; q++) keep[q] = 0.0f, hp[q] = 0.0f;
#pragma nounroll
    for (int t = a.T - 1; t >= 0; t--) {
        const size_t row0 = (size_t)t * a.S + s0;
        if (tid < N) {
#pragma unroll
            for (int q = 0; q < FIT_TILE; q++) {
                float daz = 0.0f, dac = 0.0f;
                const float carried = keep[q];   // what step t + 1 left for h[t], this thread's own part
                hp[q] = 0.0f, keep[q] = 0.0f;
                if (s0 + q < a.S) {
                    const size_t at = (row0 + q) * N + k;
                    const float dh = ((a.GH[at] + carried) + part[q * N + k]) + part[(FIT_TILE + q) * N + k];
                    const float z = a.Z[at], c = a.C[at];
                    hp[q] = t > 0 ? a.H[at - (size_t)a.S * N] : 0.0f;
                    dac = dh * (1.0f - z) * fit_dact(a.act, c);
                    daz = dh * (hp[q] - c) * (z * (1.0f - z));
                    keep[q] = dh * z;
                    a.P[(row0 + q) * N3 + k] = daz;
                    a.P[(row0 + q) * N3 + 2 * N + k] = dac;
                }
                dA[q * N3 + k] = daz;
                dA[q * N3 + 2 * N + k] = dac;
            }
        }
        __syncthreads();
        if (tid < N) {
            float acc[FIT_TILE];
#pragma unroll
            for (int q = 0; q < FIT_TILE; q++) acc[q] = 0.0f;
            for (int jj = 0; jj < N; jj += 4) {
                const float u0 = UT[(2 * N + jj) * N + k], u1 = UT[(2 * N + jj + 1) * N + k], u2 = UT[(2 * N + jj + 2) * N + k],
                            u3 = UT[(2 * N + jj + 3) * N + k];
#pragma unroll
                for (int q = 0; q < FIT_TILE; q++) {
                    const float4 d4 = *(const float4 *)(dA + q * N3 + 2 * N + jj);
                    acc[q] = fmaf(d4.w, u3, fmaf(d4.z, u2, fmaf(d4.y, u1, fmaf(d4.x, u0, acc[q]))));
                }
            }
#pragma unroll
            for (int q = 0; q < FIT_TILE; q++) {
                float dar = 0.0f;
                if (s0 + q < a.S) {
                    const float r = a.R[(row0 + q) * N + k];
                    dar = acc[q] * hp[q] * (r * (1.0f - r));
                    keep[q] = keep[q] + acc[q] * r;
                    a.P[(row0 + q) * N3 + N + k] = dar;
                }
                dA[q * N3 + N + k] = dar;
            }
        }
        __syncthreads();
        {
            float acc[FIT_TILE];
#pragma unroll
            for (int q = 0; q < FIT_TILE; q++) acc[q] = 0.0f;
            for (int jj = 0; jj < N; jj += 4) {
                const float u0 = UT[(half * N + jj) * N + k], u1 = UT[(half * N + jj + 1) * N + k], u2 = UT[(half * N + jj + 2) * N + k],
                            u3 = UT[(half * N + jj + 3) * N + k];
#pragma unroll
                for (int q = 0; q < FIT_TILE; q++) {
                    const float4 d4 = *(const float4 *)(dA + q * N3 + half * N + jj);
                    acc[q] = fmaf(d4.w, u3, fmaf(d4.z, u2, fmaf(d4.y, u1, fmaf(d4.x, u0, acc[q]))));
                }
            }
#pragma unroll
            for (int q = 0; q < FIT_TILE; q++) part[(half * FIT_TILE + q) * N + k] = acc[q];
        }
        __syncthreads();
    }
}

// ---- k_fit_loss: the loss terms of every row and dL/d(pre-activation) of the two output layers -----------------------------------------------
// thread = row.  The three sums over rows (w Lg, w Lv, w msse) are taken in f64: a tree over the block in LDS, one partial per block,
// and k_fit_loss_final adds the blocks in order.
struct FitLossArgs {
    FitSeg rows;           // the caller's rows (w: 87)
    const float *w;        // NULL or weights[t * wft + s * wfs]
    long long wft, wfs;
    const float *G, *PV;   // [N][22], [N]: the outputs
    float *dO, *dV;        // [N][22], [N]: dL/d(pre-activation); NULL: loss terms only
    double *part;          // [blocks][3]
    int S, N;
};

__global__ void __launch_bounds__(256) k_fit_loss(FitLossArgs a)
{
    __shared__ double red[3][256];
    const int tid = threadIdx.x, row = blockIdx.x * 256 + tid;
    // Keras' epsilon, applied in f32: hi = 1 - 2^-23.  From the f32 outputs on, a row's terms are taken in f64 and rounded once: the
    // logarithms of the clamped labels are the same few constants in every row, and an ulp of theirs would not average out over the rows.
    const float lo = 1e-7f, hi = 1.0f - 1e-7f;
    double Lg = 0.0, Lv = 0.0, ms = 0.0, wt = 0.0;
    if (row < a.N) {
        const int t = row / a.S, s = row - t * a.S;
        const float *x = a.rows.p + (long long)t * a.rows.ft + (long long)s * a.rows.fs;
        wt = a.w ? (double)a.w[(long long)t * a.wft + (long long)s * a.wfs] : 1.0;
        const double cg = 10.0 * wt / (double)a.N / 22.0, cv = 0.5 * wt / (double)a.N;
        for (int b = 0; b < FIT_NG; b++) {
            const float yf = x[FIT_NF + b];
            const double y = (double)yf, g = (double)a.G[(size_t)row * FIT_NG + b], yc = (double)fminf(fmaxf(yf, lo), hi);
            const double m = fmin(y + 1.0, 1.0);
            const double sg = sqrt(g), e = sg - sqrt(fmax(y, 0.0)), e2 = e * e;
            const double ly = log(yc), l1 = log(1.0 - yc);
            const double ce = -(g * ly + (1.0 - g) * l1);
            Lg += m * (10.0 * (e2 * e2) + e2 + 0.01 * ce);
            ms += m * e2;
            if (a.dO) {
                const double dg = m * ((40.0 * (e2 * e) + 2.0 * e) * (0.5 / sg) + 0.01 * (l1 - ly));
                a.dO[(size_t)row * FIT_NG + b] = (float)(cg * dg * (g * (1.0 - g)));
            }
        }
        Lg = Lg / 22.0, ms = ms / 22.0;
        const float vf = x[FIT_VCOL];
        const double v = (double)vf, p = (double)a.PV[row], vc = (double)fminf(fmaxf(vf, lo), hi);
        const double lv = log(vc), l1 = log(1.0 - vc), av = 2.0 * fabs(v - 0.5);
        Lv = av * -(p * lv + (1.0 - p) * l1);
        if (a.dV) a.dV[row] = (float)(cv * av * (l1 - lv) * (p * (1.0 - p)));
    }
    red[0][tid] = wt * Lg, red[1][tid] = wt * Lv, red[2][tid] = wt * ms;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st)
            for (int i = 0; i < 3; i++) red[i][tid] += red[i][tid + st];
        __syncthreads();
    }
    if (tid < 3) a.part[(size_t)blockIdx.x * 3 + tid] = red[tid][0];
}

// the input and recurrent matrices of the three GRUs: what the L2 term covers (train/rnn_train.py:67-73)
__device__ __forceinline__ bool fit_regularised(int i)
{
    return (i >= NNN_FIT_OFF_VAD_W && i < NNN_FIT_OFF_VAD_B) || (i >= NNN_FIT_OFF_NOISE_W && i < NNN_FIT_OFF_NOISE_B) ||
           (i >= NNN_FIT_OFF_DN_W && i < NNN_FIT_OFF_DN_B);
}

// one block: the blocks' partial sums in order, the L2 term (f64, fixed tree), and the five figures of nnn_fit_losses
__global__ void __launch_bounds__(256) k_fit_loss_final(const double *part, int nblk, const float *par, float reg, int N, float *out)
{
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double sq = 0.0;
    for (int i = NNN_FIT_OFF_VAD_W + tid; i < NNN_FIT_OFF_DN_B; i += 256)
        if (fit_regularised(i)) sq += (double)par[i] * (double)par[i];
    red[tid] = sq;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) red[tid] += red[tid + st];
        __syncthreads();
    }
    if (tid == 0) {
        double s[3] = {0.0, 0.0, 0.0};
        for (int b = 0; b < nblk; b++)
            for (int i = 0; i < 3; i++) s[i] += part[(size_t)b * 3 + i];
        const double lg = 10.0 * s[0] / N, lv = 0.5 * s[1] / N, lr = (double)reg * red[0];
        out[0] = (float)(lg + lv + lr), out[1] = (float)lg, out[2] = (float)lv, out[3] = (float)lr, out[4] = (float)(s[2] / N);
    }
}

// ---- k_fit_xgrad: gradients of a layer's inputs, out[row][k] (+)= sum_j D[row][j] W[k][j] -------------------------------------------------
// A block takes FIT_RB rows, whose deltas go through LDS; a thread owns one (row, k) at a time, consecutive threads consecutive k.
// `acc`: add to what out holds (a source that feeds several layers).  `act` >= 0: the source is a dense layer whose values are Y; the
// finished sum is multiplied by its activation's derivative and becomes that layer's delta.
struct FitXgradArgs {
    const float *D;        // [N][ncols]
    const float *W;        // first of the kn rows of the weight matrix that belong to this source, row stride ncols
    float *out;            // [N][kn]
    const float *Y;
    int ncols, kn, acc, act, N;
};

__global__ void __launch_bounds__(256) k_fit_xgrad(FitXgradArgs a)
{
    __shared__ float Dl[FIT_RB * 288];
    const int tid = threadIdx.x, row0 = blockIdx.x * FIT_RB, nr = a.N - row0 < FIT_RB ? a.N - row0 : FIT_RB;
    for (int i = tid; i < nr * a.ncols; i += 256) Dl[i] = a.D[(size_t)row0 * a.ncols + i];
    __syncthreads();
    for (int i = tid; i < nr * a.kn; i += 256) {
        const int r = i / a.kn, k = i - r * a.kn;
        const float *w = a.W + (size_t)k * a.ncols, *d = Dl + r * a.ncols;
        float sum = 0.0f;
        for (int j = 0; j < a.ncols; j++) sum = fmaf(d[j], w[j], sum);
        const size_t at = (size_t)(row0 + r) * a.kn + k;
        if (a.acc) sum = a.out[at] + sum;
        if (a.act >= 0) sum = sum * fit_dact(a.act, a.Y[at]);
        a.out[at] = sum;
    }
}

// ---- k_fit_wgrad / k_fit_reduce: dW[k][j] = sum over rows of A[row][k] D[row][j] -------------------------------------------------------------
// The rows are split into `gridDim.x` ranges of `rps` rows (a function of the call's row count alone).  Block (split, k tile): thread j
// owns column j of FIT_KT rows of the matrix; the range goes by in chunks of FIT_RB rows, A through LDS, D straight from memory
// (coalesced over j); a chunk is summed in f32 FMAs and the chunks in f64.  The partial sums go to part[split][the tensor's place in the
// parameter vector]; k_fit_reduce adds the splits in order (f64), adds the L2 term's 2 reg W and rounds once.
struct FitWgradArgs {
    FitIn A;
    const float *D;        // [N][dld], columns col0 .. col0 + nc - 1
    float *part;           // [splits][FIT_NP], already offset to the tensor
    int dld, col0, nc, ld; // ld: row stride of the tensor (its column col0 + j is D's)
    int S, N, rps;
};

__global__ void __launch_bounds__(320) k_fit_wgrad(FitWgradArgs a)
{
    __shared__ float As[FIT_RB * FIT_KT];
    const int j = threadIdx.x, bd = blockDim.x, k0 = blockIdx.y * FIT_KT, K = a.A.K;
    const int r0 = blockIdx.x * a.rps, r1 = r0 + a.rps < a.N ? r0 + a.rps : a.N;
    double accd[FIT_KT];
#pragma unroll
    for (int kk = 0; kk < FIT_KT; kk++) accd[kk] = 0.0;
    for (int c = r0; c < r1; c += FIT_RB) {
        __syncthreads();
        for (int i = j; i < FIT_RB * FIT_KT; i += bd) {
            const int r = i / FIT_KT, kk = i - r * FIT_KT, row = c + r;
            As[i] = row < r1 && k0 + kk < K ? fit_in(a.A, row / a.S, row % a.S, a.S, k0 + kk) : 0.0f;
        }
        __syncthreads();
        float acc[FIT_KT];
#pragma unroll
        for (int kk = 0; kk < FIT_KT; kk++) acc[kk] = 0.0f;
        for (int r = 0; r < FIT_RB && c + r < r1; r++) {
            const float d = j < a.nc ? a.D[(size_t)(c + r) * a.dld + a.col0 + j] : 0.0f;
#pragma unroll
            for (int kk = 0; kk < FIT_KT; kk++) acc[kk] = fmaf(As[r * FIT_KT + kk], d, acc[kk]);
        }
#pragma unroll
        for (int kk = 0; kk < FIT_KT; kk++) accd[kk] += (double)acc[kk];
    }
    if (j < a.nc)
        for (int kk = 0; kk < FIT_KT && k0 + kk < K; kk++)
            a.part[(size_t)blockIdx.x * FIT_NP + (size_t)(k0 + kk) * a.ld + a.col0 + j] = (float)accd[kk];
}

__global__ void __launch_bounds__(256) k_fit_reduce(const float *part, int nsplit, const float *par, float reg, float *grad)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= FIT_NP) return;
    double s = 0.0;
    for (int sp = 0; sp < nsplit; sp++) s += (double)part[(size_t)sp * FIT_NP + i];
    if (fit_regularised(i)) s += 2.0 * (double)reg * (double)par[i];
    grad[i] = (float)s;
}

// ---- k_fit_adam ---------------------------------------------------------------------------------------------------------------------------
// Adam as Keras runs it and the clip, per element in f32, every statement one IEEE operation (the build has -ffp-contract=off): bit for
// bit a NumPy float32 restatement given the same gradient.  omb1 = 1 - beta1 and omb2 = 1 - beta2 are f32 differences taken on the host.
__global__ void __launch_bounds__(256) k_fit_adam(float *par, float *m, float *v, const float *grad, float b1, float omb1, float b2, float omb2,
                                                  float lr_t, float eps, float clip)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= FIT_NP) return;
    const float g = grad[i];
    const float m1 = __fadd_rn(__fmul_rn(b1, m[i]), __fmul_rn(omb1, g));
    const float v1 = __fadd_rn(__fmul_rn(b2, v[i]), __fmul_rn(omb2, __fmul_rn(g, g)));
    const float den = __fadd_rn(sqrtf(v1), eps);
    const float upd = __fmul_rn(lr_t, m1) / den;
    float p = par[i] - upd;
    p = fminf(fmaxf(p, -clip), clip);
    m[i] = m1, v[i] = v1, par[i] = p;
}

// ---- the host side --------------------------------------------------------------------------------------------------------------------------
struct FitGruBufs { float *P, *Z, *R, *C, *H, *GH; };

struct nnn_fit {
    int device = 0, max_seq = 0, max_window = 0;
    nnn_fit_settings set = {1e-3f, 0.9f, 0.999f, 1e-7f, 1e-6f, 0.499f};
    uint8_t header[6][3];                       // the .rnn file's six layer headers: inputs, neurons, activation
    int act_d = 0, act_g[3] = {0, 0, 0};
    int64_t step = 0;
    bool have_grad = false;
    float *d_par = nullptr, *d_grad = nullptr, *d_m = nullptr, *d_v = nullptr;
    float *d_part = nullptr;                    // [FIT_SPLITS][FIT_NP]
    float *d_rowbuf = nullptr;                  // max_seq x max_window x FIT_ROW_FLOATS: carved per call (fit_carve)
    double *d_lpart = nullptr;                  // [loss blocks][3]
    float *d_loss = nullptr;                    // [5]
    hipStream_t own_stream = nullptr;
    hipEvent_t ev_last = nullptr;
    hipStream_t last_stream = nullptr;
    bool have_last = false;
    // device buffers of the host entry points (made on first use, grow only)
    float *h_rows = nullptr, *h_w = nullptr, *h_out = nullptr;
    size_t h_rows_cap = 0, h_w_cap = 0, h_out_cap = 0;
};

// the buffers of a call of N rows inside d_rowbuf
struct FitCarve {
    float *D, *dD, *G, *PV, *dO, *dV;
    FitGruBufs g[3];
};

static const int kFitN[3] = {FIT_NV, FIT_NN, FIT_NDN};
static const int kFitW[3] = {NNN_FIT_OFF_VAD_W, NNN_FIT_OFF_NOISE_W, NNN_FIT_OFF_DN_W};
static const int kFitU[3] = {NNN_FIT_OFF_VAD_U, NNN_FIT_OFF_NOISE_U, NNN_FIT_OFF_DN_U};
static const int kFitB[3] = {NNN_FIT_OFF_VAD_B, NNN_FIT_OFF_NOISE_B, NNN_FIT_OFF_DN_B};

static FitCarve fit_carve(const nnn_fit *f, size_t N)
{
    FitCarve c;
    float *p = f->d_rowbuf;
    auto take = [&](int width) { float *q = p; p += N * (size_t)width; return q; };
    c.D = take(FIT_ND), c.dD = take(FIT_ND), c.G = take(FIT_NG), c.dO = take(FIT_NG), c.PV = take(1), c.dV = take(1);
    for (int l = 0; l < 3; l++) {
        const int n = kFitN[l];
        c.g[l].P = take(3 * n), c.g[l].Z = take(n), c.g[l].R = take(n), c.g[l].C = take(n), c.g[l].H = take(n), c.g[l].GH = take(n);
    }
    return c;
}

static size_t fit_gru_lds(int n, bool backward)
{
    return sizeof(float) * ((size_t)n * 3 * n + (backward ? FIT_TILE * 3 * n + 2 * FIT_TILE * n : 3 * FIT_TILE * n));
}

static void fit_launch_gru(int layer, bool backward, const FitGruArgs &a, hipStream_t st)
{
    const unsigned blocks = (unsigned)((a.S + FIT_TILE - 1) / FIT_TILE);
    const size_t lds = fit_gru_lds(kFitN[layer], backward);
    if (layer == 0) {
        if (backward) hipLaunchKernelGGL(k_fit_gru_bwd<FIT_NV>, dim3(blocks), dim3(2 * FIT_NV), lds, st, a);
        else hipLaunchKernelGGL(k_fit_gru_fwd<FIT_NV>, dim3(blocks), dim3(2 * FIT_NV), lds, st, a);
    } else if (layer == 1) {
        if (backward) hipLaunchKernelGGL(k_fit_gru_bwd<FIT_NN>, dim3(blocks), dim3(2 * FIT_NN), lds, st, a);
        else hipLaunchKernelGGL(k_fit_gru_fwd<FIT_NN>, dim3(blocks), dim3(2 * FIT_NN), lds, st, a);
    } else {
        if (backward) hipLaunchKernelGGL(k_fit_gru_bwd<FIT_NDN>, dim3(blocks), dim3(2 * FIT_NDN), lds, st, a);
        else hipLaunchKernelGGL(k_fit_gru_fwd<FIT_NDN>, dim3(blocks), dim3(2 * FIT_NDN), lds, st, a);
    }
}

// the denoise GRU's kernels hold more LDS than a kernel may without asking: a per-device function attribute
static int fit_raise_lds()
{
    HIPCHK(hipFuncSetAttribute((const void *)k_fit_gru_fwd<FIT_NDN>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fit_gru_lds(FIT_NDN, false)));
    HIPCHK(hipFuncSetAttribute((const void *)k_fit_gru_bwd<FIT_NDN>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fit_gru_lds(FIT_NDN, true)));
    return 0;
}

extern "C" void nnn_fit_destroy(nnn_fit *f)
{
    if (!f) return;
    NNN_RT_LOCK;
    hipSetDevice(f->device);
    if (f->have_last) hipEventSynchronize(f->ev_last);
    if (f->own_stream) hipStreamSynchronize(f->own_stream);
    hipFree(f->d_par); hipFree(f->d_grad); hipFree(f->d_m); hipFree(f->d_v); hipFree(f->d_part); hipFree(f->d_rowbuf);
    hipFree(f->d_lpart); hipFree(f->d_loss); hipFree(f->h_rows); hipFree(f->h_w); hipFree(f->h_out);
    if (f->ev_last) hipEventDestroy(f->ev_last);
    if (f->own_stream) hipStreamDestroy(f->own_stream);
    delete f;
}

// the template's parameters / 256 in file order, or why it cannot be one
static int fit_read_template(nnn_fit *f, const uint8_t *bytes, size_t len, std::vector<float> &par)
{
    RNNModel *m = nnn_model_parse(bytes, len);
    if (!m) return fail("nnn_fit_create: malformed .rnn template");
    const NnnDense *dl[3] = {&m->input_dense, &m->denoise_output, &m->vad_output};
    const NnnGru *gl[3] = {&m->vad_gru, &m->noise_gru, &m->denoise_gru};
    const int want[6][2] = {{FIT_NF, FIT_ND}, {FIT_ND, FIT_NV}, {FIT_NF + FIT_ND + FIT_NV, FIT_NN}, {FIT_NF + FIT_NV + FIT_NN, FIT_NDN}, {FIT_NDN, FIT_NG}, {FIT_NV, 1}};
    const int got[6][3] = {{dl[0]->nb_inputs, dl[0]->nb_neurons, dl[0]->activation}, {gl[0]->nb_inputs, gl[0]->nb_neurons, gl[0]->activation},
                           {gl[1]->nb_inputs, gl[1]->nb_neurons, gl[1]->activation}, {gl[2]->nb_inputs, gl[2]->nb_neurons, gl[2]->activation},
                           {dl[1]->nb_inputs, dl[1]->nb_neurons, dl[1]->activation}, {dl[2]->nb_inputs, dl[2]->nb_neurons, dl[2]->activation}};
    int rc = 0;
    for (int l = 0; l < 6 && !rc; l++)
        if (got[l][0] != want[l][0] || got[l][1] != want[l][1])
            rc = fail("nnn_fit_create: layer %d of the template is %d -> %d; the trainer handles the reference's shape only (42-24, 24-24, 90-48, 114-96, 96-22, 24-1)",
                      l, got[l][0], got[l][1]);
    if (!rc && (got[4][2] != FIT_SIGMOID || got[5][2] != FIT_SIGMOID))
        rc = fail("nnn_fit_create: the template's output layers must be sigmoid (the loss takes the square root of the output)");
    if (!rc) {
        for (int l = 0; l < 6; l++)
            for (int i = 0; i < 3; i++) f->header[l][i] = (uint8_t)got[l][i];
        const int8_t *b = m->blob.data();
        auto put = [&](size_t ofs, size_t n) { for (size_t i = 0; i < n; i++) par.push_back((float)b[ofs + i] / 256.0f); };
        put(dl[0]->weights, FIT_NF * FIT_ND), put(dl[0]->bias, FIT_ND);
        for (int l = 0; l < 3; l++) {
            const size_t n = (size_t)gl[l]->nb_neurons;
            put(gl[l]->weights, 3 * n * gl[l]->nb_inputs), put(gl[l]->rec, 3 * n * n), put(gl[l]->bias, 3 * n);
        }
        put(dl[1]->weights, FIT_NDN * FIT_NG), put(dl[1]->bias, FIT_NG), put(dl[2]->weights, FIT_NV), put(dl[2]->bias, 1);
        if (par.size() != (size_t)FIT_NP) rc = fail("nnn_fit_create: the template holds %zu parameters, not %d", par.size(), FIT_NP);
    }
    delete m;
    return rc;
}

extern "C" nnn_fit *nnn_fit_create(const uint8_t *rnn_bytes, size_t len, int max_seq, int max_window, int device)
{
    if (max_seq < 1 || max_window < 1) { fail("nnn_fit_create: max_seq = %d, max_window = %d", max_seq, max_window); return nullptr; }
    if ((double)max_seq * (double)max_window > 1e9) { fail("nnn_fit_create: %d x %d rows are more than a call holds", max_seq, max_window); return nullptr; }
    nnn_fit *f = new nnn_fit();
    f->device = device, f->max_seq = max_seq, f->max_window = max_window;
    std::vector<float> par;
    if (rnn_bytes) {
        if (fit_read_template(f, rnn_bytes, len, par)) { delete f; return nullptr; }
    } else {   // train/rnn_train.py:66-75
        const uint8_t h[6][3] = {{42, 24, FIT_TANH}, {24, 24, FIT_TANH}, {90, 48, FIT_RELU}, {114, 96, FIT_TANH}, {96, 22, FIT_SIGMOID}, {24, 1, FIT_SIGMOID}};
        memcpy(f->header, h, sizeof(h));
        par.assign((size_t)FIT_NP, 0.0f);
    }
    f->act_d = f->header[0][2];
    for (int l = 0; l < 3; l++) f->act_g[l] = f->header[1 + l][2];
    NNN_RT_LOCK;
    if (hipSetDevice(device) != hipSuccess) { fail("nnn_fit_create: no such HIP device"); delete f; return nullptr; }
    const size_t rows = (size_t)max_seq * max_window, lblocks = (rows + 255) / 256;
    bool ok = true;
    auto dev = [&](auto **q, size_t bytes) { ok = ok && hipMalloc((void **)q, bytes) == hipSuccess && hipMemset(*q, 0, bytes) == hipSuccess; };
    dev(&f->d_par, FIT_NP * sizeof(float)), dev(&f->d_grad, FIT_NP * sizeof(float)), dev(&f->d_m, FIT_NP * sizeof(float)), dev(&f->d_v, FIT_NP * sizeof(float));
    dev(&f->d_part, (size_t)FIT_SPLITS * FIT_NP * sizeof(float));
    dev(&f->d_rowbuf, rows * FIT_ROW_FLOATS * sizeof(float));
    dev(&f->d_lpart, lblocks * 3 * sizeof(double));
    dev(&f->d_loss, 5 * sizeof(float));
    ok = ok && hipMemcpy(f->d_par, par.data(), FIT_NP * sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipStreamCreateWithFlags(&f->own_stream, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&f->ev_last, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipDeviceSynchronize() == hipSuccess;   // (the memsets above are on the legacy stream; the calls are on non-blocking ones)
    if (!ok) {
        nnn_fit_destroy(f);
        fail("nnn_fit_create: allocation failed (the saved activations are %d bytes for each of %d x %d rows)", NNN_FIT_ROW_BYTES, max_seq, max_window);
        return nullptr;
    }
    if (fit_raise_lds()) { nnn_fit_destroy(f); return nullptr; }
    return f;
}

// everything enqueued so far is done
static int fit_drain(nnn_fit *f)
{
    HIPCHK(hipSetDevice(f->device));
    if (f->have_last) HIPCHK(hipEventSynchronize(f->ev_last));
    return 0;
}

static float *fit_select(nnn_fit *f, int which)
{
    return which == NNN_FIT_SEL_PARAMS ? f->d_par : which == NNN_FIT_SEL_GRAD ? f->d_grad : which == NNN_FIT_SEL_ADAM_M ? f->d_m : which == NNN_FIT_SEL_ADAM_V ? f->d_v : nullptr;
}

extern "C" int nnn_fit_get(nnn_fit *f, int which, float *out)
{
    if (!f) return fail("null trainer");
    if (!out) return fail("nnn_fit_get: null buffer");
    float *src = fit_select(f, which);
    if (!src) return fail("nnn_fit_get: selector %d is none of NNN_FIT_SEL_*", which);
    NNN_RT_LOCK;
    if (int rc = fit_drain(f)) return rc;
    HIPCHK(hipMemcpy(out, src, FIT_NP * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int nnn_fit_set(nnn_fit *f, int which, const float *in)
{
    if (!f) return fail("null trainer");
    if (!in) return fail("nnn_fit_set: null buffer");
    if (which == NNN_FIT_SEL_GRAD) return fail("nnn_fit_set: the gradient is the trainer's own (nnn_fit_grad_*); it cannot be set");
    float *dst = fit_select(f, which);
    if (!dst) return fail("nnn_fit_set: selector %d is none of NNN_FIT_SEL_*", which);
    for (int i = 0; i < FIT_NP; i++)
        if (!std::isfinite(in[i])) return fail("nnn_fit_set: value %d is not finite", i);
    NNN_RT_LOCK;
    if (int rc = fit_drain(f)) return rc;
    HIPCHK(hipMemcpy(dst, in, FIT_NP * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

extern "C" int nnn_fit_get_step(nnn_fit *f, int64_t *step)
{
    if (!f || !step) return fail("nnn_fit_get_step: null %s", f ? "pointer" : "trainer");
    *step = f->step;
    return 0;
}

extern "C" int nnn_fit_set_step(nnn_fit *f, int64_t step)
{
    if (!f) return fail("null trainer");
    if (step < 0) return fail("nnn_fit_set_step: step = %lld", (long long)step);
    f->step = step;
    return 0;
}

extern "C" int nnn_fit_get_settings(nnn_fit *f, nnn_fit_settings *s)
{
    if (!f || !s) return fail("nnn_fit_get_settings: null %s", f ? "pointer" : "trainer");
    *s = f->set;
    return 0;
}

extern "C" int nnn_fit_set_settings(nnn_fit *f, const nnn_fit_settings *s)
{
    if (!f || !s) return fail("nnn_fit_set_settings: null %s", f ? "pointer" : "trainer");
    const float v[6] = {s->lr, s->beta1, s->beta2, s->epsilon, s->reg, s->clip};
    for (float x : v)
        if (!std::isfinite(x) || x < 0.0f) return fail("nnn_fit_set_settings: a setting is negative or not finite");
    if (s->beta1 >= 1.0f || s->beta2 >= 1.0f) return fail("nnn_fit_set_settings: beta1 and beta2 must be below 1");
    f->set = *s;
    return 0;
}

extern "C" int nnn_fit_export_rnn(nnn_fit *f, uint8_t *out, size_t cap)
{
    if (!f) return fail("null trainer");
    if (!out || cap < (size_t)NNN_FIT_RNN_BYTES) return fail("nnn_fit_export_rnn: the file is %d bytes", NNN_FIT_RNN_BYTES);
    std::vector<float> par((size_t)FIT_NP);
    if (int rc = nnn_fit_get(f, NNN_FIT_SEL_PARAMS, par.data())) return rc;
    for (int i = 0; i < FIT_NP; i++)
        if (!std::isfinite(par[i])) return fail("nnn_fit_export_rnn: parameter %d is not finite", i);
    const int first[7] = {NNN_FIT_OFF_IN_W, NNN_FIT_OFF_VAD_W, NNN_FIT_OFF_NOISE_W, NNN_FIT_OFF_DN_W, NNN_FIT_OFF_OUT_W, NNN_FIT_OFF_VOUT_W, FIT_NP};
    uint8_t *q = out;
    for (int l = 0; l < 6; l++) {
        for (int i = 0; i < 3; i++) *q++ = f->header[l][i];
        for (int i = first[l]; i < first[l + 1]; i++) {
            float y = nearbyintf(256.0f * par[i]);   // (256 x is exact; the default rounding mode is to nearest even, Python's round)
            y = y < -128.0f ? -128.0f : y > 127.0f ? 127.0f : y;
            *q++ = (uint8_t)(int8_t)(int)y;
        }
    }
    return 0;
}

// what every call checks before anything is enqueued, and the stream it runs on
static int fit_begin(nnn_fit *f, const nnn_fit_rows *r, void *hip_stream, const char *who, hipStream_t *st)
{
    if (!r || !r->rows) return fail("%s: null rows", who);
    if (r->n_seq < 1 || r->n_seq > f->max_seq) return fail("%s: n_seq = %d outside [1, %d]", who, r->n_seq, f->max_seq);
    if (r->window < 1 || r->window > f->max_window) return fail("%s: window = %d outside [1, %d]", who, r->window, f->max_window);
    HIPCHK(hipSetDevice(f->device));
    *st = hip_stream ? (hipStream_t)hip_stream : f->own_stream;
    if (f->have_last && f->last_stream != *st) HIPCHK(hipStreamWaitEvent(*st, f->ev_last, 0));   // (the buffers are the previous call's until then)
    return 0;
}

static int fit_end(nnn_fit *f, hipStream_t st)
{
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(f->ev_last, st));
    f->last_stream = st;
    f->have_last = true;
    return 0;
}

static FitSeg fit_seg(const float *p, int S, int w) { return FitSeg{p, (long long)S * w, (long long)w, w}; }

static FitIn fit_concat(std::initializer_list<FitSeg> segs)
{
    FitIn in = {};
    in.mode = FIT_IN_CONCAT;
    for (const FitSeg &s : segs) in.seg[in.nseg++] = s, in.K += s.w;
    return in;
}

static void fit_proj(hipStream_t st, const FitIn &in, const float *W, const float *b, float *out, int ncols, int act, int S, int N)
{
    FitProjArgs a = {in, W, b, out, ncols, act, S, N};
    const int threads = ncols >= 256 ? 256 : (ncols + 63) / 64 * 64;
    hipLaunchKernelGGL(k_fit_proj, dim3((unsigned)((N + FIT_RB - 1) / FIT_RB)), dim3((unsigned)threads), 0, st, a);
}

// the three GRUs' inputs (src/rnn.rs:356-371)
static FitIn fit_gru_input(int l, const FitCarve &c, const FitSeg &feat, int S)
{
    if (l == 0) return fit_concat({fit_seg(c.D, S, FIT_ND)});
    if (l == 1) return fit_concat({fit_seg(c.D, S, FIT_ND), fit_seg(c.g[0].H, S, FIT_NV), feat});
    return fit_concat({fit_seg(c.g[0].H, S, FIT_NV), fit_seg(c.g[1].H, S, FIT_NN), feat});
}

static FitGruArgs fit_gru_args(const nnn_fit *f, int l, const FitCarve &c, int S, int T)
{
    FitGruArgs a = {f->d_par + kFitU[l], c.g[l].P, c.g[l].Z, c.g[l].R, c.g[l].C, c.g[l].H, c.g[l].GH, f->act_g[l], S, T};
    return a;
}

static void fit_forward(nnn_fit *f, const nnn_fit_rows *r, const FitCarve &c, float *gains, float *vad, hipStream_t st)
{
    const int S = r->n_seq, T = r->window, N = S * T;
    const float *par = f->d_par;
    const FitSeg feat = {r->rows, (long long)r->frame_stride, (long long)r->seq_stride, FIT_NF};
    fit_proj(st, fit_concat({feat}), par + NNN_FIT_OFF_IN_W, par + NNN_FIT_OFF_IN_B, c.D, FIT_ND, f->act_d, S, N);
    for (int l = 0; l < 3; l++) {
        fit_proj(st, fit_gru_input(l, c, feat, S), par + kFitW[l], par + kFitB[l], c.g[l].P, 3 * kFitN[l], FIT_LINEAR, S, N);
        fit_launch_gru(l, false, fit_gru_args(f, l, c, S, T), st);
    }
    fit_proj(st, fit_concat({fit_seg(c.g[2].H, S, FIT_NDN)}), par + NNN_FIT_OFF_OUT_W, par + NNN_FIT_OFF_OUT_B, gains, FIT_NG, FIT_SIGMOID, S, N);
    fit_proj(st, fit_concat({fit_seg(c.g[0].H, S, FIT_NV)}), par + NNN_FIT_OFF_VOUT_W, par + NNN_FIT_OFF_VOUT_B, vad, 1, FIT_SIGMOID, S, N);
}

static void fit_loss(nnn_fit *f, const nnn_fit_rows *r, const FitCarve &c, bool deltas, hipStream_t st)
{
    const int S = r->n_seq, N = S * r->window, blocks = (N + 255) / 256;
    FitLossArgs a = {};
    a.rows = FitSeg{r->rows, (long long)r->frame_stride, (long long)r->seq_stride, NNN_FIT_ROW};
    a.w = r->w, a.wft = (long long)r->w_frame_stride, a.wfs = (long long)r->w_seq_stride;
    a.G = c.G, a.PV = c.PV, a.dO = deltas ? c.dO : nullptr, a.dV = deltas ? c.dV : nullptr;
    a.part = f->d_lpart, a.S = S, a.N = N;
    hipLaunchKernelGGL(k_fit_loss, dim3((unsigned)blocks), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_fit_loss_final, dim3(1), dim3(256), 0, st, (const double *)f->d_lpart, blocks, (const float *)f->d_par, f->set.reg, N, f->d_loss);
}

static void fit_xgrad(hipStream_t st, const float *D, int ncols, const float *W, int kn, float *out, bool acc, int act, const float *Y, int N)
{
    FitXgradArgs a = {D, W, out, Y, ncols, kn, acc ? 1 : 0, act, N};
    hipLaunchKernelGGL(k_fit_xgrad, dim3((unsigned)((N + FIT_RB - 1) / FIT_RB)), dim3(256), 0, st, a);
}

// the split of a call's rows: ranges of a whole number of chunks, at most FIT_SPLITS of them
static void fit_split(int N, int *nsplit, int *rps)
{
    const int chunks = (N + FIT_RB - 1) / FIT_RB, per = (chunks + FIT_SPLITS - 1) / FIT_SPLITS;
    *rps = per * FIT_RB;
    *nsplit = (N + *rps - 1) / *rps;
}

static void fit_wgrad(nnn_fit *f, hipStream_t st, const FitIn &A, const float *D, int dld, int col0, int nc, int off, int ld, int S, int N)
{
    FitWgradArgs a = {};
    a.A = A, a.D = D, a.part = f->d_part + off, a.dld = dld, a.col0 = col0, a.nc = nc, a.ld = ld, a.S = S, a.N = N;
    int nsplit;
    fit_split(N, &nsplit, &a.rps);
    const int threads = nc <= 128 ? 128 : (nc + 63) / 64 * 64;
    hipLaunchKernelGGL(k_fit_wgrad, dim3((unsigned)nsplit, (unsigned)((A.K + FIT_KT - 1) / FIT_KT)), dim3((unsigned)threads), 0, st, a);
}

static FitIn fit_ones()
{
    FitIn in = {};
    in.mode = FIT_IN_ONES, in.K = 1;
    return in;
}

static void fit_backward(nnn_fit *f, const nnn_fit_rows *r, const FitCarve &c, hipStream_t st)
{
    const int S = r->n_seq, T = r->window, N = S * T;
    const float *par = f->d_par;
    const FitSeg feat = {r->rows, (long long)r->frame_stride, (long long)r->seq_stride, FIT_NF};
    const FitGruBufs &gv = c.g[0], &gn = c.g[1], &gd = c.g[2];
    // dL/dh of the three GRUs from the layers above them, top down; a GRU's backward pass turns P into its deltas
    fit_xgrad(st, c.dO, FIT_NG, par + NNN_FIT_OFF_OUT_W, FIT_NDN, gd.GH, false, -1, nullptr, N);
    fit_xgrad(st, c.dV, 1, par + NNN_FIT_OFF_VOUT_W, FIT_NV, gv.GH, false, -1, nullptr, N);
    fit_launch_gru(2, true, fit_gru_args(f, 2, c, S, T), st);
    fit_xgrad(st, gd.P, 3 * FIT_NDN, par + NNN_FIT_OFF_DN_W, FIT_NV, gv.GH, true, -1, nullptr, N);                              // denoise input = [vad | noise | features]
    fit_xgrad(st, gd.P, 3 * FIT_NDN, par + NNN_FIT_OFF_DN_W + FIT_NV * 3 * FIT_NDN, FIT_NN, gn.GH, false, -1, nullptr, N);
    fit_launch_gru(1, true, fit_gru_args(f, 1, c, S, T), st);
    fit_xgrad(st, gn.P, 3 * FIT_NN, par + NNN_FIT_OFF_NOISE_W, FIT_ND, c.dD, false, -1, nullptr, N);                            // noise input = [dense | vad | features]
    fit_xgrad(st, gn.P, 3 * FIT_NN, par + NNN_FIT_OFF_NOISE_W + FIT_ND * 3 * FIT_NN, FIT_NV, gv.GH, true, -1, nullptr, N);
    fit_launch_gru(0, true, fit_gru_args(f, 0, c, S, T), st);
    fit_xgrad(st, gv.P, 3 * FIT_NV, par + NNN_FIT_OFF_VAD_W, FIT_ND, c.dD, true, f->act_d, c.D, N);                             // -> the input dense layer's delta
    // the fifteen tensors
    fit_wgrad(f, st, fit_concat({feat}), c.dD, FIT_ND, 0, FIT_ND, NNN_FIT_OFF_IN_W, FIT_ND, S, N);
    fit_wgrad(f, st, fit_ones(), c.dD, FIT_ND, 0, FIT_ND, NNN_FIT_OFF_IN_B, FIT_ND, S, N);
    for (int l = 0; l < 3; l++) {
        const int n = kFitN[l], n3 = 3 * n;
        FitIn hprev = fit_concat({fit_seg(c.g[l].H, S, n)});
        hprev.mode = FIT_IN_HPREV;
        FitIn rhp = hprev;
        rhp.mode = FIT_IN_RH, rhp.r = c.g[l].R;
        fit_wgrad(f, st, fit_gru_input(l, c, feat, S), c.g[l].P, n3, 0, n3, kFitW[l], n3, S, N);
        fit_wgrad(f, st, hprev, c.g[l].P, n3, 0, 2 * n, kFitU[l], n3, S, N);
        fit_wgrad(f, st, rhp, c.g[l].P, n3, 2 * n, n, kFitU[l], n3, S, N);
        fit_wgrad(f, st, fit_ones(), c.g[l].P, n3, 0, n3, kFitB[l], n3, S, N);
    }
    fit_wgrad(f, st, fit_concat({fit_seg(gd.H, S, FIT_NDN)}), c.dO, FIT_NG, 0, FIT_NG, NNN_FIT_OFF_OUT_W, FIT_NG, S, N);
    fit_wgrad(f, st, fit_ones(), c.dO, FIT_NG, 0, FIT_NG, NNN_FIT_OFF_OUT_B, FIT_NG, S, N);
    fit_wgrad(f, st, fit_concat({fit_seg(gv.H, S, FIT_NV)}), c.dV, 1, 0, 1, NNN_FIT_OFF_VOUT_W, 1, S, N);
    fit_wgrad(f, st, fit_ones(), c.dV, 1, 0, 1, NNN_FIT_OFF_VOUT_B, 1, S, N);
    int nsplit, rps;
    fit_split(N, &nsplit, &rps);
    hipLaunchKernelGGL(k_fit_reduce, dim3((FIT_NP + 255) / 256), dim3(256), 0, st, (const float *)f->d_part, nsplit, par, f->set.reg, f->d_grad);
}

extern "C" int nnn_fit_forward_device(nnn_fit *f, const nnn_fit_rows *r, float *d_gains, float *d_vad, void *hip_stream)
{
    if (!f) return fail("null trainer");
    hipStream_t st;
    if (int rc = fit_begin(f, r, hip_stream, "nnn_fit_forward", &st)) return rc;
    if (!d_gains || !d_vad) return fail("nnn_fit_forward: null output");
    fit_forward(f, r, fit_carve(f, (size_t)r->n_seq * r->window), d_gains, d_vad, st);
    return fit_end(f, st);
}

extern "C" int nnn_fit_loss_device(nnn_fit *f, const nnn_fit_rows *r, void *hip_stream)
{
    if (!f) return fail("null trainer");
    hipStream_t st;
    if (int rc = fit_begin(f, r, hip_stream, "nnn_fit_loss", &st)) return rc;
    const FitCarve c = fit_carve(f, (size_t)r->n_seq * r->window);
    fit_forward(f, r, c, c.G, c.PV, st);
    fit_loss(f, r, c, false, st);
    return fit_end(f, st);
}

extern "C" int nnn_fit_grad_device(nnn_fit *f, const nnn_fit_rows *r, void *hip_stream)
{
    if (!f) return fail("null trainer");
    hipStream_t st;
    if (int rc = fit_begin(f, r, hip_stream, "nnn_fit_grad", &st)) return rc;
    const FitCarve c = fit_carve(f, (size_t)r->n_seq * r->window);
    fit_forward(f, r, c, c.G, c.PV, st);
    fit_loss(f, r, c, true, st);
    fit_backward(f, r, c, st);
    f->have_grad = true;
    return fit_end(f, st);
}

extern "C" int nnn_fit_step(nnn_fit *f, void *hip_stream)
{
    if (!f) return fail("null trainer");
    if (!f->have_grad) return fail("nnn_fit_step: no gradient yet (nnn_fit_grad_* comes first)");
    HIPCHK(hipSetDevice(f->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : f->own_stream;
    if (f->have_last && f->last_stream != st) HIPCHK(hipStreamWaitEvent(st, f->ev_last, 0));
    const nnn_fit_settings &s = f->set;
    const double t = (double)++f->step;
    const float lr_t = (float)((double)s.lr * sqrt(1.0 - pow((double)s.beta2, t)) / (1.0 - pow((double)s.beta1, t)));
    hipLaunchKernelGGL(k_fit_adam, dim3((FIT_NP + 255) / 256), dim3(256), 0, st, f->d_par, f->d_m, f->d_v, (const float *)f->d_grad, s.beta1, 1.0f - s.beta1,
                       s.beta2, 1.0f - s.beta2, lr_t, s.epsilon, s.clip);
    return fit_end(f, st);
}

extern "C" int nnn_fit_losses(nnn_fit *f, float out[5])
{
    if (!f) return fail("null trainer");
    if (!out) return fail("nnn_fit_losses: null buffer");
    NNN_RT_LOCK;
    if (int rc = fit_drain(f)) return rc;
    HIPCHK(hipMemcpy(out, f->d_loss, 5 * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

static int fit_room(nnn_fit *f, float *&q, size_t &cap, size_t bytes)
{
    if (bytes <= cap) return 0;
    NNN_RT_LOCK;
    if (int rc = fit_drain(f)) return rc;
    HIPCHK(hipFree(q));
    q = nullptr, cap = 0;
    HIPCHK(hipMalloc((void **)&q, bytes));
    cap = bytes;
    return 0;
}

// the host entry points' rows (and weights) on the device, dense [window][n_seq][87]
static int fit_upload(nnn_fit *f, const float *rows, const float *w, int n_seq, int window, const char *who, nnn_fit_rows *r)
{
    if (!rows) return fail("%s: null rows", who);
    if (n_seq < 1 || n_seq > f->max_seq) return fail("%s: n_seq = %d outside [1, %d]", who, n_seq, f->max_seq);
    if (window < 1 || window > f->max_window) return fail("%s: window = %d outside [1, %d]", who, window, f->max_window);
    const size_t N = (size_t)n_seq * window;
    HIPCHK(hipSetDevice(f->device));
    if (int rc = fit_room(f, f->h_rows, f->h_rows_cap, N * NNN_FIT_ROW * sizeof(float))) return rc;
    if (w)
        if (int rc = fit_room(f, f->h_w, f->h_w_cap, N * sizeof(float))) return rc;
    if (f->have_last && f->last_stream != f->own_stream) HIPCHK(hipStreamWaitEvent(f->own_stream, f->ev_last, 0));
    HIPCHK(hipMemcpyAsync(f->h_rows, rows, N * NNN_FIT_ROW * sizeof(float), hipMemcpyHostToDevice, f->own_stream));
    if (w) HIPCHK(hipMemcpyAsync(f->h_w, w, N * sizeof(float), hipMemcpyHostToDevice, f->own_stream));
    *r = nnn_fit_rows{f->h_rows, (size_t)n_seq * NNN_FIT_ROW, (size_t)NNN_FIT_ROW, w ? f->h_w : nullptr, (size_t)n_seq, 1, n_seq, window};
    return 0;
}

extern "C" int nnn_fit_forward_host(nnn_fit *f, const float *rows, int n_seq, int window, float *gains, float *vad)
{
    if (!f) return fail("null trainer");
    if (!gains || !vad) return fail("nnn_fit_forward: null output");
    nnn_fit_rows r;
    if (int rc = fit_upload(f, rows, nullptr, n_seq, window, "nnn_fit_forward", &r)) return rc;
    const size_t N = (size_t)n_seq * window;
    if (int rc = fit_room(f, f->h_out, f->h_out_cap, N * (FIT_NG + 1) * sizeof(float))) return rc;
    if (int rc = nnn_fit_forward_device(f, &r, f->h_out, f->h_out + N * FIT_NG, f->own_stream)) return rc;
    HIPCHK(hipMemcpyAsync(gains, f->h_out, N * FIT_NG * sizeof(float), hipMemcpyDeviceToHost, f->own_stream));
    HIPCHK(hipMemcpyAsync(vad, f->h_out + N * FIT_NG, N * sizeof(float), hipMemcpyDeviceToHost, f->own_stream));
    HIPCHK(hipStreamSynchronize(f->own_stream));
    return 0;
}

extern "C" int nnn_fit_loss_host(nnn_fit *f, const float *rows, const float *w, int n_seq, int window)
{
    if (!f) return fail("null trainer");
    nnn_fit_rows r;
    if (int rc = fit_upload(f, rows, w, n_seq, window, "nnn_fit_loss", &r)) return rc;
    if (int rc = nnn_fit_loss_device(f, &r, f->own_stream)) return rc;
    HIPCHK(hipStreamSynchronize(f->own_stream));
    return 0;
}

extern "C" int nnn_fit_grad_host(nnn_fit *f, const float *rows, const float *w, int n_seq, int window)
{
    if (!f) return fail("null trainer");
    nnn_fit_rows r;
    if (int rc = fit_upload(f, rows, w, n_seq, window, "nnn_fit_grad", &r)) return rc;
    if (int rc = nnn_fit_grad_device(f, &r, f->own_stream)) return rc;
    HIPCHK(hipStreamSynchronize(f->own_stream));
    return 0;
}

extern "C" int nnn_fit_debug_recurrence(nnn_fit *f, int layer, int backward, int n_seq, int window, int reps, void *hip_stream)
{
    if (!f) return fail("null trainer");
    if (layer < 0 || layer > 2 || reps < 0) return fail("nnn_fit_debug_recurrence: layer %d outside [0, 2] or negative reps", layer);
    if (n_seq < 1 || n_seq > f->max_seq || window < 1 || window > f->max_window)
        return fail("nnn_fit_debug_recurrence: %d x %d outside [1, %d] x [1, %d]", n_seq, window, f->max_seq, f->max_window);
    HIPCHK(hipSetDevice(f->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : f->own_stream;
    if (f->have_last && f->last_stream != st) HIPCHK(hipStreamWaitEvent(st, f->ev_last, 0));
    const FitCarve c = fit_carve(f, (size_t)n_seq * window);
    for (int i = 0; i < reps; i++) fit_launch_gru(layer, backward != 0, fit_gru_args(f, layer, c, n_seq, window), st);
    return fit_end(f, st);
}
