#pragma once
// nnn_features.hip -- K9, the feature stage's pieces (run inside the RNN kernels), its stand-alone kernel k_features and k_train_rows.  Not a
// translation unit: nnn_kernels.hip includes it between the transforms and the RNN.

namespace nnn {

// ---------------------------------------------------------------------------------------------
// K9  features: the 42 RNN inputs from band energies, pitch and the cepstral history.
//     ref: src/features.rs:135-219, src/lib.rs:139-148.  lane = stream; runs on wave 0 of the RNN kernel.
// ---------------------------------------------------------------------------------------------

// The feature stage runs inside the RNN kernel, lane = stream, in three steps so that only the truly serial part
// sits on one wave: (1) wave 0: band energies -> correlation DCT, log-energy DCT (the new cepstrum), silence
// flag, while waves 1..7 stage the 8 x 22 cepstral ring in LDS; (2) wave 0: ring update and delta features;
// (3) all waves: the 28 pairwise cepstral distances of the spectral-variability feature; wave 0 finishes.
struct FeatHead {
    float fpitch;
    bool silent;
};

// The head of the feature stage (correlation normalisation, log energies, silence test, both DCTs) is done by
// k_fft_p; this picks its results up: the new cepstrum (rows 0..21) and the pitch-correlation DCT (rows 22..27) go to
// the block's LDS staging (`cn`).  `lane` = the stream's row in its 64-stream tile (global layouts), `ll` = its column
// in the staging, `ls` = the staging's row stride (columns per block).
__device__ __forceinline__ void features_load(const Buffers &b, int tile, int lane, int ll, int ls, FeatHead &h, float *cn)
{
    const float *cg = NNN_TI(b.cn, 28, tile, lane);
    float v[28];
#pragma unroll
    for (int i = 0; i < 28; i++) v[i] = cg[(size_t)i * TILE];
    const int pitch = NNN_TI(b.pitch, 1, tile, lane)[0];
    h.silent = NNN_TI(b.silence, 1, tile, lane)[0] != 0;
    h.fpitch = 0.01f * ((float)pitch - 300.0f);
#pragma unroll
    for (int i = 0; i < 28; i++) cn[i * ls + ll] = v[i];
}

// ring update + delta features (wave 0, after the ring has been staged in crs)
__device__ __forceinline__ void features_deltas(const Buffers &b, int tile, int lane, int ll, int ls, const FeatHead &h, float *crs,
                                                const float *cn, float (&fr)[NFEAT])
{
    if (h.silent) {   // "if there's no audio, avoid messing up the state" (ref: src/features.rs:160-166)
#pragma unroll
        for (int i = 0; i < NFEAT; i++) fr[i] = 0.0f;
        return;
    }
    int *midp = NNN_TI(b.mem_id, 1, tile, lane);
    float *cm = NNN_TI(b.ceps_mem, CEPS_MEM * NB, tile, lane);
    int mem_id = midp[0];
    const int c0 = mem_id, c1 = mem_id < 1 ? CEPS_MEM + mem_id - 1 : mem_id - 1;
    const int c2 = mem_id < 2 ? CEPS_MEM + mem_id - 2 : mem_id - 2;
    float c[NB];
#pragma unroll
    for (int k = 0; k < NB; k++) {
        c[k] = cn[k * ls + ll];
        cm[(size_t)(c0 * NB + k) * TILE] = c[k];
        crs[(c0 * NB + k) * ls + ll] = c[k];
    }
    mem_id += 1;
    if (mem_id == CEPS_MEM) mem_id = 0;
    midp[0] = mem_id;
#pragma unroll
    for (int i = 0; i < NB; i++) fr[i] = c[i];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        const float v1 = crs[(c1 * NB + i) * ls + ll], v2 = crs[(c2 * NB + i) * ls + ll];
        const float v0 = c[i];
        fr[i] = v0 + v1 + v2;
        fr[NB + i] = v0 - v2;
        fr[NB + 6 + i] = v0 - 2.0f * v1 + v2;
        fr[NB + 12 + i] = cn[(NB + i) * ls + ll];
    }
    fr[40] = h.fpitch;
    fr[41] = 0.0f;
}

// pair p of the 28 unordered pairs (i < j) of ring rows
__device__ __forceinline__ void pair_of(int p, int &i, int &j)
{
    i = 0;
    int rem = p;
#pragma unroll
    for (int u = 0; u < 7; u++) {
        const int cnt = 7 - u;
        if (i == u && rem >= cnt) { rem -= cnt; i = u + 1; }
    }
    j = i + 1 + rem;
}

// squared cepstral distance of one pair, summed over the 22 bands in order (ref: src/features.rs:203-208)
__device__ __forceinline__ float pair_dist(const float *crs, int p, int lane, int ls)
{
    int i, j;
    pair_of(p, i, j);
    float dist = 0.0f;
#pragma unroll
    for (int k = 0; k < NB; k++) {
        float d = crs[(i * NB + k) * ls + lane] - crs[(j * NB + k) * ls + lane];
        dist += d * d;
    }
    return dist;
}

// spectral variability = mean_i min_{j != i} dist(i, j) - 2.1 from the 28 staged pair distances
__device__ __forceinline__ float spectral_variability(const float *dists, int lane, int ls)
{
    float mind[CEPS_MEM];
#pragma unroll
    for (int i = 0; i < CEPS_MEM; i++) mind[i] = 1e15f;
    int p = 0;
#pragma unroll
    for (int i = 0; i < CEPS_MEM; i++)
#pragma unroll
        for (int j = i + 1; j < CEPS_MEM; j++) {
            const float d = dists[p * ls + lane];
            mind[i] = fminf(mind[i], d);
            mind[j] = fminf(mind[j], d);
            p++;
        }
    float sv = 0.0f;
#pragma unroll
    for (int i = 0; i < CEPS_MEM; i++) sv += mind[i];
    return sv / (float)CEPS_MEM - 2.1f;
}

// ---------------------------------------------------------------------------------------------
// K9b features, stand-alone: the same feature stage as the RNN kernel's prologue for callers that stop at the 42
//     features (training-data generation, ref: src/training.rs:113-160).  One 64-stream tile per block, 8 waves.
// ---------------------------------------------------------------------------------------------
constexpr int FEAT_WAVES = 8;
__global__ void __launch_bounds__(64 * FEAT_WAVES) k_features(Buffers b0, int g)
{
    __shared__ float crs[CEPS_MEM * NB * TILE];   // staged cepstral ring
    __shared__ float dists[28 * TILE];            // new cepstrum / correlation DCT, then the pair distances
    const int wave = (int)(threadIdx.x >> 6), lane = threadIdx.x & 63, tile = blockIdx.x;
    // the frames of a group one after the other (the cepstral ring is the tile's own state, carried through memory)
#pragma unroll 1
    for (int fr_i = 0; fr_i < g; fr_i++) {
    const Buffers b = frame_view(b0, fr_i);
    if (fr_i) __syncthreads();
    FeatHead fh;
    float fr[NFEAT];
    if (wave == 0) {
        features_load(b, tile, lane, lane, TILE, fh, dists);
    } else {
        const float *cm = NNN_TI(b.ceps_mem, CEPS_MEM * NB, tile, lane);
        for (int r = wave - 1; r < CEPS_MEM * NB; r += FEAT_WAVES - 1) crs[r * TILE + lane] = cm[(size_t)r * TILE];
    }
    __syncthreads();
    if (wave == 0) features_deltas(b, tile, lane, lane, TILE, fh, crs, dists, fr);
    __syncthreads();
    for (int p = wave; p < 28; p += FEAT_WAVES) dists[p * TILE + lane] = pair_dist(crs, p, lane, TILE);
    __syncthreads();
    if (wave == 0) {
        if (!fh.silent) fr[41] = spectral_variability(dists, lane, TILE);
        float *f = NNN_TI(b.feat, NFEAT, tile, lane);
#pragma unroll
        for (int k = 0; k < NFEAT; k++) f[(size_t)k * TILE] = fr[k];
    }
    }
}

// One training row per stream (ref: src/training.rs:136-158): the combined signal's 42 features, 22 ideal band gains
// sqrt((Ex_clean + 1e-3) / (Ex_combined + 1e-3)) capped at 1 (-1 where both energies are below 5e-2, and from the
// band cutoff up; cutoff 0 on silent frames), 22 noise levels log10(Ex_noise + 1e-2), and the caller's VAD label.
constexpr int TRAIN_COLS = NFEAT + 2 * NB + 1;
__global__ void __launch_bounds__(64) k_train_rows(Buffers comb, Buffers clean, Buffers noise, const int *cutoff, const float *vad,
                                                   float *rows)
{
    __shared__ float row[TILE][TRAIN_COLS + 1];
    // block index = frame * tiles + tile: the frames of a group in one launch, frame f's labels and rows f * S further on
    const int NTl = comb.S_pad / TILE, frame = (int)blockIdx.x / NTl;
    const int lane = threadIdx.x, tile = (int)blockIdx.x - frame * NTl, s = tile * TILE + lane;
    comb = frame_view(comb, frame);
    clean = frame_view(clean, frame);
    noise = frame_view(noise, frame);
    cutoff += (size_t)frame * comb.S;
    vad += (size_t)frame * comb.S;
    rows += (size_t)frame * comb.S * TRAIN_COLS;
    if (s < comb.S) {
        const bool silent = NNN_TI(comb.silence, 1, tile, lane)[0] != 0;
        const int cut = silent ? 0 : cutoff[s];
        const float *f = NNN_TI(comb.feat, NFEAT, tile, lane);
        for (int k = 0; k < NFEAT; k++) row[lane][k] = f[(size_t)k * TILE];
        const float *ec = NNN_TI(clean.ex, NB, tile, lane), *ex = NNN_TI(comb.ex, NB, tile, lane), *en = NNN_TI(noise.ex, NB, tile, lane);
        for (int i = 0; i < NB; i++) {
            const float c = ec[(size_t)i * TILE], x = ex[(size_t)i * TILE];
            float g = -1.0f;
            if (i < cut && !(c < 5e-2f && x < 5e-2f)) g = fminf(sqrtf((c + 1e-3f) / (x + 1e-3f)), 1.0f);
            row[lane][NFEAT + i] = g;
            row[lane][NFEAT + NB + i] = log10f(en[(size_t)i * TILE] + 1e-2f);
        }
        row[lane][NFEAT + 2 * NB] = vad[s];
    }
    __syncthreads();
    // rows of the tile are contiguous in the output: write them coalesced
    const int n = (comb.S - tile * TILE < TILE ? comb.S - tile * TILE : TILE) * TRAIN_COLS;
    float *o = rows + (size_t)tile * TILE * TRAIN_COLS;
    for (int i = lane; i < n; i += 64) o[i] = row[i / TRAIN_COLS][i % TRAIN_COLS];
}

}  // namespace nnn
