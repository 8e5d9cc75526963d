#pragma once
// nnn_split.hip -- the two boundary kernels of the split calls (nnn_batch_analyze_* / nnn_batch_synthesize_*):
// k_features_out hands the feature rows of a frame group to the caller, k_gains_in takes the caller's band gains in place of the network's.
// Not a translation unit: nnn_kernels.hip includes it behind the synthesis.

namespace nnn {

// ---------------------------------------------------------------------------------------------
// K12 features out: the feature stage's rows (k_features: tile-interleaved, lane = stream) as the caller's stream-major records,
//     rows[(t * S + s) * 42 + k], and the silence flags, flags[t * S + s] = 0 / 1.  One block per (frame, tile); block index =
//     frame * tiles + tile.  A tile's 64 x 42 floats are one contiguous 10 752-byte run of the caller's buffer: the block transposes
//     them through LDS into an image of that run and stores the image in 16-byte pieces.
//     The run starts on a 16-byte boundary only when (t * S) is even (a record is 168 bytes), so the image sits in LDS `shift` floats in,
//     shift = the run's first float modulo 4: LDS piece j is then the aligned 16 bytes at (run - shift) + 4 j whatever the caller's
//     alignment (4 bytes is all that is asked).  A piece is stored whole when its four floats belong to rows that are written; the
//     pieces at the run's ends and those that touch a row that is not -- padding behind the batch's last stream, a held stream -- go
//     float by float, the floats of such rows not at all.
//     LDS: the transposing writes have lanes 168 bytes apart, 2-way on the 32 write banks (lanes l and l + 16); the 16-byte reads are
//     consecutive.  42 write instructions per block either way.
// ---------------------------------------------------------------------------------------------
constexpr int FOUT_T = 256;
__global__ void __launch_bounds__(FOUT_T) k_features_out(Buffers b, float *rows, int *flags, int g)
{
    __shared__ float4 img4[(TILE * NFEAT + 4 + 3) / 4];
    float *img = (float *)img4;
    const int NTl = b.NT, frame = (int)blockIdx.x / NTl, tile = (int)blockIdx.x - frame * NTl;
    if (frame >= g) return;
    const int n_rows = b.S - tile * TILE < TILE ? b.S - tile * TILE : TILE;   // (the last tile: S % 64 streams)
    const unsigned long long w = live_word(b, tile) & (n_rows >= 64 ? ~0ull : (1ull << n_rows) - 1ull);   // bit i: row i of the tile is written
    if (!w) return;   // (block-uniform: every stream of the tile held)
    b = frame_view(b, frame);
    const int wave = (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    float *run = rows + ((size_t)frame * b.S + (size_t)tile * TILE) * NFEAT;
    const int shift = (int)(((size_t)run >> 2) & 3);
    const float *f = NNN_TI(b.feat, NFEAT, tile, lane);
    for (int k = wave; k < NFEAT; k += FOUT_T / 64) img[shift + lane * NFEAT + k] = f[(size_t)k * TILE];
    if (threadIdx.x < TILE && ((w >> lane) & 1ull))
        flags[(size_t)frame * b.S + tile * TILE + lane] = NNN_TI(b.silence, 1, tile, lane)[0] != 0 ? 1 : 0;
    __syncthreads();
    const int n = n_rows * NFEAT;                       // floats of the run that exist
    float *base = run - shift;                          // 16-byte aligned
    for (int j = (int)threadIdx.x; 4 * j < shift + n; j += FOUT_T) {
        const float4 v = img4[j];
        const int e0 = 4 * j - shift;                   // the piece's first float within the run
        const int r0 = e0 >= 0 ? e0 / NFEAT : -1, r3 = (e0 + 3) / NFEAT;
        if (e0 >= 0 && e0 + 3 < n && ((w >> r0) & 1ull) && ((w >> r3) & 1ull)) {
            ((float4 *)base)[j] = v;
        } else {
            const float c[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int e = e0 + i;
                if (e >= 0 && e < n && ((w >> (e / NFEAT)) & 1ull)) run[e] = c[i];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// K13 gains in: the caller's band gains gains[(t * S + s) * 22 + band] (and, optionally, VAD values vad[t * S + s]) into the scratch rows
//     k_synth reads -- g_raw, g, vad of frame sets 0 .. g - 1 -- with the smoothing g = max(g, 0.6 lastg), lastg = g of
//     src/denoise.rs:106-109 that the RNN kernels do in their epilogue (k_rnn: the gains layer's sink), in that arithmetic: plain f32
//     multiply and max.  One block per tile, four waves; lane = stream, wave w owns bands w, w + 4, ...: one (stream, band) chain per
//     lane and slot, its lastg in a register across the `g` frames of the launch (the frames are serial in lastg, so they share a launch).
//     A frame's 64 x 22 gains are one contiguous run of the caller's buffer: read with consecutive lanes on consecutive floats into LDS
//     (rows 23 floats apart: the transposed reads, lanes a row apart, fall on distinct banks), two buffers in turn, one barrier per frame.
//     Silent frames (the scratch `silence` flag of k_fft_xp): the caller's gains are ignored, lastg stays, the rows read zero as they do
//     behind the RNN kernels.  Held streams: their gains are not used and nothing of theirs is written; nor is the
//     padding behind the batch's last stream, which has no rows in the caller's buffers.
// ---------------------------------------------------------------------------------------------
constexpr int GIN_T = 256, GIN_W = GIN_T / 64, GIN_SLOTS = (NB + GIN_W - 1) / GIN_W, GIN_STR = NB + 1;
__global__ void __launch_bounds__(GIN_T) k_gains_in(Buffers b, const float *gains, const float *vad, int g)
{
    __shared__ float img[2][TILE * GIN_STR];
    const int tile = (int)blockIdx.x, wave = (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int n_rows = b.S - tile * TILE < TILE ? b.S - tile * TILE : TILE;
    const unsigned long long wr = live_word(b, tile) & (n_rows >= 64 ? ~0ull : (1ull << n_rows) - 1ull);
    if (!wr) return;   // (block-uniform)
    const bool mine = ((wr >> lane) & 1ull) != 0ull;
    const int n = n_rows * NB;
    float lg[GIN_SLOTS];
#pragma unroll
    for (int j = 0; j < GIN_SLOTS; j++) {
        const int band = wave + GIN_W * j;
        lg[j] = (mine && band < NB) ? NNN_TI(b.lastg, NB, tile, lane)[(size_t)band * TILE] : 0.0f;
    }
#pragma unroll 1
    for (int f = 0; f < g; f++) {
        float *im = img[f & 1];
        const float *run = gains + ((size_t)f * b.S + (size_t)tile * TILE) * NB;
        for (int e = (int)threadIdx.x; e < n; e += GIN_T) im[(e / NB) * GIN_STR + e % NB] = run[e];
        const bool silent = NNN_TIF(b, silence, 1, f, tile, lane)[0] != 0;
        __syncthreads();   // (the buffer written now was last read two frames back, ahead of the previous frame's barrier)
        if (!mine) continue;
#pragma unroll
        for (int j = 0; j < GIN_SLOTS; j++) {
            const int band = wave + GIN_W * j;
            if (band >= NB) continue;
            const float gr = silent ? 0.0f : im[lane * GIN_STR + band];
            float gs = 0.0f;
            if (!silent) {
                gs = fmaxf(gr, 0.6f * lg[j]);
                lg[j] = gs;
            }
            NNN_TIF(b, g_raw, NB, f, tile, lane)[(size_t)band * TILE] = gr;
            NNN_TIF(b, g, NB, f, tile, lane)[(size_t)band * TILE] = gs;
        }
        if (wave == 0) NNN_TIF(b, vad, 1, f, tile, lane)[0] = (silent || !vad) ? 0.0f : vad[(size_t)f * b.S + tile * TILE + lane];
    }
    if (!mine) return;
#pragma unroll
    for (int j = 0; j < GIN_SLOTS; j++) {
        const int band = wave + GIN_W * j;
        if (band < NB) NNN_TI(b.lastg, NB, tile, lane)[(size_t)band * TILE] = lg[j];
    }
}

}  // namespace nnn
