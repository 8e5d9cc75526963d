#pragma once
// nnn_stream_state.hip -- the device side of the per-stream state records: the record's word layout (SS_*), SsArgs, which the host fills, the
// ss_* helpers and the k_ss_* kernels.  Not a translation unit: nnn_batch_streams.hip includes it under "per-stream state records", ahead of the host
// functions that launch these kernels; it sits at global scope there, behind `using namespace nnn`.

constexpr int SS_WORDS = NNN_STREAM_STATE_BYTES / 4;
constexpr int SS_W_TI = NNN_STREAM_STATE_OFF_MEM_ID / 4;           // words 6 .. 10: mem_id, last_period, last_gain, mem_hp_x[2] (TI rows 0 .. 4)
constexpr int SS_W_IN = NNN_STREAM_STATE_OFF_INPUT_MEM / 4;
constexpr int SS_W_SYN = NNN_STREAM_STATE_OFF_SYNTHESIS_MEM / 4;
constexpr int SS_W_CEPS = NNN_STREAM_STATE_OFF_CEPSTRAL_MEM / 4;    // ceps_mem then lastg: TI rows 5 .. 202
constexpr int SS_W_GRU = NNN_STREAM_STATE_OFF_VAD_GRU / 4;
constexpr int SS_GRU = 128;
constexpr int SS_TI_ROWS = 5 + CEPS_MEM * NB + NB;
constexpr int SS_DEC = 3 * 240;     // decimated values of frames frame_count - 3 .. - 1: what the next frame's 864-value window reaches back to
constexpr int SS_DEC_X0 = HIST - 3 * FRAME;   // input_mem index of frame frame_count - 3's first sample
constexpr int SS_SMALL = 32;        // index lists up to this long travel in the kernel arguments
constexpr int SS_CHUNK = 96;        // samples per LDS chunk of the tile kernel's import
static_assert(NNN_STREAM_STATE_OFF_LASTG / 4 == SS_W_CEPS + CEPS_MEM * NB && SS_W_GRU == SS_W_CEPS + CEPS_MEM * NB + NB + 2, "record layout");
static_assert(SS_W_GRU + 3 * SS_GRU == SS_WORDS && SS_W_SYN == SS_W_IN + HIST && SS_W_CEPS == SS_W_SYN + FRAME, "record layout");
static_assert(HIST % SS_CHUNK == 0 && SS_DEC_X0 % SS_CHUNK == 0 && FRAME % SS_CHUNK == 0, "chunking");

struct SsArgs {
    const int *dims;    // per tile: GRU sizes of its model, nv | nn << 8 | ndn << 16
    const int *idx;     // mode 2: the index list in device memory
    int small[SS_SMALL];   // mode 1
    int mode;           // stream of entry i: 0 = first + i, 1 = small[i], 2 = idx[i]
    int first, n;
    int rb_in;          // ring position of input_mem[0] (newest frame in the slot before frame_count's)
    int dec_row0;       // decimated-ring row of the first value of frame frame_count - 3
    int slot_next;      // ring slot of frame frame_count
    const int *flag;    // device import: != 0 = the record check refused the list (nothing is written)
    // hold / resume (nnn_batch_hold_streams): the records are the batch's own parked ones, record of stream s at index s, and the kernel
    // that moves a stream's state also flips its bit of the live mask
    int by_stream;      // mode 1 / 2: the record of entry i is record ss_stream(i), not record i (mode 0: the caller offsets the pointer)
    int live_op;        // 0 = leave the mask alone, 1 = clear the listed streams' bits (hold), 2 = set them (resume)
    unsigned long long *live;
};
// bits of one tile's live word: a plain vector atomic (the launches of a batch are ordered, the streams of a list may share a word)
__device__ __forceinline__ void ss_live_bits(const SsArgs &a, int tile, unsigned long long bits)
{
#ifdef __HIPCC__
    if (a.live_op == 1) atomicAnd(a.live + tile, ~bits);
    else atomicOr(a.live + tile, bits);
#else   // (the tests' interpreter runs one thread at a time)
    if (a.live_op == 1) a.live[tile] &= ~bits;
    else a.live[tile] |= bits;
#endif
}
__device__ __forceinline__ int ss_stream(const SsArgs &a, int i) { return a.mode == 0 ? a.first + i : (a.mode == 1 ? a.small[i] : a.idx[i]); }

// the 32-bit word of TI row r (record order: mem_id, last_period, last_gain, mem_hp_x[0..1], ceps_mem[8][22], lastg[22]) of a stream
__device__ __forceinline__ unsigned *ss_ti(const Buffers &b, int r, int tile, int lane)
{
    if (r == 0) return (unsigned *)NNN_TI(b.mem_id, 1, tile, lane);
    if (r == 1) return (unsigned *)NNN_TI(b.last_period, 1, tile, lane);
    if (r == 2) return (unsigned *)NNN_TI(b.last_gain, 1, tile, lane);
    if (r < 5) return (unsigned *)(NNN_TI(b.hp_mem, 2, tile, lane) + (size_t)(r - 3) * TILE);
    if (r < 5 + CEPS_MEM * NB) return (unsigned *)(NNN_TI(b.ceps_mem, CEPS_MEM * NB, tile, lane) + (size_t)(r - 5) * TILE);
    return (unsigned *)(NNN_TI(b.lastg, NB, tile, lane) + (size_t)(r - 5 - CEPS_MEM * NB) * TILE);
}
// record word j -> TI row, or -1
__device__ __forceinline__ int ss_ti_row(int j)
{
    if (j >= SS_W_TI && j < SS_W_TI + 5) return j - SS_W_TI;
    if (j >= SS_W_CEPS && j < SS_W_CEPS + CEPS_MEM * NB + NB) return 5 + j - SS_W_CEPS;
    return -1;
}
// stream s's GRU row k (0 vad, 1 noise, 2 denoise): rows of the model's own width inside a tile sized for the widest model
__device__ __forceinline__ unsigned *ss_gru(const Buffers &b, int k, int s, int n)
{
    const size_t tile = (size_t)(s / TILE), r = (size_t)(s % TILE);
    float *p = k == 0 ? b.gru_v + tile * TILE * b.gru_v_w : (k == 1 ? b.gru_n + tile * TILE * b.gru_n_w : b.gru_dn + tile * TILE * b.gru_dn_w);
    return (unsigned *)(p + r * (size_t)n);
}
__device__ __forceinline__ size_t ss_hist_at(const Buffers &b, const SsArgs &a, int s, int i)   // input_mem[i] of stream s in the ring
{
    int p = a.rb_in + i;
    if (p >= ring_len(b.nslot)) p -= ring_len(b.nslot);
    return (size_t)s * hist_stride(b.nslot) + p;
}
// record word j of stream s, every word but the TI rows (ti = nullptr: those too, read one at a time)
__device__ __forceinline__ unsigned ss_export_word(const Buffers &b, const SsArgs &a, int s, int j, int dims)
{
    if (j < SS_W_IN) {
        const int r = ss_ti_row(j);
        if (r >= 0) return *ss_ti(b, r, s / TILE, s % TILE);
        if (j == 0) return NNN_STREAM_STATE_MAGIC;
        if (j == 1) return NNN_STREAM_STATE_VERSION;
        if (j == 2) return NNN_STREAM_STATE_BYTES;
        if (j < 6) return (unsigned)((dims >> (8 * (j - 3))) & 255);
        return 0u;
    }
    if (j < SS_W_SYN) return ((const unsigned *)b.hist)[ss_hist_at(b, a, s, j - SS_W_IN)];
    if (j < SS_W_CEPS) return ((const unsigned *)b.synth_mem)[(size_t)s * FRAME + (j - SS_W_SYN)];
    if (j < SS_W_GRU) {
        const int r = ss_ti_row(j);
        return r >= 0 ? *ss_ti(b, r, s / TILE, s % TILE) : 0u;
    }
    const int k = (j - SS_W_GRU) / SS_GRU, u = (j - SS_W_GRU) % SS_GRU, n = (dims >> (8 * k)) & 255;
    return u < n ? ss_gru(b, k, s, n)[u] : 0u;
}
// record word j (value v) of stream s into the batch: everything but the TI rows and the derived values
__device__ __forceinline__ void ss_import_word(const Buffers &b, const SsArgs &a, int s, int j, unsigned v, int dims)
{
    if (j < SS_W_IN) return;
    if (j < SS_W_SYN) {
        const size_t at = ss_hist_at(b, a, s, j - SS_W_IN);
        ((unsigned *)b.hist)[at] = v;
        if (at == (size_t)s * hist_stride(b.nslot)) ((unsigned *)b.hist)[at + ring_len(b.nslot)] = v;   // hist[ring_len] repeats hist[0]
        return;
    }
    if (j < SS_W_CEPS) { ((unsigned *)b.synth_mem)[(size_t)s * FRAME + (j - SS_W_SYN)] = v; return; }
    if (j < SS_W_GRU) return;
    const int k = (j - SS_W_GRU) / SS_GRU, u = (j - SS_W_GRU) % SS_GRU, n = (dims >> (8 * k)) & 255;
    if (u < n) ss_gru(b, k, s, n)[u] = v;
}
// decimated value k (0 .. SS_DEC) from input_mem x[SS_DEC_X0 + 2k - 1 .. + 1], as k_hp / k_hp2 make it, into its ring row (and the mirror)
__device__ __forceinline__ void ss_dec_store(const Buffers &b, const SsArgs &a, int tile, int lane, int k, float xa, float xm, float xn)
{
    const int nslot = b.nslot;
    int row = a.dec_row0 + k;
    if (row >= dec_ring_len(nslot)) row -= dec_ring_len(nslot);
    float *ring = NNN_TI(b.dec, dec_len(nslot), tile, lane);
    const float dv = ((xa + xn) / 2.0f + xm) / 2.0f;
    ring[(size_t)row * TILE] = dv;
    if (row < DEC_MIRROR * 240) ring[(size_t)(dec_ring_len(nslot) + row) * TILE] = dv;
}
// x_lp[0] of the next frame (its window starts at input_mem[480]) and the last filtered sample
__device__ __forceinline__ void ss_derived(const Buffers &b, const SsArgs &a, int tile, int lane, float x480, float x481, float x_last)
{
    NNN_TI(b.xlp0, b.nslot, tile, lane)[(size_t)a.slot_next * TILE] = (x481 / 2.0f + x480) / 2.0f;   // as hp_frame
    NNN_TI(b.hp_last, 1, tile, lane)[0] = x_last;
}

// a few streams: one block of 256 threads per list entry
__global__ void __launch_bounds__(256) k_ss_export_streams(Buffers b, SsArgs a, unsigned *dst)
{
    const int i = blockIdx.x, s = ss_stream(a, i), dims = a.dims[s / TILE];
    unsigned *rec = dst + (size_t)(a.by_stream ? s : i) * SS_WORDS;
    for (int j = threadIdx.x; j < SS_WORDS; j += 256) rec[j] = ss_export_word(b, a, s, j, dims);
    if (a.live_op && threadIdx.x == 0) ss_live_bits(a, s / TILE, 1ull << (s % TILE));
}
// src = nullptr: the zero record (reset)
__global__ void __launch_bounds__(256) k_ss_import_streams(Buffers b, SsArgs a, const unsigned *src)
{
    if (a.flag && a.flag[0]) return;
    const int i = blockIdx.x, s = ss_stream(a, i), dims = a.dims[s / TILE], tile = s / TILE, lane = s % TILE;
    const unsigned *rec = src ? src + (size_t)(a.by_stream ? s : i) * SS_WORDS : nullptr;
    if (a.live_op && threadIdx.x == 0) ss_live_bits(a, tile, 1ull << lane);
    for (int j = threadIdx.x; j < SS_WORDS; j += 256) {
        const unsigned v = rec ? rec[j] : 0u;
        const int r = ss_ti_row(j);
        if (r >= 0) *ss_ti(b, r, tile, lane) = v;
        else ss_import_word(b, a, s, j, v, dims);
    }
    const float *x = rec ? (const float *)(rec + SS_W_IN) : nullptr;
    for (int k = threadIdx.x; k < SS_DEC; k += 256) {
        const int p = SS_DEC_X0 + 2 * k;
        ss_dec_store(b, a, tile, lane, k, x ? x[p - 1] : 0.0f, x ? x[p] : 0.0f, x ? x[p + 1] : 0.0f);
    }
    if (threadIdx.x == 0) ss_derived(b, a, tile, lane, x ? x[FRAME] : 0.0f, x ? x[FRAME + 1] : 0.0f, x ? x[HIST - 1] : 0.0f);
}

// A contiguous run of streams (a migration, a whole batch): one block per tile, lane = stream on the TI rows (one 256-byte row per wave
// instruction), the record's TI words transposed through LDS; the stream-major parts are contiguous runs of the record either way.
// the bits of the streams of `tile` that a contiguous list (mode 0) names
__device__ __forceinline__ unsigned long long ss_tile_bits(const SsArgs &a, int tile)
{
    const int lo = a.first > tile * TILE ? a.first - tile * TILE : 0, hi = a.first + a.n < (tile + 1) * TILE ? a.first + a.n - tile * TILE : TILE;
    const unsigned long long upto = hi >= TILE ? ~0ull : (1ull << hi) - 1ull;
    return upto & ~((1ull << lo) - 1ull);
}
__global__ void __launch_bounds__(256) k_ss_export_tiles(Buffers b, SsArgs a, unsigned *dst)
{
    __shared__ unsigned T[SS_TI_ROWS][TILE + 1];
    const int tile = a.first / TILE + (int)blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int dims = a.dims[tile];
    for (int r = wave; r < SS_TI_ROWS; r += 4) T[r][lane] = *ss_ti(b, r, tile, lane);
    __syncthreads();
    for (int q = 0; q < TILE; q++) {
        const int s = tile * TILE + q;
        if (s < a.first || s >= a.first + a.n) continue;
        unsigned *rec = dst + (size_t)(s - a.first) * SS_WORDS;
        for (int j = tid; j < SS_WORDS; j += 256) {
            const int r = ss_ti_row(j);
            rec[j] = r >= 0 ? T[r][q] : ss_export_word(b, a, s, j, dims);
        }
    }
    if (a.live_op && tid == 0) ss_live_bits(a, tile, ss_tile_bits(a, tile));
}
__global__ void __launch_bounds__(256) k_ss_import_tiles(Buffers b, SsArgs a, const unsigned *src)
{
    __shared__ unsigned T[SS_TI_ROWS][TILE + 1];
    __shared__ float X[TILE][SS_CHUNK + 1];   // a chunk of input_mem of every stream, and the sample before it (column 0)
    if (a.flag && a.flag[0]) return;
    const int tile = a.first / TILE + (int)blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int dims = a.dims[tile];
    if (a.live_op && tid == 0) ss_live_bits(a, tile, ss_tile_bits(a, tile));
    const int s_me = tile * TILE + lane;
    const bool mine = s_me >= a.first && s_me < a.first + a.n;   // (lane = stream)
    auto rec_of = [&](int q) { return src + (size_t)(tile * TILE + q - a.first) * SS_WORDS; };
    auto listed = [&](int q) { const int s = tile * TILE + q; return s >= a.first && s < a.first + a.n; };
    // TI rows: records -> LDS (each stream's words in runs) -> one row of 64 streams per store
    for (int e = tid; e < TILE * SS_TI_ROWS; e += 256) {
        const int q = e / SS_TI_ROWS, r = e - q * SS_TI_ROWS;
        T[r][q] = (src && listed(q)) ? rec_of(q)[r < 5 ? SS_W_TI + r : SS_W_CEPS + r - 5] : 0u;
    }
    __syncthreads();
    if (mine)
        for (int r = wave; r < SS_TI_ROWS; r += 4) *ss_ti(b, r, tile, lane) = T[r][lane];
    // overlap memory and GRU rows: runs of the record
    for (int q = 0; q < TILE; q++) {
        if (!listed(q)) continue;
        const int s = tile * TILE + q;
        for (int j = SS_W_SYN + tid; j < SS_W_CEPS; j += 256) ss_import_word(b, a, s, j, src ? rec_of(q)[j] : 0u, dims);
        for (int j = SS_W_GRU + tid; j < SS_WORDS; j += 256) ss_import_word(b, a, s, j, src ? rec_of(q)[j] : 0u, dims);
    }
    // input_mem in chunks through LDS: the history ring (runs of each stream), the decimated ring (rows of 64 streams), x_lp[0], the last sample
    for (int c = 0; c < HIST / SS_CHUNK; c++) {
        __syncthreads();   // (the previous chunk has been read)
        for (int e = tid; e < TILE * (SS_CHUNK + 1); e += 256) {
            const int q = e / (SS_CHUNK + 1), i = e - q * (SS_CHUNK + 1), x = c * SS_CHUNK + i - 1;
            X[q][i] = (src && listed(q) && x >= 0) ? ((const float *)rec_of(q))[SS_W_IN + x] : 0.0f;
        }
        __syncthreads();
        for (int e = tid; e < TILE * SS_CHUNK; e += 256) {
            const int q = e / SS_CHUNK, i = e - q * SS_CHUNK;
            if (listed(q)) ss_import_word(b, a, tile * TILE + q, SS_W_IN + c * SS_CHUNK + i, __float_as_uint(X[q][i + 1]), dims);
        }
        if (mine && c * SS_CHUNK >= SS_DEC_X0)
            for (int kl = wave; kl < SS_CHUNK / 2; kl += 4)
                ss_dec_store(b, a, tile, lane, (c * SS_CHUNK - SS_DEC_X0) / 2 + kl, X[lane][2 * kl], X[lane][2 * kl + 1], X[lane][2 * kl + 2]);
        if (mine && wave == 0 && c == FRAME / SS_CHUNK) NNN_TI(b.xlp0, b.nslot, tile, lane)[(size_t)a.slot_next * TILE] = (X[lane][2] / 2.0f + X[lane][1]) / 2.0f;
        if (mine && wave == 0 && c == HIST / SS_CHUNK - 1) NNN_TI(b.hp_last, 1, tile, lane)[0] = X[lane][SS_CHUNK];
    }
}
// a device import's records against their target streams (magic, version, size, GRU sizes): any mismatch drops the whole list
__global__ void __launch_bounds__(256) k_ss_check(SsArgs a, const unsigned *src, int *flag, int *report)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const unsigned *rec = src + (size_t)i * SS_WORDS;
    const int dims = a.dims[ss_stream(a, i) / TILE];
    bool bad = rec[0] != NNN_STREAM_STATE_MAGIC || rec[1] != NNN_STREAM_STATE_VERSION || rec[2] != NNN_STREAM_STATE_BYTES;
    for (int k = 0; k < 3; k++) bad = bad || rec[3 + k] != (unsigned)((dims >> (8 * k)) & 255);
    if (bad) {   // (every writer writes the same value)
        flag[0] = 1;
        report[0] = 1;
    }
}

// The listed streams that are held keep their state in the parked record, not in the batch: an export's record comes from there
// (to_records), an import's or a reset's (src = nullptr: the zero record) goes there.  Runs behind the ordinary kernel of the call, which
// has read or written the held streams' dead batch state to no effect.
__global__ void __launch_bounds__(256) k_ss_parked(SsArgs a, const unsigned long long *live, unsigned *park, int to_records, unsigned *recs, const unsigned *src)
{
    if (a.flag && a.flag[0]) return;
    const int i = blockIdx.x, s = ss_stream(a, i), dims = a.dims[s / TILE];
    if ((live[s / TILE] >> (s % TILE)) & 1ull) return;
    unsigned *slab = park + (size_t)s * SS_WORDS;
    for (int j = threadIdx.x; j < SS_WORDS; j += 256) {
        if (to_records) recs[(size_t)i * SS_WORDS + j] = slab[j];
        else if (src) slab[j] = src[(size_t)i * SS_WORDS + j];
        else slab[j] = j == 0 ? NNN_STREAM_STATE_MAGIC : j == 1 ? NNN_STREAM_STATE_VERSION : j == 2 ? NNN_STREAM_STATE_BYTES : j < 6 ? (unsigned)((dims >> (8 * (j - 3))) & 255) : 0u;
    }
}
