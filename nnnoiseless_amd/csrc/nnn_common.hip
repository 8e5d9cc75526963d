#pragma once
// nnn_common.hip -- what more than one stage uses: the tile-interleaved addressing macros, the XCD block mapping, the phase stamps, the
// constant tables, the PCM conversions at the boundary and a call's per-frame parameters.  Not a translation unit: nnn_kernels.hip includes
// it first, and nnn_hp.hip, compiled on its own, includes nothing else.
#include "nnn_layout.h"
#include <nnn_mfma.h>

namespace nnn {

#define NNN_TI(ptr, len, tile, lane) ((ptr) + ((size_t)(tile) * (len)) * TILE + (lane))
// the same for a per-frame scratch array of frame `f` of a group (set f lies f * S_pad * len after set 0, see frame_view):
// kernels that loop over a group's frames address single fields this way instead of re-basing the whole argument block
#define NNN_TIF(b, field, len, f, tile, lane) ((b).field + ((size_t)(b).S_pad * (size_t)(f) + (size_t)(tile) * TILE) * (size_t)(len) + (lane))

// A launch of a kernel without cross-frame recurrence covers several consecutive frames: block index = frame * PER +
// block-of-frame.  Re-bases the (by-value) Buffers `b` on that frame's scratch set; `frame` and `bx` are left in scope.
#define NNN_FRAME_SPLIT(PER)                              \
    const int frame = (int)blockIdx.x / (int)(PER);      \
    const int bx = (int)blockIdx.x - frame * (int)(PER); \
    b = frame_view(b, frame);

// Block index -> (tile, block of the tile) for kernels that give a tile's 64 streams to `bpt` consecutive blocks.  Workgroup i runs on
// XCD i mod 8 (observed dispatch order; a speed matter only), so consecutive blocks would spread a tile over several XCDs -- and the
// tile-interleaved per-stream scalars (band energies, gains, cepstrum, pitch: 64 streams to a 256-byte row) would be fetched into,
// and written back from, as many L2s.  Tile t goes to XCD t mod 8 instead: where k_hp's block t and k_pitch's blocks of tile t ran.
__device__ __forceinline__ void xcd_tile_block(int blk, int ntiles, int bpt, int &tile, int &sub)
{
    const int m8 = ntiles & ~7;   // the tiles that come in eights are dealt to the XCDs; the last few keep block order
    if (blk < m8 * bpt) {
        const int xcd = blk & 7, j = blk >> 3;
        tile = xcd + 8 * (j / bpt);
        sub = j % bpt;
    } else {
        const int r = blk - m8 * bpt;
        tile = m8 + r / bpt;
        sub = r % bpt;
    }
}
// the same for launches that cover `n` units (frames, chunks of frames) per tile-block, the units of a tile-block on consecutive
// blocks of its XCD: blk -> (unit, tile, sub)
__device__ __forceinline__ void xcd_tile_block_units(int blk, int ntiles, int bpt, int n, int &unit, int &tile, int &sub)
{
    const int m8 = ntiles & ~7;
    if (blk < m8 * bpt * n) {
        const int xcd = blk & 7, j = blk >> 3, tb = j / n;
        unit = j - tb * n;
        tile = xcd + 8 * (tb / bpt);
        sub = tb % bpt;
    } else {
        // (what is left keeps the order the kernels had before: unit-major)
        const int r = blk - m8 * bpt * n, per = (ntiles - m8) * bpt;
        unit = r / per;
        const int q = r - unit * per;
        tile = m8 + q / bpt;
        sub = q % bpt;
    }
}

// Optional phase stamps (developer instrumentation, off in the shipped build): block 0 / thread 0 records the
// shader clock at labelled points so a phase breakdown can be read back through nnn_batch_read_stamps.
#ifdef NNN_STAMPS
#define NNN_STAMP(b, i) do { if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) (b).stamps[i] = (long long)__builtin_readcyclecounter(); } while (0)
// the same from lane 0 of any wave of block 0, when `cond` holds (role-by-role breakdowns)
#define NNN_STAMPW(b, i, cond) do { if (blockIdx.x == 0 && (threadIdx.x & 63) == 0 && (cond)) (b).stamps[i] = (long long)__builtin_readcyclecounter(); } while (0)
#ifndef NNN_WFSTAMP_PHASE
#define NNN_WFSTAMP_PHASE 1
#endif
#else
#define NNN_STAMP(b, i) do { } while (0)
#define NNN_STAMPW(b, i, cond) do { } while (0)
#endif

// Bark-ish band edges in units of 4 bins (ref: src/lib.rs:55-58) and SECOND_CHECK (ref: src/pitch.rs:489)
// (internal linkage: the library is two translation units since round 6 -- nnn_hp.hip -- and each carries its own copy)
#ifdef __HIPCC__
#define NNN_CONSTANT static __constant__
#else
#define NNN_CONSTANT __constant__   // (the tests' interpreter build defines __constant__ as static)
#endif
#define NNN_EBAND {0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24, 28, 34, 40, 48, 60, 78, 100}
NNN_CONSTANT int kEband[NB] = NNN_EBAND;
constexpr int kEbandHost[NB] = NNN_EBAND;   // the same edges for host code (the tables of creation): kEband is a device symbol
NNN_CONSTANT int kSecondCheck[16] = {0, 0, 3, 2, 3, 2, 5, 2, 3, 2, 3, 2, 5, 2, 3, 2};

// ---- PCM formats at the boundary ------------------------------------------------------------------
// Input conversions of the reference's callers: i16 samples are used as they are (src/nnnoiseless.rs:179-228 hands
// i16-range floats to process_frame), unit-range floats are scaled by 32768 (src/signal.rs:95-100).
template <int FMT> __device__ __forceinline__ float pcm_load(const char *p)
{
    if (FMT == PCM_I16) return (float)ld_global<short>(p);
    const float v = ld_global<float>(p);
    return FMT == PCM_F32_UNIT ? v * 32768.0f : v;
}
// Output conversions: round-half-away + clamp to i16 (RawFrameWriter / WavFrameWriter, src/nnnoiseless.rs:147-177),
// /32768 then clamp to [-1, 1] (DenoiseSignal::next, src/signal.rs:123-127).
__device__ __forceinline__ short pcm_to_i16(float v) { return (short)roundf(fminf(fmaxf(v, -32768.0f), 32767.0f)); }
__device__ __forceinline__ float pcm_to_unit(float v)
{
    v = v / 32768.0f;
    if (v < -1.0f) v = -1.0f;
    if (v > 1.0f) v = 1.0f;
    return v;
}
__device__ __forceinline__ void pcm_store(char *p, int fmt, float v)
{
    if (fmt == PCM_I16) *(short *)p = pcm_to_i16(v);
    else *(float *)p = fmt == PCM_F32_UNIT ? pcm_to_unit(v) : v;
}

// Entry t of a call's per-frame parameter table from the call's own parameters `v` (frame 0): what k_fill_params writes, and what
// k_hp -- the first kernel of a call -- works out for itself when the table is its to fill.
__device__ __forceinline__ StepParams step_params_at(const StepParams &v, int t, int nslot)
{
    StepParams p = v;
    p.in = v.in + (long long)t * v.frame_stride;
    p.out = v.out + (long long)(t - v.discard) * v.frame_stride;   // dropped frames take no room in the output
    p.discard = t < v.discard;
    p.vad = v.vad ? v.vad + (size_t)t * v.n_streams : nullptr;
    p.slot = (v.slot + t) % nslot;
    p.log = (v.log && t < v.log_frames) ? v.log + (size_t)t * v.n_streams * FRAME_LOG_WORDS : nullptr;
    return p;
}

}  // namespace nnn
