#pragma once
// nnn_synth.hip -- K11, the synthesis: band gain interpolation, synth_frame (also the fused back end's frame body) and k_synth.  Not a
// translation unit: nnn_kernels.hip includes it last of the stages, behind k_rnn_wf.

namespace nnn {

// interpolated band gain at bin k (ref: src/lib.rs:84-97): zero for k >= 400
__device__ __forceinline__ float interp_gain(const float *g, int k, const float *bin_frac, const unsigned char *bin_band)
{
    if (k >= 400) return 0.0f;
    int i = bin_band[k];
    float frac = bin_frac[bsk(k)];   // (the LDS table is skewed)
    return fmaf(frac, g[i + 1], (1.0f - frac) * g[i]);
}
// the same for two gain vectors at once (one look-up of the bin's band and weight serves both)
__device__ __forceinline__ void interp_gain2(const float *ga, const float *gb, int k, const float *bin_frac, const unsigned char *bin_band,
                                             float &ra, float &rb)
{
    ra = 0.0f;
    rb = 0.0f;
    if (k >= 400) return;
    const int i = bin_band[k];
    const float frac = bin_frac[bsk(k)], om = 1.0f - frac;
    ra = fmaf(frac, ga[i + 1], om * ga[i]);
    rb = fmaf(frac, gb[i + 1], om * gb[i]);
}

// ---------------------------------------------------------------------------------------------
// K11 synth: pitch filter, band renormalisation, gains, inverse FFT, window, overlap-add.
//     ref: src/features.rs:223-275, src/denoise.rs:103-114.  One wave per stream; the launch loops over the `g` frames of
//     its group with the overlap memory in registers (read and written once per group, not per frame).
// ---------------------------------------------------------------------------------------------
// ---- pitch filter, band renormalisation, gains, inverse transform, overlap-add for the stream of this wave (ref: src/features.rs:223-275,
//      src/denoise.rs:103-114) on spectra in the wave's registers in the transforms' own bin order (rfft_slot_bin): the frame body of
//      k_synth (spectra from memory) and of the fused back end (spectra straight from its transforms).  b_* are the lane's band
//      (lane < NB) quantities.  The overlap memory is `smv` (sample quads of lane j: samples 4 j + 256 u .. + 3), loaded and stored
//      around the frame when SMV_IO (the fused kernel: eight registers it has not got across a frame) or carried by the caller.
// The band and the interpolation weight of a lane's eight bins are constants of the lane: k_synth, which loops over the frames of a group,
// reads them from the tables once per launch and keeps them in registers (BinConst; round 5: two LDS reads and their index arithmetic less
// per bin and use, three uses per frame: k_synth -2.7 %); the fused back end, which has no registers to spare, looks them up where it
// needs them (null).  Same products of the same factors either way.  (At 128 registers the kernel now spills one 64-bit value, the address
// of the stream's overlap memory: stored before the frame loop, reloaded once behind it -- two scratch accesses per launch, none per frame.)
struct BinConst { int band[8]; float frac[8]; };   // band: -1 = no gain there (bins from 400 up, empty slots)
// PLAIN (round 5): the call's boundary format is process_frame's own -- f32 in the range of an i16, one channel -- known when the kernel is launched:
// the conversions, the channel arithmetic and their branches are compiled out of the instantiation the bench and most device-buffer callers run.
// TRANSFORMED: called behind the inverse transform, ahead of the overlap-add.  Xr, Pk and the band quantities have been dead since the spectrum
// went to LDS, and the transform's own registers are free again: k_synth requests its next frame's inputs there (see k_synth).  The fused
// back end passes nothing.
struct SynthNoHook { __device__ __forceinline__ void operator()() const {} };
template <bool SMV_IO, bool PLAIN = false, class TRANSFORMED = SynthNoHook>
__device__ __forceinline__ void synth_frame(const Buffers &b, const StepParams *sp, int f, int tile, int sl, int s, int lane, const FftLds &t, float2 *A,
                                         float *r, float2 (&Xr)[8], const float2 (&Pk)[8], float b_ex, float b_ep, float b_xp, float b_graw,
                                         float b_g, float vadv, bool live, float *sm, float4 (&smq)[2], const BinConst *bc = nullptr,
                                         TRANSFORMED &&transformed = SynthNoHook())
{
    if (SMV_IO) {
#pragma unroll
        for (int u = 0; u < 2; u++) smq[u] = lane + 64 * u < FRAME / 4 ? ((const float4 *)sm)[lane + 64 * u] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    float *ebuf = (float *)A, *r2 = r + NB, *gg = r + 2 * NB;
    float *vad_out = sp->vad;
    const int fmt = PLAIN ? (int)PCM_F32 : sp->fmt;
    const int ch = PLAIN ? 1 : sp->channels, grp = s / ch, elem = pcm_elem_bytes(fmt), sstride = ch * elem;
    char *o = sp->out + (long long)grp * sp->group_stride + (long long)(s - grp * ch) * elem;
    const bool store = s < b.S && !sp->discard;
    int bmask = 1 << NB;             // lane 0: this frame's branch mask (bit 22: silent)
    if (live) {
        const bool up = b_xp > b_graw;   // the branch the parity tests compare (ref: src/features.rs:227)
        const int mask = (int)(wave_ballot(up && lane < NB) & ((1ull << NB) - 1));   // bit i: band i took `exp > g`
        if (lane < NB) {
            float v;
            if (up) v = 1.0f;
            else {
                float exp_sq = b_xp * b_xp, g_sq = b_graw * b_graw;
                v = exp_sq * (1.0f - g_sq) / (0.001f + g_sq * (1.0f - exp_sq));
            }
            v = sqrtf(fminf(fmaxf(v, 0.0f), 1.0f));
            v *= sqrtf(b_ex / (1e-8f + b_ep));
            r[lane] = v;
            gg[lane] = b_g;
        }
        wave_lds_sync();
        if (lane == 0) {
            NNN_TIF(b, branch, 1, f, tile, sl)[0] = mask;
            bmask = mask;
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int k = rfft_slot_bin(lane, u);
            if (k >= 0) {
                float2 X = Xr[u];
                const float2 P = k < 400 ? Pk[u] : make_float2(0.0f, 0.0f);   // from bin 400 up the filter gain is zero
                float rf;
                if (!SMV_IO && bc) {
                    const int i = bc->band[u] < 0 ? 0 : bc->band[u];
                    const float fr = bc->frac[u];
                    rf = bc->band[u] < 0 ? 0.0f : fmaf(fr, r[i + 1], (1.0f - fr) * r[i]);
                } else rf = interp_gain(r, k, t.frac, t.band);
                X.x = fmaf(P.x, rf, X.x);
                X.y = fmaf(P.y, rf, X.y);
                Xr[u] = X;
                if (k < 400) ebuf[bsk(k)] = fmaf(X.y, X.y, X.x * X.x);
            }
        }
        wave_lds_sync();
        {
            const float *const v[1] = {ebuf};
            float ne[1];
            band_sums_par<1>(t, v, ne, lane);
            if (lane < NB) r2[lane] = sqrtf(b_ex / (1e-8f + ne[0]));
        }
        wave_lds_sync();
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int k = rfft_slot_bin(lane, u);
            if (k >= 0) {
                float rf, gf;
                if (!SMV_IO && bc) {
                    const int i = bc->band[u] < 0 ? 0 : bc->band[u];
                    const float fr = bc->frac[u], om = 1.0f - fr;
                    rf = bc->band[u] < 0 ? 0.0f : fmaf(fr, r2[i + 1], om * r2[i]);
                    gf = bc->band[u] < 0 ? 0.0f : fmaf(fr, gg[i + 1], om * gg[i]);
                } else interp_gain2(r2, gg, k, t.frac, t.band, rf, gf);
                Xr[u].x *= rf; Xr[u].y *= rf;
                Xr[u].x *= gf; Xr[u].y *= gf;
            }
        }
    } else if (lane == 0) {
        NNN_TIF(b, branch, 1, f, tile, sl)[0] = 1 << NB;
    }
    if (sp->log && s < b.S) {   // parity-test record of this frame: pitch index, branch mask, smoothed gains
        unsigned *lg = sp->log + (size_t)s * FRAME_LOG_WORDS;
        if (lane < NB) lg[2 + lane] = __float_as_uint(live ? b_g : 0.0f);
        if (lane == 0) {
            lg[0] = (unsigned)NNN_TIF(b, pitch, 1, f, tile, sl)[0];
            lg[1] = (unsigned)bmask;
        }
    }
#pragma unroll
    for (int u = 0; u < 8; u++) {
        const int k = rfft_slot_bin(lane, u);
        if (k >= 0) A[k] = Xr[u];
    }
    wave_lds_sync();
    // complex-to-real 960-point inverse as a 480-point complex inverse (see k_synth)
    float2 zin[8];
    {
        const int j = lane < FFT_P1 ? lane : FFT_P1 - 1;
#pragma unroll
        for (int rr = 0; rr < 8; rr++) {
            const int k = j + FFT_P1 * rr;
            float2 a = A[k], c = A[NFFT - k];
            float2 e2 = make_float2(a.x + c.x, a.y - c.y);
            float2 d = make_float2(a.x - c.x, a.y + c.y);
            float2 w = t.tw[k];
            w.y = -w.y;
            float2 o2 = cmulf(d, w);
            zin[rr] = make_float2(e2.y + o2.x, e2.x - o2.y);
        }
    }
    wave_lds_sync();   // the spectrum has been read: the transform takes its buffer
    // (from here on a lane owns sample quads: samples 4 j + 256 u .. + 3 of both halves, j = lane, u < 2 -- 16-byte reads of the
    // transform, the window and the overlap memory, 16-byte stores of the audio; same arithmetic per sample as with pairs)
    float4 wlo[2], whi[2];   // the two window halves
#pragma unroll
    for (int u = 0; u < 2; u++) {
        const int n = lane + 64 * u;
        const bool on = n < FRAME / 4;
        wlo[u] = on ? ((const float4 *)b.window_s)[n] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);   // (window / 2: the inverse transform's halving rides on it)
        whi[u] = on ? ((const float4 *)b.window_s)[FRAME / 4 + n] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    fft480_regs<true, !SMV_IO>(zin, A, t.tw, lane);   // time samples: x[2n] = A[n].y, x[2n+1] = A[n].x
    transformed();
    if (lane == 0 && vad_out && s < b.S) vad_out[s] = vadv;
    const bool quad_ok = ch == 1 && (((size_t)o) & (size_t)(4 * elem - 1)) == 0;
#pragma unroll
    for (int u = 0; u < 2; u++) {
        const int n = lane + 64 * u;
        if (n < FRAME / 4) {
            const float4 lo = ((const float4 *)A)[n], hi = ((const float4 *)A)[n + FRAME / 4];   // (A[2n], A[2n + 1]) each
            const float u0 = hi.y * whi[u].x, u1 = hi.x * whi[u].y, u2 = hi.w * whi[u].z, u3 = hi.z * whi[u].w;   // (x / 2) * w and x * (w / 2) are the same float
            if (store) {
                const float y0 = fmaf(lo.y, wlo[u].x, smq[u].x), y1 = fmaf(lo.x, wlo[u].y, smq[u].y), y2 = fmaf(lo.w, wlo[u].z, smq[u].z),
                            y3 = fmaf(lo.z, wlo[u].w, smq[u].w);
                if (quad_ok && fmt == PCM_F32) ((float4 *)o)[n] = make_float4(y0, y1, y2, y3);
                else if (quad_ok && fmt == PCM_I16)
                    ((uint2 *)o)[n] = make_uint2((unsigned)(unsigned short)pcm_to_i16(y0) | ((unsigned)(unsigned short)pcm_to_i16(y1) << 16),
                                                 (unsigned)(unsigned short)pcm_to_i16(y2) | ((unsigned)(unsigned short)pcm_to_i16(y3) << 16));
                else if (quad_ok) ((float4 *)o)[n] = make_float4(pcm_to_unit(y0), pcm_to_unit(y1), pcm_to_unit(y2), pcm_to_unit(y3));
                else {
                    pcm_store(o + (long long)(4 * n) * sstride, fmt, y0);
                    pcm_store(o + (long long)(4 * n + 1) * sstride, fmt, y1);
                    pcm_store(o + (long long)(4 * n + 2) * sstride, fmt, y2);
                    pcm_store(o + (long long)(4 * n + 3) * sstride, fmt, y3);
                }
            }
            smq[u] = make_float4(u0, u1, u2, u3);
            if (SMV_IO) ((float4 *)sm)[n] = smq[u];
        }
    }
    wave_lds_sync();   // A is refilled by the next frame
}

// wait until every vector-memory access the wave has issued is complete (the tests' interpreter has none in flight)
__device__ __forceinline__ void vm_wait_all()
{
#ifdef __HIPCC__
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0) alone: expcnt and lgkmcnt at their maxima
#endif
}

#ifndef NNN_SYN_MINWAVES
#define NNN_SYN_MINWAVES 4
#endif
template <bool PLAIN>
__global__ void __launch_bounds__(64 * FFT_SPB, NNN_SYN_MINWAVES) k_synth(Buffers b, const StepParams *__restrict__ sp0, int g)
{
    __shared__ FftLds t;
    __shared__ float2 A_[FFT_SPB][NFFT_BUF];   // also the per-bin energies of the band renormalisation (before A is filled)
    __shared__ float r_[FFT_SPB][3 * NB];
    const int wave = threadIdx.x >> 6;
    float2 *A = A_[wave];
    float *r = r_[wave];
    int tile, sub;
    xcd_tile_block((int)blockIdx.x, b.NT, TILE / FFT_SPB, tile, sub);
    if (tile * TILE + sub * FFT_SPB >= b.S) return;   // (a block whose streams are all padding -- the last tile of a batch that is not a multiple of 64 -- has nothing to do)
    if (!live_any(b, tile, sub * FFT_SPB, FFT_SPB)) return;   // (... or all held, nnn_batch_hold_streams)
    const int lane0 = threadIdx.x & 63, sl = sub * FFT_SPB + wave, s = tile * TILE + sl;
    int lane = lane0;
    fft_tables_load(t, b, true);
    float *sm = b.synth_mem + (size_t)s * FRAME;
    float4 smq[2];   // overlap memory as sample quads, carried from frame to frame in registers
#pragma unroll
    for (int u = 0; u < 2; u++) smq[u] = lane + 64 * u < FRAME / 4 ? ((const float4 *)sm)[lane + 64 * u] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    __syncthreads();   // tables in place; from here on every wave is on its own (a silent stream skips the filter)
    BinConst bc;
#pragma unroll
    for (int u = 0; u < 8; u++) {
        const int k = rfft_slot_bin(lane0, u);
        const bool on = k >= 0 && k < 400;
        bc.band[u] = on ? (int)t.band[on ? k : 0] : -1;
        bc.frac[u] = on ? t.frac[bsk(on ? k : 0)] : 0.0f;
    }
    // (a held stream beside live ones, nnn_batch_hold_streams, is handed to the frame body under a padding stream's index: like one, it
    // writes neither audio nor VAD nor frame log, and the caller's bytes stay as they were.  The mask is constant for the call.)
    const int s_out = live_stream(b, tile, sl) ? s : b.S_pad;
    // The frame loop is software-pipelined.  Every global load of a frame is independent of the frame before it, so frame f + 1's inputs --
    // the X and P rows, the five band quantities, the silence flag and the VAD -- are requested inside frame f, into the registers that
    // held frame f's, and a frame starts on data that is on its way or there instead of on two trips to memory in a row (the silence flag's,
    // then everything else's) that only the three other waves of the SIMD cover.  The request goes out behind the inverse transform
    // (synth_frame's TRANSFORMED) and lands under the overlap-add and the next frame's head: the transform's last pass leaves no register
    // free at four waves per SIMD (eight more live values there spill), the stretch behind it leaves forty.
    // The element offsets of a frame's scratch set (NNN_TIF: set f lies f * S_pad * LEN behind set 0) are stepped from frame to frame as
    // wave-uniform values; the addresses are formed where the loads are issued, from the laundered lane.  (sp0 is restrict-qualified -- no
    // kernel writes the parameter table it reads -- so that a frame's parameters are scalar loads: as vector loads at the head of the
    // frame they were counted behind the requests, and the wait for them waited for every request.)
    const int sl_u = __builtin_amdgcn_readfirstlane(sl);   // (the wave's row, in a scalar register)
    const size_t step1 = (size_t)b.S_pad, stepb = step1 * NB, stepx = step1 * FSTR;
    size_t o1 = (size_t)tile * TILE + sl_u, ob = (size_t)tile * TILE * NB + sl_u, ox = o1 * FSTR;   // frame 0's
    float2 Xr[8], Pr[8];
    float b_ex, b_ep, b_xp, b_graw, b_g, vadv;
    int silent;
    // `on` false (behind the group's last frame): nothing is loaded, and nothing of the frame before stays live across the transform
    auto fetch = [&](int ln, bool on) {
        silent = 0;
        vadv = b_ex = b_ep = b_xp = b_graw = b_g = 0.0f;
#pragma unroll
        for (int u = 0; u < 8; u++) Xr[u] = Pr[u] = make_float2(0.0f, 0.0f);
        if (!on) return;
        // in the order the frame's head asks for them (loads return in order): the silence flag, the band quantities, then the spectra
        silent = b.silence[o1];
        if (ln < NB) {
            b_xp = b.exp_[ob + (size_t)ln * TILE];
            b_graw = b.g_raw[ob + (size_t)ln * TILE];
            b_ex = b.ex[ob + (size_t)ln * TILE];
            b_ep = b.ep[ob + (size_t)ln * TILE];
            b_g = b.g[ob + (size_t)ln * TILE];
        }
        vadv = b.vad[o1];
        // (the spectra arrive as the transforms held them, (bin k, bin 480 - k) pairs in 16-byte loads: spectrum_load)
        spectrum_load(b.X + ox, Xr, ln);
        spectrum_load_p(b.P + ox, Pr, ln);
    };
    fetch(lane0, true);
    for (int f = 0; f < g; f++) {
        lane = launder_v(lane0);   // keep the frame loop's addresses inside the loop (see launder_v)
        const bool live = silent == 0;
        synth_frame<false, PLAIN>(b, sp0 + f, f, tile, sl, s_out, lane, t, A, r, Xr, Pr, b_ex, b_ep, b_xp, b_graw, b_g, vadv, live, sm, smq, &bc, [&]() {
            // (the window quads, requested ahead of the transform, are the only loads still counted: have them waited for here, where they
            // have long landed -- loads return in order, and a wait for them behind the requests below would wait for those too)
            vm_wait_all();
            o1 += step1; ob += stepb; ox += stepx;
            fetch(lane, f + 1 < g);
        });
    }
#pragma unroll
    for (int u = 0; u < 2; u++)
        if (lane0 + 64 * u < FRAME / 4) ((float4 *)sm)[lane0 + 64 * u] = smq[u];
}

#pragma clang fp contract(off)

}  // namespace nnn
