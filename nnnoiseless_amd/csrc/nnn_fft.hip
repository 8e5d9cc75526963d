#pragma once
// nnn_fft.hip -- the 960-point transforms and what rides on them: the FFT in LDS, band sums, windows, spectrum I/O, K8 k_fft_xp / k_fft_x and
// xt_rider.  Not a translation unit: nnn_kernels.hip includes it between the pitch stage and the feature stage; the synthesis and the fused
// back end (nnn_back.hip) use its transforms.

namespace nnn {

// ---------------------------------------------------------------------------------------------
// Real 960-point transforms as 480-point complex FFTs in LDS (Stockham autosort, radices 8 x 6 x 10,
// one wave per transform) plus the split/merge step.  The reference's FFT is third-party
// (easyfft 0.4.2 -> realfft 3.5.0 -> rustfft 6.4.1; call sites src/features.rs:264,290),
// un-normalised in both directions.
// ---------------------------------------------------------------------------------------------
// Everything from here to the end of k_fft_x, and k_synth further down, is downstream of an FFT: the reference itself is only
// defined to f32 rounding there (its FFT picks AVX / SSE / scalar code at run time) and parity is a tolerance.  A multiply fuses
// with an add exactly where the source says fmaf (complex products, band sums); nowhere else.  Round 3 let the compiler fuse at
// will in these regions (#pragma clang fp contract(fast): -5 % / -1 % static vector instructions in k_fft_xp / k_synth, no measured
// time, profiles/r3_experiments_ab.txt block A).  Round 4 took that back: the same source then rounds the same way in every kernel
// it is inlined into, and the fused back end (k_back) -- the same transforms and synthesis inside another kernel, where the
// compiler's choices came out differently in a third of the spectrum's bins -- gives the bits of k_fft_xp / k_synth, so a stream
// may change back end from call to call.
constexpr int NFFT = 480;

__device__ __forceinline__ float2 cmulf(float2 a, float2 w)
{
    return make_float2(fmaf(a.x, w.x, -a.y * w.y), fmaf(a.x, w.y, a.y * w.x));
}
__device__ __forceinline__ float2 cadd(float2 a, float2 c) { return make_float2(a.x + c.x, a.y + c.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 c) { return make_float2(a.x - c.x, a.y - c.y); }
__device__ __forceinline__ float2 mul_mi(float2 a) { return make_float2(a.y, -a.x); }  // a * (-i)

__device__ __forceinline__ void bfly2(float2 &a, float2 &c) { float2 t = csub(a, c); a = cadd(a, c); c = t; }

__device__ __forceinline__ void dft8(float2 *v)
{
    const float h = 0.70710678118654752440f;
    float2 a0 = v[0], a1 = v[1], a2 = v[2], a3 = v[3], a4 = v[4], a5 = v[5], a6 = v[6], a7 = v[7];
    bfly2(a0, a4); bfly2(a1, a5); bfly2(a2, a6); bfly2(a3, a7);
    a5 = make_float2((a5.x + a5.y) * h, (a5.y - a5.x) * h);   // * exp(-i pi/4)
    a6 = mul_mi(a6);                                          // * exp(-i pi/2)
    a7 = make_float2((a7.y - a7.x) * h, (-a7.x - a7.y) * h);  // * exp(-3i pi/4)
    bfly2(a0, a2); bfly2(a1, a3); bfly2(a4, a6); bfly2(a5, a7);
    a3 = mul_mi(a3); a7 = mul_mi(a7);
    bfly2(a0, a1); bfly2(a2, a3); bfly2(a4, a5); bfly2(a6, a7);
    v[0] = a0; v[4] = a1; v[2] = a2; v[6] = a3; v[1] = a4; v[5] = a5; v[3] = a6; v[7] = a7;
}

__device__ __forceinline__ void dft3(float2 &v0, float2 &v1, float2 &v2)
{
    const float s = 0.86602540378443864676f;  // sin(2 pi / 3)
    float2 t1 = cadd(v1, v2);
    float2 t2 = csub(v1, v2);
    float2 m = make_float2(fmaf(-0.5f, t1.x, v0.x), fmaf(-0.5f, t1.y, v0.y));
    v0 = cadd(v0, t1);
    // v1 = m + (-i s t2), v2 = m - (-i s t2): the products fused into the sums (written out: the compiler's own contraction is off)
    v1 = make_float2(fmaf(s, t2.y, m.x), fmaf(-s, t2.x, m.y));
    v2 = make_float2(fmaf(-s, t2.y, m.x), fmaf(s, t2.x, m.y));
}

__device__ __forceinline__ void dft5(float2 &v0, float2 &v1, float2 &v2, float2 &v3, float2 &v4)
{
    const float c1 = 0.30901699437494742410f, c2 = -0.80901699437494742410f;  // cos(2pi/5), cos(4pi/5)
    const float s1 = 0.95105651629515357212f, s2 = 0.58778525229247312917f;   // sin(2pi/5), sin(4pi/5)
    float2 a1 = cadd(v1, v4), b1 = csub(v1, v4);
    float2 a2 = cadd(v2, v3), b2 = csub(v2, v3);
    float2 x0 = v0;
    float2 m1 = make_float2(fmaf(c2, a2.x, fmaf(c1, a1.x, x0.x)), fmaf(c2, a2.y, fmaf(c1, a1.y, x0.y)));
    float2 m2 = make_float2(fmaf(c1, a2.x, fmaf(c2, a1.x, x0.x)), fmaf(c1, a2.y, fmaf(c2, a1.y, x0.y)));
    float2 n1 = make_float2(fmaf(s2, b2.y, s1 * b1.y), -fmaf(s2, b2.x, s1 * b1.x));   // -i (s1 b1 + s2 b2)
    float2 n2 = make_float2(fmaf(-s1, b2.y, s2 * b1.y), -fmaf(-s1, b2.x, s2 * b1.x));  // -i (s2 b1 - s1 b2)
    v0 = make_float2(x0.x + a1.x + a2.x, x0.y + a1.y + a2.y);
    v1 = cadd(m1, n1);
    v4 = csub(m1, n1);
    v2 = cadd(m2, n2);
    v3 = csub(m2, n2);
}

// 6 = 2 x 3 and 10 = 2 x 5 by the prime-factor map (no inner twiddles):
// input n = (N2 n1 + 2 n2) mod N, output k = (N2 k1 + c k2) mod N with c = 4 (N = 6) or 6 (N = 10).
__device__ __forceinline__ void dft6(float2 *v)
{
    float2 a0 = v[0], a1 = v[2], a2 = v[4], b0 = v[3], b1 = v[5], b2 = v[1];
    dft3(a0, a1, a2);
    dft3(b0, b1, b2);
    v[0] = cadd(a0, b0); v[3] = csub(a0, b0);
    v[4] = cadd(a1, b1); v[1] = csub(a1, b1);
    v[2] = cadd(a2, b2); v[5] = csub(a2, b2);
}

__device__ __forceinline__ void dft10(float2 *v)
{
    float2 a0 = v[0], a1 = v[2], a2 = v[4], a3 = v[6], a4 = v[8];
    float2 b0 = v[5], b1 = v[7], b2 = v[9], b3 = v[1], b4 = v[3];
    dft5(a0, a1, a2, a3, a4);
    dft5(b0, b1, b2, b3, b4);
    v[0] = cadd(a0, b0); v[5] = csub(a0, b0);
    v[6] = cadd(a1, b1); v[1] = csub(a1, b1);
    v[2] = cadd(a2, b2); v[7] = csub(a2, b2);
    v[8] = cadd(a3, b3); v[3] = csub(a3, b3);
    v[4] = cadd(a4, b4); v[9] = csub(a4, b4);
}

template <int R> __device__ __forceinline__ void dftR(float2 *v)
{
    if (R == 8) dft8(v);
    else if (R == 6) dft6(v);
    else dft10(v);
}

// The wave = stream transform kernels run FFT_SPB streams per block (one wave each) so that the block's waves share
// one copy of the read-only tables in LDS: every table read sits on a wave's dependent chain, and from LDS it costs
// ~100 cycles instead of a trip to L2.  After the tables are in place (one __syncthreads) the waves never meet again:
// each synchronises only with itself (wave_lds_sync) on its own LDS region.
constexpr int FFT_SPB = 4;
// Per-bin arrays that the band sums read (lane = a segment of <= 8 consecutive bins: neighbouring lanes 8 floats apart, every
// read 8-way bank-conflicted) are kept skewed, bin k at k + k / 8: neighbouring
// lanes then sit 9 floats apart.  Lanes that walk the bins in order (k = lane + 64 u) pay nothing: the skew of their index is a
// per-lane constant.  k_fft_xp 19.6 -> 18.9 us per frame at 4096 streams, 325 -> 321 at 65536 (same box).
__device__ __forceinline__ int bsk(int k) { return k + (k >> 3); }
constexpr int BSK_LEN = 400 + 400 / 8;
// Lane twiddles (since round 5): the second and third pass's twiddles as the lanes use them -- a
// lane's twiddles are constants of the lane, one LDS read each instead of index, wrap and sign (five vector instructions a piece) -- in
// k_synth, whose blocks copy the tables once per group of frames (-6.6 % vector instructions, -1.5 % time: profiles/r4_experiments_ab.txt M,
// profiles/r5_experiments_ab.txt C); the kernels whose blocks copy the tables per stream-frame keep the half circle and copy the part of
// the image before these tables only.  Same products of the same factors: bit-identical to the variant without.
constexpr int FFT_TW2 = 2 * 5 * 64, FFT_TW3 = 9 * 64;
struct alignas(16) FftLds {
    float2 tw[NFFT];           // exp(-2 pi i k / 960), k < 480; the other half of the circle is the negation
    float frac[BSK_LEN];       // triangular band weights (ref: src/lib.rs:65-82), skewed (bsk)
    unsigned char band[400];   // band of each bin
    short seg[256];            // band-sum segmentation (see band_sums_par): k0[64], count[64], first segment[32] and segments[32] per
                               // interval, [192 + s]: segments behind segment s in its interval
    float dct[NB * NB];        // DCT table (ref: src/lib.rs:118-127): the feature head's two transforms read 44 of its rows per stream-frame
                               // (from global memory they were half of k_fft_xp's vector-memory instructions; same time either way)
    float pad_[2];
    float2 tw2[FFT_TW2];       // fft_pass<6, 8>: [it][r - 1][lane]; copied only by the kernels that use them (fft_tables_load)
    float2 tw3[FFT_TW3];       // fft_pass<10, 48>: [r - 1][lane]
};
static_assert(sizeof(FftLds) % 16 == 0, "copied as 16-byte pieces");
constexpr int FFT_TABLES_SHORT = (int)offsetof(FftLds, tw2);
static_assert(FFT_TABLES_SHORT % 16 == 0, "");
// Fills the block's tables from the image the host built in exactly this layout (Buffers::fft_img): a straight copy of 16-byte
// pieces.  (Building them in the kernel from the plain tables -- skewed index, byte and short conversions, scattered narrow LDS
// stores -- cost k_fft_xp 190 of its 1530 vector instructions per stream-frame.)  Every thread of the block calls it, the caller
// synchronises.
__device__ __forceinline__ void fft_tables_load(FftLds &t, const Buffers &b, bool lane_tw = false)
{
    const int tid = threadIdx.x, nt = blockDim.x;
    const uint4 *src = (const uint4 *)b.fft_img;
    uint4 *dst = (uint4 *)&t;
    const int n = (lane_tw ? (int)sizeof(FftLds) : FFT_TABLES_SHORT) / 16;
    // every piece a thread copies is requested before the first one is stored: one trip to the L2 per block instead of one per piece
    // (until round 5 the loop waited for each load before it asked for the next: three to five trips on the block's critical path)
    constexpr int MAXIT = 5;   // blocks of >= 256 threads
    static_assert(sizeof(FftLds) / 16 <= (size_t)MAXIT * 256, "");
    uint4 r[MAXIT];
#pragma unroll
    for (int k = 0; k < MAXIT; k++) {
        const int i = tid + k * nt;
        if (i < n) r[k] = ld_global_u4(src + i);
    }
#pragma unroll
    for (int k = 0; k < MAXIT; k++) {
        const int i = tid + k * nt;
        if (i < n) dst[i] = r[k];
    }
    for (int i = tid + MAXIT * nt; i < n; i += nt) dst[i] = ld_global_u4(src + i);   // blocks of fewer than 256 threads: the rest, piece by piece
}
// the host's side of it
__host__ inline void fft_tables_image(FftLds &t, const float2 *tw960, const float *bin_frac, const int *bin_band, const int *seg, const float *dct)
{
    memset(&t, 0, sizeof(t));
    for (int i = 0; i < NB * NB; i++) t.dct[i] = dct[i];
    for (int i = 0; i < NFFT; i++) t.tw[i] = tw960[i];
    auto at = [&](int k) { const float2 w = tw960[k >= NFFT ? k - NFFT : k]; return k >= NFFT ? make_float2(-w.x, -w.y) : w; };   // tw960_at
    for (int it = 0; it < 2; it++)       // fft_pass<6, 8>: butterfly j = lane + 64 it < 80, k = j % 8, twiddle (r k 20) % 960
        for (int r = 1; r < 6; r++)
            for (int l = 0; l < 64; l++) t.tw2[(it * 5 + r - 1) * 64 + l] = at((r * ((l + 64 * it) % 8) * 20) % 960);
    for (int r = 1; r < 10; r++)         // fft_pass<10, 48>: butterfly j = lane < 48, k = j, twiddle (r k 2) % 960
        for (int l = 0; l < 64; l++) t.tw3[(r - 1) * 64 + l] = at((r * (l % 48) * 2) % 960);
    for (int i = 0; i < 400; i++) {
        t.frac[i + (i >> 3)] = bin_frac[i];
        t.band[i] = (unsigned char)bin_band[i];
    }
    for (int i = 0; i < 192; i++) t.seg[i] = (short)seg[i];
    for (int iv = 0; iv < NB - 1; iv++)
        for (int i = 0; i < seg[160 + iv]; i++) t.seg[192 + seg[128 + iv] + i] = (short)(seg[160 + iv] - 1 - i);
}
__device__ __forceinline__ float2 tw960_at(const float2 *tw, int k)   // k in [0, 960)
{
    const float2 w = tw[k >= NFFT ? k - NFFT : k];
    return k >= NFFT ? make_float2(-w.x, -w.y) : w;
}

// one Stockham pass of the 480-point transform, in place: every lane pulls its butterflies into registers,
// the wave synchronises, then scatters the results (autosort order).  Radix R, NS = product of the radices
// already applied; tw = the LDS half-table of exp(-2 pi i k / 960).  One buffer per transform keeps LDS small
// enough for a full complement of waves per CU.
// The first pass scatters with a stride of 8 elements (64 bytes): 32 lanes on 4 bank pairs, every store 8-way conflicted
// -- as many LDS cycles as all other accesses of the transform together.  Its output (and the second pass's input) is
// therefore skewed, element i at i + i / 8 (stride 9: conflict-free); the buffer holds NFFT_BUF elements for that.
// The second pass's output (the third's input) is padded the same way for the same reason (round 5): its butterflies j and j + 8 of one
// 16-lane store group wrote elements 48 apart -- the same banks -- so every block of 48 elements now starts 8 further on (element i at
// i + 8 (i / 48), 552 elements): the two halves of a store group sit 56 apart, 8 modulo 16, and the third pass reads with stride 56.
constexpr int NFFT_BUF = 560;
constexpr int FFT_P2PAD = 8;
// LT: `tw` is the pass's own per-lane twiddle table ([it][r - 1][lane], FftLds::tw2 / tw3) instead of the half circle
template <int R, int NS, bool SKEW_IN, bool SKEW_OUT, bool LT = false>
__device__ __forceinline__ void fft_pass(float2 *buf, const float2 *tw, int lane)
{
    constexpr int NBF = NFFT / R, IT = (NBF + 63) / 64;
    constexpr bool PAD_OUT = NS == 8 && R == 6, PAD_IN = NS == 48 && R == 10;   // the second pass's padded output = the third's input
    static_assert(!PAD_IN || NBF == 48, "");
    static_assert(!SKEW_IN || NBF % 8 == 0, "skewed reads assume r * NBF is a multiple of 8");
    static_assert(!SKEW_OUT || (NS == 1 && R == 8), "skewed writes are the first pass's");
    float2 v[IT][R];
#pragma unroll
    for (int it = 0; it < IT; it++) {
        const int j = lane + 64 * it;
        if (j < NBF) {
            const int k = j % NS;
            const int jj = SKEW_IN ? j + (j >> 3) : j;
#pragma unroll
            for (int r = 0; r < R; r++) v[it][r] = buf[jj + (SKEW_IN ? r * NBF + r * NBF / 8 : (PAD_IN ? r * (NBF + FFT_P2PAD) : r * NBF))];
            if (NS > 1) {
                constexpr int step = 960 / (NS * R);
#pragma unroll
                for (int r = 1; r < R; r++) v[it][r] = cmulf(v[it][r], LT ? tw[(it * (R - 1) + r - 1) * 64 + lane] : tw960_at(tw, (r * k * step) % 960));
            }
            dftR<R>(v[it]);
        }
    }
    wave_lds_sync();
#pragma unroll
    for (int it = 0; it < IT; it++) {
        const int j = lane + 64 * it;
        if (j < NBF) {
            const int base = SKEW_OUT ? 9 * j : (j / NS) * (NS * R + (PAD_OUT ? FFT_P2PAD : 0)) + (j % NS);   // skewed: element 8 j + r at 9 j + r
#pragma unroll
            for (int r = 0; r < R; r++) buf[base + r * NS] = v[it][r];
        }
    }
    wave_lds_sync();
}

// forward 480-point FFT in place (natural order in, natural order out); buf has room for NFFT_BUF elements
__device__ __forceinline__ void fft480(float2 *buf, const float2 *tw, int lane)
{
    fft_pass<8, 1, false, true>(buf, tw, lane);
    fft_pass<6, 8, true, false>(buf, tw, lane);
    fft_pass<10, 48, false, false>(buf, tw, lane);
}
// The same with the input handed over in registers in the first pass's own order -- lane j < 60 holds elements j + 60 r, r < 8
// (lanes 60..63 hold anything) -- instead of staged in buf: both callers can produce their input in that order, which saves the
// staging store, the first pass's reads and a synchronisation per transform.  Every earlier reader of buf must be done.
// RL (the fused back end, a wave of 128 registers that also holds two spectra): the lane index is laundered between the passes, so that
// each pass forms its LDS addresses and twiddle indices where it starts instead of all of them up front (see launder_v)
template <bool RL = false, bool LT = false>
__device__ __forceinline__ void fft480_regs(float2 (&v)[8], float2 *buf, const float2 *tw, int lane)
{
    dft8(v);
    if (lane < NFFT / 8) {
#pragma unroll
        for (int r = 0; r < 8; r++) buf[9 * lane + r] = v[r];   // skewed, as fft_pass<8, 1, false, true> leaves it
    }
    wave_lds_sync();
    if (RL) lane = launder_v(lane);
    if (LT) {   // (tw = FftLds::tw of a block that copied the whole image)
        const float2 *tw2 = (const float2 *)((const char *)tw + (offsetof(FftLds, tw2) - offsetof(FftLds, tw)));
        fft_pass<6, 8, true, false, true>(buf, tw2, lane);
        if (RL) lane = launder_v(lane);
        fft_pass<10, 48, false, false, true>(buf, tw2 + FFT_TW2, lane);
        return;
    }
    fft_pass<6, 8, true, false>(buf, tw, lane);
    if (RL) lane = launder_v(lane);
    fft_pass<10, 48, false, false>(buf, tw, lane);
}
constexpr int FFT_P1 = NFFT / 8;   // butterflies (= lanes at work) of the first pass

// band sums in the reference's accumulation order (ref: src/lib.rs:65-82): out[b] first receives
// the frac-weighted terms of interval b-1, then the (1-frac)-weighted terms of interval b.
__device__ __forceinline__ float band_sum(const float *v, int bnd, const float *bin_frac)
{
    const int e_lo = bnd >= 1 ? kEband[bnd - 1] : 0, e_mid = kEband[bnd], e_hi = bnd < NB - 1 ? kEband[bnd + 1] : 0;
    float acc = 0.0f;
    if (bnd >= 1)
        for (int k = 4 * e_lo; k < 4 * e_mid; k++) acc += bin_frac[k] * v[k];
    if (bnd < NB - 1)
        for (int k = 4 * e_mid; k < 4 * e_hi; k++) acc += (1.0f - bin_frac[k]) * v[k];
    if (bnd == 0 || bnd == NB - 1) acc *= 2.0f;
    return acc;
}

// Parallel band sums for tolerance-only quantities (every band energy is downstream of an FFT): the 21 band intervals are cut
// into 54 segments of 4 or 8 bins (table t.seg; an 8-bin segment starts on a multiple of 8, so a segment's bins are contiguous
// in the skewed arrays too).  Lane = segment forms the two triangularly weighted partial sums of its bins for up to NQ
// quantities -- eight unrolled steps, the shorter segments masked; the segments of an interval sit on consecutive lanes and are
// summed across lanes by a segmented suffix sum (four shuffle rounds: intervals have at most 11 segments); lane = band then takes
// the frac-weighted total of the interval below it and the (1 - frac)-weighted total of its own (ref: src/lib.rs:65-82).
// (Until round 3 the partial sums went through LDS and lane = band looped over up to 11 of them, twice: with the per-bin loop
// that was a third of k_fft_xp's vector instructions, issued for 22 or 54 of 64 lanes.)  Every lane of the wave must call it.
template <int NQ>
__device__ __forceinline__ void band_sums_par(const FftLds &t, const float *const (&v)[NQ], float (&out)[NQ], int lane)
{
    const short *seg = t.seg;
    // lane = slot: k0, bin count (0: an idle slot) and the number of the interval's segments behind this one.  The slots of an interval
    // never straddle a row of 16 lanes (the host leaves slots idle for that, 59 of 64 in use), so the suffix sum's four rounds are DPP
    // row moves (round 5: they were wave shuffles -- an index computation and an LDS-crossbar trip each).
    const int k0 = seg[lane], cnt = seg[64 + lane], rem = seg[192 + lane];
    const int ks0 = bsk(k0);
    float pa[NQ], pb[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) { pa[q] = 0.0f; pb[q] = 0.0f; }
#pragma unroll
    for (int u = 0; u < 8; u++) {
        const float fr = t.frac[ks0 + u], om = 1.0f - fr;
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            float x = v[q][ks0 + u];
            x = u < cnt ? x : 0.0f;
            pa[q] = fmaf(om, x, pa[q]);
            pb[q] = fmaf(fr, x, pb[q]);
        }
    }
    // segmented suffix sum: afterwards the first segment of every interval holds the interval's totals
#define NNN_SUFFIX_ROUND(D)                                                          \
    _Pragma("unroll") for (int q = 0; q < NQ; q++) {                                 \
        const float ta = dpp_row_down<D>(pa[q]), tb = dpp_row_down<D>(pb[q]);        \
        pa[q] += rem >= D ? ta : 0.0f;                                               \
        pb[q] += rem >= D ? tb : 0.0f;                                               \
    }
    NNN_SUFFIX_ROUND(1) NNN_SUFFIX_ROUND(2) NNN_SUFFIX_ROUND(4) NNN_SUFFIX_ROUND(8)
#undef NNN_SUFFIX_ROUND
    // lane = band: interval `lane - 1` from below, interval `lane` above
    const int bnd = lane < NB ? lane : 0;
    const int lo = seg[128 + (bnd >= 1 ? bnd - 1 : 0)], hi = seg[128 + (bnd < NB - 1 ? bnd : 0)];
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        const float fb = wave_read(pb[q], lo), fa = wave_read(pa[q], hi);
        float o = (bnd >= 1 ? fb : 0.0f) + (bnd < NB - 1 ? fa : 0.0f);
        if (bnd == 0 || bnd == NB - 1) o *= 2.0f;
        out[q] = lane < NB ? o : 0.0f;
    }
}

// ---------------------------------------------------------------------------------------------
// K8  fft_xp: transform_input (window, real FFT, normalise, band energy) at lag 0 and at lag = pitch, one after the
//     other in the same wave: X never leaves the registers between its own transform and the band correlation with P
//     (ref: src/features.rs:119-135, 281-298, src/lib.rs:65-82, 150-155).  One wave per stream, one launch per frame
//     group.  Ends with the head of the feature stage (ref: src/features.rs:135-170).  WITH_P = false: the lag-0
//     transform and its band energies only (the clean / noise states of the training rows).
// ---------------------------------------------------------------------------------------------
// one DCT output (ref: src/lib.rs:139-148): sequential sum over the 22 inputs, scaled in double
__device__ __forceinline__ float dct_out(const float *x, const float *dct, int i)
{
    float sum = 0.0f;
#pragma unroll
    for (int j = 0; j < NB; j++) sum += x[j] * dct[j * NB + i];
    return (float)((double)sum * 0.30151134457776363 /* sqrt(2/22) */);
}

struct __attribute__((packed, aligned(4))) SamplePair { float x, y; };   // two consecutive samples: one 8-byte load at 4-byte alignment
// windowed 960 samples ending `lag` samples before the newest one -> Z (packed as 480 complex), transform in place,
// spectrum bins into Y (lane owns bins lane + 64 u), scaled by wnorm
// the 960 samples ending `lag` samples before the newest one, as the sample pairs n = j + 60 r of the transform's first pass
__device__ __forceinline__ void window_load(const float *h, int ring, int rb, int lag, int lane, SamplePair (&sm)[8])
{
    int start = rb + (HIST - WINDOW) - lag;   // in (0, 2 ring)
    if (start >= ring) start -= ring;
    const int j = lane < FFT_P1 ? lane : FFT_P1 - 1;   // (lanes 60..63 shadow lane 59 and store nothing)
    // Pair r sits 8 FFT_P1 r bytes behind pair 0, less the ring's length when that is past the ring's end: of x and x - 4 ring taken as
    // unsigned numbers the smaller is the one in range.  Three 32-bit instructions per pair and an offset the load adds to the
    // stream's (wave-uniform) base itself; as signed indices with a compare and a 64-bit address each, it was seven.
    const unsigned x0 = 4u * (unsigned)(start + 2 * j), ring4 = 4u * (unsigned)ring;
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const unsigned x = x0 + (unsigned)(8 * FFT_P1 * r), y = x - ring4;
        sm[r] = *(const SamplePair *)((const char *)h + (x < y ? x : y));   // (the pair that starts on the ring's last sample reads the copy of sample 0 kept behind it)
    }
}
template <bool RL = false>
__device__ __forceinline__ void window_rfft(const Buffers &b, const SamplePair (&sm)[8], const float2 (&w)[8], const FftLds &t,
                                            float2 *Z, float2 (&Y)[8], int lane, bool first)
{
    // sample pairs n = j + 60 r straight into the first pass's registers (w holds the window in the same order)
    float2 v[8];
#pragma unroll
    for (int r = 0; r < 8; r++) v[r] = make_float2(sm[r].x * w[r].x, sm[r].y * w[r].y);
    if (first) __syncthreads();   // tables in place; from here on every wave is on its own
    fft480_regs<RL>(v, Z, t.tw, lane);
    if (RL) lane = launder_v(lane);
    // Bins k and 480 - k come from the same two transform outputs (E[480 - k] = conj E[k], O[480 - k] = conj O[k], the twiddle
    // of 480 - k is -conj of k's): a lane takes them as a pair -- one read of each output, one twiddle, one complex product for
    // both -- and owns bins rfft_slot_bin(lane, u): k = lane + 64 u in slots u < 4 (k <= 240), 480 - k in slot 4 + u (k < 240).
    // (the split step's factor 1/2 rides on the analysis window, Buffers::window_a -- an exact scaling.  The normalisation 1 / 480
    // stays here: folded into the window as well it rounds every coefficient a second time, a window that is no longer the
    // reference's bit for bit, and on a signal with a huge slowly decaying component -- the high-passed DC step of the edge-case
    // set -- the leakage of that component differs enough to move the gains by three times the reference's own f32 / f64 spread.)
    const float wn = b.wnorm;
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int k = lane + 64 * u;
        if (k <= NFFT / 2) {
            const float2 zk = Z[k], zn = Z[k ? NFFT - k : 0];
            const float2 e = make_float2(zk.x + zn.x, zk.y - zn.y);
            const float2 o = make_float2(zk.y + zn.y, -(zk.x - zn.x));   // (zk - conj zn) / i
            const float2 wo = cmulf(o, t.tw[k]);
            Y[u] = make_float2((e.x + wo.x) * wn, (e.y + wo.y) * wn);
            Y[4 + u] = make_float2((e.x - wo.x) * wn, -(e.y - wo.y) * wn);   // conj(E - W O)
        }
    }
    wave_lds_sync();   // the transform has been read: its buffer now takes the per-bin products for the band sums
}
// bin of slot u of a lane's spectrum registers (see window_rfft); -1: an empty slot
__device__ __forceinline__ int rfft_slot_bin(int lane, int u)
{
    const int k = lane + 64 * (u & 3);
    if (u < 4) return k <= NFFT / 2 ? k : -1;
    return k < NFFT / 2 ? NFFT - k : -1;
}

// What the fused back end (k_back, nnn_back.hip) keeps of a frame's transforms instead of sending it through HBM: both spectra in the
// registers of the stream's wave (slot order of window_rfft), the three per-band quantities the pitch filter needs on lanes 0..21, the
// silence flag; the feature head's 28 outputs go to `cnw` (LDS) for the feature stage that follows on the same wave.
struct XpKeep {
    float2 X[8], P[8];
    float ex, ep, xn;     // lane < NB: band energies of X and P, normalised correlation
    int silent;           // wave-uniform
    int sl;               // in: the stream's row in its tile
    float *cnw;           // in: LDS staging of the frame's cepstrum (22) + pitch-correlation DCT (6)
    int *flag;            // in: one LDS word of the wave (the silence flag travels through it)
};
// a spectrum in the wave's registers (slot order, see window_rfft) <-> its row in memory: pair (slot u, slot 4 + u) = (bin k, bin 480 - k)
// of lane j's k = j + 64 u as one 16-byte access at float4 index 64 u + j (FSTR in nnn_layout.h)
__device__ __forceinline__ void spectrum_store(float2 *row, const float2 (&S)[8], int lane)
{
#pragma unroll
    for (int u = 0; u < 4; u++)
        if (lane + 64 * u <= NFFT / 2) ((float4 *)row)[64 * u + lane] = make_float4(S[u].x, S[u].y, S[4 + u].x, S[4 + u].y);
}
__device__ __forceinline__ void spectrum_load(const float2 *row, float2 (&S)[8], int lane)
{
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const float4 v = lane + 64 * u <= NFFT / 2 ? ((const float4 *)row)[64 * u + lane] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        S[u] = make_float2(v.x, v.y);
        S[4 + u] = make_float2(v.z, v.w);
    }
}

// The pitch-lagged spectrum P the same way, except that the partners of slot 0 -- bins 417 .. 480, which the pitch filter never reads (its
// gain is zero from bin 400 up, ref: src/lib.rs:84-97) -- stay out of the row: 64 lone bins (8 bytes each) first, then the pairs of slots
// 1 .. 3; with the parity taps on the 64 partners follow behind (P_TAIL).  13 % fewer bytes for P than whole pairs.
constexpr int P_PAIRS0 = 64, P_TAIL = 64 + 2 * 177;   // float2 index of the first pair (slot 1) and of the taps-only partners of slot 0
__device__ __forceinline__ void spectrum_store_p(float2 *row, const float2 (&S)[8], int lane, bool taps)
{
    row[lane] = S[0];
    if (taps) row[P_TAIL + lane] = S[4];
#pragma unroll
    for (int u = 1; u < 4; u++)
        if (lane + 64 * u <= NFFT / 2) ((float4 *)(row + P_PAIRS0))[64 * (u - 1) + lane] = make_float4(S[u].x, S[u].y, S[4 + u].x, S[4 + u].y);
}
__device__ __forceinline__ void spectrum_load_p(const float2 *row, float2 (&S)[8], int lane)
{
    S[0] = row[lane];
    S[4] = make_float2(0.0f, 0.0f);   // (bins 417 .. 480: never read)
#pragma unroll
    for (int u = 1; u < 4; u++) {
        const float4 v = lane + 64 * u <= NFFT / 2 ? ((const float4 *)(row + P_PAIRS0))[64 * (u - 1) + lane] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        S[u] = make_float2(v.x, v.y);
        S[4 + u] = make_float2(v.z, v.w);
    }
}

#ifndef NNN_FH_STRIDE
#define NNN_FH_STRIDE 24
#endif
constexpr int FH_STRIDE = NNN_FH_STRIDE;   // floats between the feature head's three staged band arrays (22 used of each)
static_assert(FH_STRIDE >= NB, "");
// XR (fused, one-frame calls): X and its band energies are in memory already -- computed by rider blocks of k_pitch's launch, which needs
// nothing of what the pitch analysis finds (xt_rider) -- and are fetched instead of computed.
// SPECTRA false (k_fft_feat, the VAD-only calls): nobody reads X and P behind this launch, and they are not stored.
template <bool WITH_P, bool FUSED = false, bool XR = false, bool SPECTRA = true>
__device__ __forceinline__ void transform_inputs(const Buffers &b, const StepParams *sp, int tile_in, int sub, FftLds &t, float2 *Z, float *part,
                                                 XpKeep *keep = nullptr)
{
    int tile = tile_in;
    // (fused: the lane index is laundered again between the stages -- see launder_v -- so that the addresses of a later stage are formed
    // where it starts instead of at the top of the function, where the first build kept dozens of them alive in spilled registers)
    int lane = threadIdx.x & 63;
    int sl = FUSED ? keep->sl : sub * FFT_SPB + (int)(threadIdx.x >> 6), s = tile * TILE + sl;
#define NNN_FUSED_RELAUNDER() do { if (FUSED) { lane = launder_v(lane); tile = launder_s(tile); sl = launder_s(sl); s = tile * TILE + sl; } } while (0)
    const int ring = ring_len(b.nslot), rb = ring_base(sp->slot, b.nslot);
    float2 w[8];   // the window at sample pairs j + 60 r: the order of the transforms' first pass (window_rfft)
#pragma unroll
    for (int r = 0; r < 8; r++) w[r] = ((const float2 *)b.window_a)[(lane < FFT_P1 ? lane : FFT_P1 - 1) + FFT_P1 * r];
    const int lag = WITH_P ? NNN_TI(b.pitch, 1, tile, sl)[0] : 0;
    if (!FUSED) fft_tables_load(t, b);   // (the fused kernel loads them once per launch)
    const float *h = b.hist + (size_t)__builtin_amdgcn_readfirstlane(s) * hist_stride(b.nslot);   // (wave = stream: a scalar base)
    // both windows' samples are requested now: the second transform's used to be requested when it started, a trip to memory on
    // the wave's critical path per stream-frame (these kernels move enough bytes for that to show)
    SamplePair sx[8], spw[8];
    if (!XR) window_load(h, ring, rb, 0, lane, sx);
    if (WITH_P && !FUSED) window_load(h, ring, rb, lag, lane, spw);   // (fused: sixteen registers it has not got; requested after the first transform)
    float2 X[8];
    float2 *dx = b.X + (size_t)s * FSTR;
    if (XR) spectrum_load(dx, X, lane);
    else window_rfft<FUSED>(b, sx, w, t, Z, X, lane, !FUSED);
    if (SPECTRA && !XR && (!FUSED || b.taps)) spectrum_store(dx, X, lane);   // (fused: the spectra stay in registers; memory sees them for the parity taps only)
    NNN_FUSED_RELAUNDER();
    float *vv = (float *)Z, *vc = vv + BSK_LEN;   // per-bin quantities of the band sums, skewed (bsk)
    float exv;
    if (XR) {
        exv = lane < NB ? NNN_TI(b.ex, NB, tile, sl)[(size_t)lane * TILE] : 0.0f;
    } else {
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int k = rfft_slot_bin(lane, u);
            if (k >= 0 && k < 400) vv[bsk(k)] = fmaf(X[u].y, X[u].y, X[u].x * X[u].x);
        }
        wave_lds_sync();
        const float *const v[1] = {vv};
        float o[1];
        band_sums_par<1>(t, v, o, lane);
        exv = o[0];
        if (lane < NB) NNN_TI(b.ex, NB, tile, sl)[(size_t)lane * TILE] = exv;
    }
    if (!WITH_P) return;
    wave_lds_sync();
    NNN_FUSED_RELAUNDER();
    float2 Y[8];
    if (FUSED) window_load(b.hist + (size_t)__builtin_amdgcn_readfirstlane(s) * hist_stride(b.nslot), ring, rb, lag, lane, spw);
    if (FUSED || !SPECTRA) {   // (the window again, from the L2: sixteen registers less across the first transform and the band sums of a wave that has 128;
                               // k_fft_feat: without it two of X's values spill across the second transform at 96 registers)
#pragma unroll
        for (int r = 0; r < 8; r++) w[r] = ((const float2 *)b.window_a)[(lane < FFT_P1 ? lane : FFT_P1 - 1) + FFT_P1 * r];
    }
    window_rfft<FUSED>(b, spw, w, t, Z, Y, lane, false);
    float2 *dp = b.P + (size_t)s * FSTR;
    if (SPECTRA && (!FUSED || b.taps)) spectrum_store_p(dp, Y, lane, b.taps != 0);
#pragma unroll
    for (int u = 0; u < 8; u++) {
        const int k = rfft_slot_bin(lane, u);
        if (k >= 0 && k < 400) {
            vv[bsk(k)] = fmaf(Y[u].y, Y[u].y, Y[u].x * Y[u].x);
            vc[bsk(k)] = fmaf(X[u].y, Y[u].y, X[u].x * Y[u].x);
        }
    }
    wave_lds_sync();
    NNN_FUSED_RELAUNDER();
    const float *const v[2] = {vv, vc};
    float o[2];
    band_sums_par<2>(t, v, o, lane);
    // Head of the feature stage (ref: src/features.rs:135-170), here because everything it needs is at hand and this
    // launch covers a whole frame group: the correlation normalised by the band energies, the floored log energies,
    // the silence test, and the two DCTs -- lane = band.  Same operations in the same order as when one lane did it all.
    wave_lds_sync();
    NNN_FUSED_RELAUNDER();
    float *xc = part, *ly = part + FH_STRIDE, *exl = part + 2 * FH_STRIDE;
    float lyv = -2.0f, xnv = 0.0f;
    if (lane < NB) {
        const float xn = o[1] / sqrtf(0.001f + exv * o[0]);
        xnv = xn;
        NNN_TI(b.ep, NB, tile, sl)[(size_t)lane * TILE] = o[0];
        NNN_TI(b.exp_, NB, tile, sl)[(size_t)lane * TILE] = xn;
        xc[lane] = xn;
        exl[lane] = exv;
        lyv = log10f(1e-2f + exv);
    }
    // The floors of the log energies (ref: src/features.rs:150-158) are a 22-step recurrence -- l_i = max(ly_i, max_{j<i} l_j - 7,
    // follow_i - 1.5) with follow decaying by 1.5 per band -- that one lane used to walk while the wave waited.  Unrolled it is
    // l_i = max over j <= i of ly_j - c(i - j) with c(0) = 0, c(d) = min(7, 1.5 d) (c is subadditive, so floors of floors add
    // nothing), plus the two start values; and since c(d) = 7 from d = 5 on: four neighbours and a prefix maximum five bands
    // back, lane = band, through shuffles.  Same values up to the rounding of the decay (one multiply instead of repeated
    // subtraction); a NaN energy is ignored by the max exactly as in the recurrence.  (Every lane takes part in the shuffles.)
    float lfl;
    {
        float pm = lyv;   // inclusive prefix maximum over the bands below (lanes past the bands hold -2: never above a log energy)
#pragma unroll
        for (int d = 1; d < 32; d *= 2) {
            const float tt = wave_read(pm, lane - d);   // (lanes below d read some other lane and keep their own value)
            pm = lane >= d ? fmaxf(pm, tt) : pm;
        }
        float m = fmaxf(fmaxf(lyv, -2.0f - 7.0f), -2.0f - 1.5f * (float)(lane + 1));
#pragma unroll
        for (int d = 1; d <= 4; d++) {
            const float tt = wave_read(lyv, lane - d) - 1.5f * (float)d;
            m = lane >= d ? fmaxf(m, tt) : m;
        }
        const float t5 = wave_read(pm, lane - 5) - 7.0f;
        lfl = lane >= 5 ? fmaxf(m, t5) : m;
    }
    if (lane < NB) ly[lane] = lfl;
    wave_lds_sync();
    if (lane == 0) {   // the silence test on the band energies summed in band order (ref: src/features.rs:160)
        float e = 0.0f;
#pragma unroll
        for (int i = 0; i < NB; i++) e += exl[i];
        NNN_TI(b.silence, 1, tile, sl)[0] = e < 0.04f ? 1 : 0;
        if (FUSED) keep->flag[0] = e < 0.04f ? 1 : 0;
    }
    // the two DCTs side by side: lanes 0..21 the cepstrum of the floored log energies, lanes 32..37 the first six coefficients
    // of the pitch correlation (ref: src/features.rs:141-147, 167-169; src/lib.rs:139-148)
    {
        const bool second = lane >= 32;
        const int i = second ? lane - 32 : lane;
        if (i < (second ? 6 : NB)) {
            float *cn = NNN_TI(b.cn, 28, tile, sl);
            float c = dct_out(second ? xc : ly, t.dct, i);
            if (second) c -= i == 0 ? 1.3f : (i == 1 ? 0.9f : 0.0f);
            else c -= i == 0 ? 12.0f : (i == 1 ? 4.0f : 0.0f);
            if (FUSED) keep->cnw[(second ? NB : 0) + i] = c;   // (the feature stage follows on this wave)
            else cn[(size_t)((second ? NB : 0) + i) * TILE] = c;
        }
    }
    if (FUSED) {
#pragma unroll
        for (int u = 0; u < 8; u++) { keep->X[u] = X[u]; keep->P[u] = Y[u]; }
        keep->ex = exv;
        keep->ep = o[0];
        keep->xn = xnv;
        wave_lds_sync();
        keep->silent = keep->flag[0];
    }
#undef NNN_FUSED_RELAUNDER
}

// five waves per SIMD (96 registers, no spill) and, with LDS kept to 27.6 KB per block, five blocks per CU: k_fft_xp -3.8 % against four
// (profiles/r5_experiments_ab.txt Q)
#ifndef NNN_FFT_MINWAVES
#define NNN_FFT_MINWAVES 5
#endif
// Block index -> (frame, tile, four streams of the tile) for the g frames of a group.  Batches of a multiple of 8 tiles: the blocks an
// XCD receives (i mod 8, in index order) are the g frames of one quartet of streams, then the next quartet's, tile t on XCD t mod 8:
// consecutive frames of a stream share three quarters of the history samples their two windows read, and blocks that run
// side by side on one XCD fetch them into its L2 once (frame-major order -- all streams of frame 0, then frame 1 ... -- puts
// 250 MB of other streams' samples between two uses of a line).
__device__ __forceinline__ void fft_block(const Buffers &b, int g, int &frame, int &tile, int &sub)
{
    xcd_tile_block_units((int)blockIdx.x, b.NT, TILE / FFT_SPB, g, frame, tile, sub);
}
__global__ void __launch_bounds__(64 * FFT_SPB, NNN_FFT_MINWAVES) k_fft_xp(Buffers b, const StepParams *sp, int g)
{
    // (the part of the tables this kernel copies and reads: with the staging below kept to what it holds, 27.6 KB -- a fifth of the CU's LDS)
    __shared__ __attribute__((aligned(16))) char tbuf[FFT_TABLES_SHORT];
    FftLds &t = *(FftLds *)tbuf;
    __shared__ float2 Z[FFT_SPB][NFFT_BUF];
    __shared__ float part[FFT_SPB][3 * FH_STRIDE];   // the feature head's staging: correlation, log energies, band energies
    int frame, tile, sub;
    fft_block(b, g, frame, tile, sub);
    if (tile * TILE + sub * FFT_SPB >= b.S) return;   // (a block whose streams are all padding -- the last tile of a batch that is not a multiple of 64 -- has nothing to do)
    if (!live_any(b, tile, sub * FFT_SPB, FFT_SPB)) return;   // (... or all held, nnn_batch_hold_streams)
    b = frame_view(b, frame);
    const int wave = threadIdx.x >> 6;
    transform_inputs<true>(b, sp + frame, tile, sub, t, Z[wave], part[wave]);
}
// k_fft_xp without the spectra's stores, for the calls that stop at the VAD (nnn_batch_vad_*): band energies, the
// normalised correlation, the feature head (cn, silence) as k_fft_xp leaves them, bit for bit; X and P never reach memory.  Same blocks,
// same LDS, same five waves per SIMD.  With the taps on the VAD calls launch k_fft_xp instead, so that the X and P taps exist.
__global__ void __launch_bounds__(64 * FFT_SPB, NNN_FFT_MINWAVES) k_fft_feat(Buffers b, const StepParams *sp, int g)
{
    __shared__ __attribute__((aligned(16))) char tbuf[FFT_TABLES_SHORT];
    FftLds &t = *(FftLds *)tbuf;
    __shared__ float2 Z[FFT_SPB][NFFT_BUF];
    __shared__ float part[FFT_SPB][3 * FH_STRIDE];
    int frame, tile, sub;
    fft_block(b, g, frame, tile, sub);
    if (tile * TILE + sub * FFT_SPB >= b.S) return;
    if (!live_any(b, tile, sub * FFT_SPB, FFT_SPB)) return;
    b = frame_view(b, frame);
    const int wave = threadIdx.x >> 6;
    transform_inputs<true, false, false, false>(b, sp + frame, tile, sub, t, Z[wave], part[wave]);
}

// Rider blocks of a one-frame k_pitch launch (blocks `riders` ..): the frame's lag-0 transform X and its band energies, eight streams
// per block (wave = stream) -- the part of the back end that needs nothing from the pitch analysis, done while the pitch blocks, one per
// compute unit and bound by their own latency chains, leave most issue slots free.  The fused back end then fetches X instead of
// computing it (k_back<.., XR>).  The code is k_fft_x's; `lds` is the pitch kernel's own LDS block, which a rider block has to itself.
struct XtLds { FftLds t; float2 Z[8][NFFT_BUF]; float part[8][4]; };
template <bool HELD> __device__ __forceinline__ void xt_rider(const Buffers &b, const StepParams *sp, int rb, void *lds)
{
    static_assert(sizeof(XtLds) <= sizeof(PkLds) && PK_T == 512 && FFT_SPB == 4, "");
    XtLds &x = *(XtLds *)lds;
    const int wave = threadIdx.x >> 6;
    if ((rb >> 3) * TILE + 8 * (rb & 7) >= b.S) return;
    if (HELD && !live_any(b, rb >> 3, 16 * ((rb & 7) >> 1), 16)) return;   // (by the sixteen streams of the k_back block that fetches this X: both run or neither)
    transform_inputs<false>(b, sp, rb >> 3, 2 * (rb & 7), x.t, x.Z[wave], x.part[wave]);   // rows 8 (rb % 8) + wave of tile rb / 8
}

// lag-0 transform and band energies only (training rows: clean and noise states)
__global__ void __launch_bounds__(64 * FFT_SPB) k_fft_x(Buffers b, const StepParams *sp, int g)
{
    __shared__ FftLds t;
    __shared__ float2 Z[FFT_SPB][NFFT_BUF];
    __shared__ float part[FFT_SPB][4];   // (the feature head's staging: unused without the second transform)
    int frame, tile, sub;
    fft_block(b, g, frame, tile, sub);
    if (tile * TILE + sub * FFT_SPB >= b.S) return;
    b = frame_view(b, frame);
    const int wave = threadIdx.x >> 6;
    transform_inputs<false>(b, sp + frame, tile, sub, t, Z[wave], part[wave]);
}

#pragma clang fp contract(off)

}  // namespace nnn
