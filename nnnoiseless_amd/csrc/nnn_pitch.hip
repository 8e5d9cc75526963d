#pragma once
// nnn_pitch.hip -- the pitch stage: k_pitch and everything only it uses.  Not a translation unit: nnn_kernels.hip includes it between the LPC
// kernels (nnn_lpc.hip) and the transforms (nnn_fft.hip).  lpc_finish, which k_lpc shares, stays in nnn_lpc.hip; xt_rider's definition in nnn_fft.hip.
//
// ---------------------------------------------------------------------------------------------
// K3  pitch: the pitch analysis of a frame from the FIR on, one block per 16 consecutive streams (a quarter tile):
//       pitch_downsample's last step FIR5 with k_lpc's taps -> pitch_buf (ref: src/pitch.rs:407-429)
//       pitch_search                 coarse cross-correlation 147 lags x 240 taps on the 4x-decimated signal, find_best_pitch,
//                                    fine cross-correlation within +-2 of 2*best / 2*second, find_best_pitch, pseudo-
//                                    interpolation (ref: src/pitch.rs:63-115, 296-405)
//       remove_doubling              (ref: src/pitch.rs:118-221)
//     pitch_buf (864 values per stream) lives in LDS from the FIR that makes it to the last inner product that reads it and
//     never travels to HBM (round 2a: written once and read by two more launches, 17 KB per stream-frame); so do the coarse
//     cross-correlation, the coarse-lag energies and the check points of the two long energy scans (fine-lag energies,
//     yy_lookup) that are looked up at data-dependent lags later in the frame.
//
//     Every sum that feeds the integer pitch index keeps the reference's order (sequential per lag / per partial), so the
//     parallelism is over streams x independent chains, lane = (stream, chain):
//       FIR                  (stream, 32-row chunk)         elementwise
//       coarse xcorr         (stream, group of 13 lags)     12 groups on three waves, packed accumulators (see the phase)
//       energy scans         (stream) on three waves        serial running sums with their clamps
//       inner products       (stream, partial q of 4), the wave picks the candidate lags: 2 (fine) or 4 (remove_doubling)
//                            candidates share every read of the fixed operand
//       decisions            (stream) on wave 0             find_best_pitch x 2, the k = 2..15 loop of remove_doubling
//     LDS layout of pitch_buf: even rows and odd rows apart, element (r, s) at (r & 1 ? ODD : 0) + (r >> 1) * 16 + s with ODD =
//     432 * 16 + 16.  ds_read_b32 / ds_read2_b32 bank modulo 32, a 32-lane group is 16 streams x 2 chains: chains reading rows r
//     and r + 2 (the inner-product partials, dealt to the lanes as q = 0, 2 | 1, 3) sit on neighbouring rows of one half,
//     chains reading rows r and r + 1 on the same row index of the two halves, which the pad
//     of 16 puts on different banks; the coarse cross-correlation reads the even half only -- the 4x-decimated signal,
//     compact -- and its two lag groups per 32 lanes start 13 rows apart: all conflict-free (round 2a: 31 % of k_pitch2's LDS
//     cycles were conflicts).  Rows 2 apart (consecutive taps of one partial, of the decimated signal, of the window pairs)
//     are 16 or 32 floats apart at any parity: one ds_read2_b32 fetches two of them into a register pair, which is what
//     v_pk_mul_f32 wants.
//     remove_doubling carries last_period / last_gain from frame to frame: the launch loops over the `g` frames of its
//     group; the next frame's decimated window is requested a frame ahead and waits in registers.
// ---------------------------------------------------------------------------------------------
namespace nnn {

constexpr int PK_SPB = 16;                       // streams per block
constexpr int PK_WAVES = 8;
constexpr int PK_T = 64 * PK_WAVES;
#ifndef NNN_PK_LC
#define NNN_PK_LC 13
#endif
constexpr int PK_LC = NNN_PK_LC;                 // coarse lags per lane: 12 groups of 13 (the last one 4 lags wide) on three waves
constexpr int PK_NG = (NLAG1 + PK_LC - 1) / PK_LC;
static_assert((PK_LC & 1) && PK_NG <= 4 * 8, "odd group size: neighbouring groups start on different row parities");
constexpr int PK_XW = (PK_NG + 3) / 4;           // waves of the coarse cross-correlation
constexpr int PK_JB = 8;                         // taps per unrolled step of the coarse cross-correlation (240 = 30 x 8)
constexpr int PK_NP = PK_LC / 2;                 // packed accumulators per lane (+ one single: PK_LC is odd)
constexpr int PK_NT = PK_JB / 2 + PK_NP;         // window pairs per alignment
static_assert((PK_NG - 1) * PK_LC + 239 + PK_JB + PK_LC < XLP / 2, "the window stays inside the even rows");
constexpr int PK_KMAX = 12;                      // largest divisor of remove_doubling that can pass its `t1 >= min_period` test
constexpr int PK_NE = 1 + 2 * (PK_KMAX - 1);     // candidate periods of the decision loop: t0, then two per divisor k = 2 .. 12
constexpr int PK_NSLOT = PK_NE + 2;              // + the two neighbours of t0
constexpr int PK_NC = 36;                        // inner-product slots: 10 fine lags | 25 candidates of remove_doubling, 32 .. 34 the refinement

constexpr int PK_HALF = (XLP / 2) * PK_SPB;      // floats of the even rows
constexpr int PK_ODD = PK_HALF + 16;             // first odd row
__device__ __forceinline__ int pk_at(int r, int s) { return ((r & 1) ? PK_ODD : 0) + (r >> 1) * PK_SPB + s; }


// running best / second-best update of find_best_pitch, ref: src/pitch.rs:383-400
struct BestPitch {
    float best_num, second_num, best_den, second_den;
    int best, second;
    __device__ void init() { best_num = -1.0f; second_num = -1.0f; best_den = 0.0f; second_den = 0.0f; best = 0; second = 1; }
    // the reference's nested ifs as selects (the same comparisons on the same values: a NaN fails them either way); this runs
    // on one wave with the rest of the block waiting, where a taken branch costs more than the selects
    __device__ __forceinline__ void update(int i, float corr, float y_sq_norm) {
        const float num = corr * corr;
        const bool in = corr > 0.0f && num * second_den > second_num * y_sq_norm;
        const bool top = in && num * best_den > best_num * y_sq_norm;
        const bool mid = in && !top;
        second_num = top ? best_num : (mid ? num : second_num);
        second_den = top ? best_den : (mid ? y_sq_norm : second_den);
        second = top ? best : (mid ? i : second);
        best_num = top ? num : best_num;
        best_den = top ? y_sq_norm : best_den;
        best = top ? i : best;
    }
    // the same with corr * corr handed in, NaN standing for "corr > 0 failed" (every comparison with it fails): the coarse search
    // squares its 147 correlations on the lanes that made them
    __device__ __forceinline__ void update_sq(int i, float num, float y_sq_norm) {
        const bool in = num * second_den > second_num * y_sq_norm;
        if (!wave_any(in)) return;   // none of the wave's streams takes this lag: nothing changes
        const bool top = in && num * best_den > best_num * y_sq_norm;
        const bool mid = in && !top;
        second_num = top ? best_num : (mid ? num : second_num);
        second_den = top ? best_den : (mid ? y_sq_norm : second_den);
        second = top ? best : (mid ? i : second);
        best_num = top ? num : best_num;
        best_den = top ? y_sq_norm : best_den;
        best = top ? i : best;
    }
};

struct Xc2 {   // xcorr[] of the fine search: zero except within 2 of 2*best / 2*second (ref: src/pitch.rs:88-96)
    float v[10];
    int lo1, lo2;
    __device__ __forceinline__ float at(int i) const
    {
        float r = 0.0f;
        if (i >= 0 && i < NLAG2) {
            const int d1 = i - lo1, d2 = i - lo2;
#pragma unroll
            for (int u = 4; u >= 0; u--) if (d2 == u) r = v[5 + u];
#pragma unroll
            for (int u = 4; u >= 0; u--) if (d1 == u) r = v[u];   // first window wins where they overlap (same value)
        }
        return r;
    }
};

__device__ __forceinline__ float pitch_gain(float xy, float xx, float yy) { return xy / sqrtf(1.0f + xx * yy); }

// The two long energy scans run once per frame, serially, and are looked up at a few data-dependent lags later in the frame.
// They leave check points in LDS (every 8th fine lag, every 5th step of yy); a lookup replays the few steps from the check
// point below it -- the same additions in the same order.  (Whole tables would be 43 KB per block; through global scratch the
// scans were bound by the depth of a wave's store queue.)
constexpr int PK_CKF = 8, PK_NCKF = (NLAG2 + PK_CKF - 1) / PK_CKF;    // 37
constexpr int PK_CKY = 5, PK_NCKY = 384 / PK_CKY + 1;                  // 77
// The certified coarse search (round 6; see the phase in k_pitch): what it keeps in LDS.
constexpr int PK_DCK = 41;                       // a stream's row of check points of the coarse lags' energy scan (one per group of four lags; an odd pitch)
constexpr int PK_RMAX = 24;                      // lags of one stream that may survive the approximate search (more: the block takes the full search)
constexpr int PK_CAP = 384;                      // ... and of the block's 16 streams together
constexpr int PK_PLW = XLP / 2 + 8;              // halfwords between two streams' bf16 planes (the 432 even rows of pitch_buf): 220 words, so that the
                                                 // eight streams of a region sit on eight different banks for the FIR's word stores
constexpr float PK_EPS = 0.0083f;                // |approximate - reference| <= PK_EPS sqrt(|x|^2 |y window|^2): two bf16 roundings 2^-7, the matrix
                                                 // cores' f32 accumulation and the reference's own sequential f32 sum well inside the rest
struct PkCert {
    float denck[PK_SPB][PK_DCK];                 // the running energy before coarse lag 4 k (find_best_pitch, ref: src/pitch.rs:380-402): check points, as for the fine lags
    float bsum[PK_SPB][27];                      // |.|^2 of the 27 blocks of 16 even rows (any nonzero value: at least 2^-120)
    unsigned mask[PK_SPB][5];                    // bit L: coarse lag L of the stream survived
    unsigned count, full, pad_[2];               // survivors of the block; != 0: the block takes the full search
    unsigned short list[PK_CAP];                 // survivors (stream << 8 | lag) ...
    float slotv[PK_SPB][PK_RMAX], slotd[PK_SPB][PK_RMAX];   // ... their exact sums and the energy each of them saw, by rank within the stream
    int slotl[PK_SPB][PK_RMAX];                  // ... and their lags
    alignas(16) unsigned short plane[(PK_SPB / 2) * PK_PLW + 16];   // bf16 even rows of streams 8 .. 15 (streams 0 .. 7: over ckf / cky, idle until the scans);
                                                                    // + the 32 bytes the last fragment read of the last stream runs over (masked).  Nothing
                                                                    // shares the planes' bytes: the search reads them while its first waves list survivors
};
struct alignas(16) PkLds {
    float pb[PK_ODD + PK_HALF];                  // the decimated window, then (in place) pitch_buf
    float ckf[PK_NCKF][PK_SPB];                  // running energy of the fine lags before lag 8 m (find_best_pitch, ref: src/pitch.rs:380-402)
    float cky[PK_NCKY][PK_SPB];                  // running energy yy of remove_doubling after step 5 m (ref: src/pitch.rs:133-142); [0] = xx
    union {
        struct { float xc[NLAG1][PK_SPB], ysq[NLAG1][PK_SPB]; } c;   // full coarse search: squared positive cross-correlation (else NaN), running energy per lag
        PkCert a;                                                      // certified coarse search
        struct {                                                       // from the fine search on
            float part[PK_NC][4][PK_SPB];        // inner-product partials [slot][q][stream] (ref: src/pitch.rs:225-244)
            float yy[32][PK_SPB];                // yy_lookup at the candidate periods
            float ye[10][PK_SPB];                // the running energy the fine lags of the two windows saw
            int cand[32][PK_SPB];                // candidate periods of remove_doubling
            int lo[2][PK_SPB];                   // first fine lag of the two windows
            int tsel[PK_SPB];                    // the period the decision loop chose
            float xx[PK_SPB], lgain[PK_SPB];     // per stream: |x|^2, the previous frame's gain ...
            int t0[PK_SPB], pprev[PK_SPB];       // ... the period before remove_doubling, the previous frame's period / 2
            float kxy[16][PK_SPB], kyy[16][PK_SPB], kg[16][PK_SPB];   // per candidate divisor k: its xy, yy, gain ...
            int kpass[16][PK_SPB];               // ... and whether it replaces the best so far
            int any_refine;                      // some stream of the block left t0: the +-1 refinement needs inner products
        } f;
    } u;
};
static_assert(sizeof(PkLds) <= 80 * 1024, "two blocks per CU");
static_assert(offsetof(PkLds, ckf) % 16 == 0 && offsetof(PkLds, u) % 16 == 0 && offsetof(PkCert, plane) % 16 == 0 && (PK_PLW * 2) % 16 == 0, "16-byte fragment reads");
static_assert(sizeof(float) * (PK_NCKF + PK_NCKY) * PK_SPB >= sizeof(unsigned short) * (PK_SPB / 2) * PK_PLW + 32, "the first eight planes fit over the check points");

// Window and FIR mapping: thread = (stream col, chunk ch of 32 rows), 27 chunks (the block's last 80 threads idle here); a
// chunk starts on an even row, so every LDS address of its 16 row pairs is the thread's base plus a constant.
constexpr int PK_CH = 32, PK_NCH = XLP / PK_CH;
static_assert(PK_NCH * PK_CH == XLP && PK_NCH * PK_SPB <= PK_T, "");

// a frame's window from the decimated-history ring: 16 lanes share a 64-byte segment of a tile row; with it the frame's five FIR
// taps (k_lpc's output, kept by ring slot)
__device__ __forceinline__ void pk_window_load(const Buffers &b, const StepParams *sp, int tile, int q0, int tid, float (&v)[PK_CH],
                                               float (&fir)[5])
{
    const int col = tid & 15, ch = tid >> 4;
    if (ch >= PK_NCH) {   // (defined on every path: otherwise the previous window stays live through the whole frame for the register allocator)
#pragma unroll
        for (int i = 0; i < PK_CH; i++) v[i] = 0.0f;
#pragma unroll
        for (int i = 0; i < 5; i++) fir[i] = 0.0f;
        return;
    }
    const int slot = sp->slot;
    {
        const float *lp = NNN_TI(b.lpc, b.nslot * 10, tile, q0 + col) + (size_t)(slot * 10) * TILE;
#pragma unroll
        for (int i = 0; i < 5; i++) fir[i] = lp[(size_t)(5 + i) * TILE];
    }
    const float *base = b.dec + ((size_t)tile * dec_len(b.nslot) + (size_t)dec_base(slot, b.nslot)) * TILE + q0;   // uniform
    const unsigned off = (unsigned)(ch * PK_CH) * TILE + (unsigned)col;
#pragma unroll
    for (int i = 0; i < PK_CH; i++) v[i] = base[off + (unsigned)i * TILE];
    if (ch == 0) v[0] = NNN_TI(b.xlp0, b.nslot, tile, q0 + col)[(size_t)slot * TILE];   // x_lp[0] is special (ref: src/pitch.rs:458)
}

// 4-way interleaved inner-product partials (ref: src/pitch.rs:225-244) of NCAND candidates against the fixed operand
// p[384 ..]: lane (s, q) accumulates x[4m+q] * y_c[4m+q] over m in order, one read of x serving every candidate;
// the caller combines ((s0+s1)+s2)+s3.  y_c starts at row yr[c].  Rows 4m + const of one stream are 32 floats apart: one
// ds_read2_b32 brings taps m, m + 1 as a register pair, one v_pk_mul_f32 forms both products, two adds in order.
template <int NCAND>
__device__ __forceinline__ void pk_inner(const float *pb, int s, int q, const int (&yr)[NCAND], float (&acc)[NCAND])
{
    constexpr int U = NCAND >= 4 ? 2 : 3;   // tap pairs per register set
    static_assert(120 % (4 * U) == 0, "");
    const float *xp = pb + pk_at(PITCH_MAX / 2 + q, s);
    const float *yp[NCAND];
#pragma unroll
    for (int c = 0; c < NCAND; c++) { acc[c] = 0.0f; yp[c] = pb + pk_at(yr[c] + q, s); }
    // two register sets in turn: the rows of the next taps travel while these are summed (round 6: with one set the compiler's loop was
    // "load, wait, use" -- every trip paid the LDS latency in full)
    v2f xa[U], ya[NCAND][U], xb[U], yb[NCAND][U];
#define NNN_LD(X, Y, M) do { _Pragma("unroll") for (int u_ = 0; u_ < U; u_++) { const int o_ = 32 * ((M) + 2 * u_); X[u_] = mk2(xp[o_], xp[o_ + 32]); \
        _Pragma("unroll") for (int c_ = 0; c_ < NCAND; c_++) Y[c_][u_] = mk2(yp[c_][o_], yp[c_][o_ + 32]); } } while (0)
#define NNN_ACC(X, Y) do { _Pragma("unroll") for (int u_ = 0; u_ < U; u_++) _Pragma("unroll") for (int c_ = 0; c_ < NCAND; c_++) { \
        const v2f pr_ = pk_mul(X[u_], Y[c_][u_]); acc[c_] = sadd(acc[c_], pr_.x); acc[c_] = sadd(acc[c_], pr_.y); } } while (0)
    NNN_LD(xa, ya, 0);
#pragma nounroll
    for (int m0 = 0; m0 < 120 - 4 * U; m0 += 4 * U) {
        NNN_LD(xb, yb, m0 + 2 * U);
        NNN_ACC(xa, ya);
        NNN_LD(xa, ya, m0 + 4 * U);
        NNN_ACC(xb, yb);
    }
    NNN_LD(xb, yb, 120 - 2 * U);
    NNN_ACC(xa, ya);
    NNN_ACC(xb, yb);
#undef NNN_LD
#undef NNN_ACC
}

// Lag K of the autocorrelation of a stream's 864-value window in LDS (`pbs` = L.pb + stream: row r at pk_at(r, 0)): the reference's
// sequential sum over i = 0 .. 859 and its tail (ref: src/pitch.rs:433-446), one lag per wave so that the lag is a compile-time
// offset into a sliding run of rows held in registers: a row is read once per lag, a step is one multiply and one dependent add.
// `blk0`, `c0`: the sum's first 16 blk0 steps were taken elsewhere (k_hp2's head waves: they need none of the new frame) and gave c0.
template <int K>
__device__ __forceinline__ float pk_autocorr(const float *pbs, int blk0 = 0, float c0 = 0.0f)
{
    const float *E = pbs + 8 * blk0 * PK_SPB, *O = E + PK_ODD;
    auto row = [&](const float *e, const float *o, int j) { return (j & 1) ? o[(j >> 1) * PK_SPB] : e[(j >> 1) * PK_SPB]; };
    float run[20];   // run[j] = x[16 blk + j]
#pragma unroll
    for (int j = 0; j < 20; j++) run[j] = row(E, O, j);
    E = pbs; O = pbs + PK_ODD;
    float c = c0;
    constexpr int NBLK = 52;   // 52 blocks of 16 steps, then 28 steps on rows 832 .. 863
#pragma nounroll   // (two blocks per trip -- the run's hand-over a renaming instead of twenty moves -- measured: no change)
    for (int blk = blk0; blk < NBLK; blk++) {
        float nxt[16];   // rows 16 (blk + 1) + 4 .. + 19 travel while this block's steps are summed
        const float *En = E + (8 * (blk + 1) + 2) * PK_SPB, *On = O + (8 * (blk + 1) + 2) * PK_SPB;
#pragma unroll
        for (int j = 0; j < 16; j++) nxt[j] = row(En, On, j);
#pragma unroll
        for (int j = 0; j < 16; j++) c += run[j] * run[j + K];
#pragma unroll
        for (int j = 0; j < 4; j++) run[j] = run[16 + j];
#pragma unroll
        for (int j = 0; j < 16; j++) run[4 + j] = nxt[j];
    }
    float last[12];   // rows 852 .. 863
#pragma unroll
    for (int j = 0; j < 12; j++) last[j] = row(E + (8 * NBLK + 10) * PK_SPB, O + (8 * NBLK + 10) * PK_SPB, j);
    auto x = [&](int i) { return i < 16 * NBLK + 20 ? run[i - 16 * NBLK] : last[i - 16 * NBLK - 20]; };   // rows 832 .. 863 (static index)
#pragma unroll
    for (int i = 16 * NBLK; i < XLP - 4; i++) c += x(i) * x(i + K);
    float d = 0.0f;   // tail d_K = sum_{i = K + 860}^{863} x[i] x[i - K], added after the main sum
#pragma unroll
    for (int i = K + XLP - 4; i < XLP; i++) d += x(i) * x(i - K);
    return c + d;
}

// ---- the serial energy scans of k_pitch on quad lanes (round 6) -------------------------------------------------------------------
// find_best_pitch and remove_doubling carry three running energies through the frame -- the energy every coarse lag sees, the one every
// fine lag sees, yy_lookup (ref: src/pitch.rs:380-402, :133-142) -- each a chain of several hundred f32 additions whose order is the
// reference's.  One wave issues one instruction every ~4.5 cycles whatever its lane count, and with lane = stream a step was six or seven
// instructions (two loads, two squares, a difference, the add, the clamp) on 16 of 64 lanes: the chains, not the arithmetic of the search,
// were the frame's critical path (round 6 stamps: 10 + 8 us of a block's 42).  Here a wave takes ONE chain for the block's 16 streams,
// lane = (stream, q): the four lanes of a quad fetch and square the rows of four consecutive steps at once, and every lane then adds the
// four terms in order, each add taking its operand from a quad lane through DPP -- the same additions in the same order, 2.25 to 4.25
// instructions per step.  Rows are requested a group ahead of the adds that use them.
constexpr int PK_FINE_K = (NLAG2 + 3) / 4;       // 74 groups of four fine lags
constexpr int PK_YY_B = 19;                      // 19 runs of twenty steps of yy_lookup (380 steps: the last four are only ever replayed)
// (the four terms are fetched by four independent DPP moves, then added by plain instructions: an add that takes its operand through DPP
// waits two more states on the sum it has just written and runs at a third of the rate -- measured, 21 against 9 cycles a step)
__device__ __forceinline__ Quad4 pk_quad4(float t)
{
    Quad4 r = quad_all(t);   // (nnn_mfma.h: four DPP moves; the tests' interpreter: one rendezvous of the wave's lanes)
    keep_rw(r.t0); keep_rw(r.t1); keep_rw(r.t2); keep_rw(r.t3);
    return r;
}
__device__ __forceinline__ float pk_add4(float y, float t)
{
    const Quad4 r = pk_quad4(t);
    y = y + r.t0;
    y = y + r.t1;
    y = y + r.t2;
    return y + r.t3;
}
// the energy every coarse lag sees (even rows only), ref: src/pitch.rs:83 -> :380-402: its start, 1 + |y4[0 .. 239]|^2 ...
__device__ __forceinline__ float pk_chain_coarse_start(const float *pbs, int cq)
{
    const float *pq = pbs + cq * PK_SPB;   // y4[4 k + cq] at pq[64 k]
    float ysq = 1.0f;
    float nx[4];
#pragma unroll
    for (int i = 0; i < 4; i++) nx[i] = pq[(4 * i) * PK_SPB];
#pragma nounroll
    for (int k0 = 0; k0 < 60; k0 += 4) {
        float cur[4];
#pragma unroll
        for (int i = 0; i < 4; i++) cur[i] = nx[i];
        const int kn = k0 + 4 < 60 ? k0 + 4 : k0;
#pragma unroll
        for (int i = 0; i < 4; i++) nx[i] = pq[(4 * (kn + i)) * PK_SPB];
#pragma unroll
        for (int i = 0; i < 4; i++) ysq = pk_add4(ysq, cur[i] * cur[i]);
    }
    return ysq;
}
// ... and groups k0 .. k1 - 1 of four lags (lag L drops y4[L] and takes y4[L + 240]); check point dn[k] = the energy before lag 4 k
constexpr int PK_COARSE_K = 38;                  // (147 lags: the 148th .. 152nd are computed and dropped)
__device__ __forceinline__ float pk_chain_coarse(const float *pbs, int cq, float ysq, int k0, int k1, float *dn)
{
    float na[2], nd[2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int L = 4 * (k0 + i) + cq < NLAG1 ? 4 * (k0 + i) + cq : NLAG1 - 1;
        na[i] = pbs[(L + 240) * PK_SPB];
        nd[i] = pbs[L * PK_SPB];
    }
#pragma nounroll
    for (int k = k0; k < k1; k += 2) {
        float ca[2], cd[2];
#pragma unroll
        for (int i = 0; i < 2; i++) { ca[i] = na[i]; cd[i] = nd[i]; }
        const int kn = k + 2 < k1 ? k + 2 : k;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int L = 4 * (kn + i) + cq < NLAG1 ? 4 * (kn + i) + cq : NLAG1 - 1;
            na[i] = pbs[(L + 240) * PK_SPB];
            nd[i] = pbs[L * PK_SPB];
        }
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const float t = ca[i] * ca[i] - cd[i] * cd[i];
            const Quad4 r = pk_quad4(t);
            if (cq == 0) dn[k + i] = ysq;
            ysq = fmaxf(ysq + r.t0, 1.0f);
            ysq = fmaxf(ysq + r.t1, 1.0f);
            ysq = fmaxf(ysq + r.t2, 1.0f);
            ysq = fmaxf(ysq + r.t3, 1.0f);
        }
    }
    return ysq;
}
// the energy every fine lag sees (ref: src/pitch.rs:97 -> :380-402): its start, 1 + |rows 0 .. 479|^2 in row order ...
__device__ __forceinline__ float pk_chain_fine_start(const float *pbs, int cq, float ysq, int k0, int k1)   // rows 4 k0 .. 4 k1 - 1 (k0, k1 multiples of 4)
{
    const float *pq = pbs + ((cq & 1) ? PK_ODD : 0) + (cq >> 1) * PK_SPB;   // row 4 k + cq at pq[32 k]
    float nx[4];
#pragma unroll
    for (int i = 0; i < 4; i++) nx[i] = pq[(2 * (k0 + i)) * PK_SPB];
#pragma nounroll
    for (int k = k0; k < k1; k += 4) {
        float cur[4];
#pragma unroll
        for (int i = 0; i < 4; i++) cur[i] = nx[i];
        const int kn = k + 4 < k1 ? k + 4 : k;
#pragma unroll
        for (int i = 0; i < 4; i++) nx[i] = pq[(2 * (kn + i)) * PK_SPB];
#pragma unroll
        for (int i = 0; i < 4; i++) ysq = pk_add4(ysq, cur[i] * cur[i]);
    }
    return ysq;
}
// ... and groups k0 .. k1 - 1 of four lags: lag 4 k + cq drops row 4 k + cq and takes row 4 k + cq + 480; check point ckf[m] = the energy
// before lag 8 m (k even)
__device__ __forceinline__ float pk_chain_fine(const float *pbs, int cq, int cs, float ysq, int k0, int k1, float (*ckf)[PK_SPB])
{
    const float *pq = pbs + ((cq & 1) ? PK_ODD : 0) + (cq >> 1) * PK_SPB;
    float na[2], nd[2];
#pragma unroll
    for (int i = 0; i < 2; i++) { na[i] = pq[(2 * (k0 + i) + 240) * PK_SPB]; nd[i] = pq[(2 * (k0 + i)) * PK_SPB]; }
#pragma nounroll
    for (int k = k0; k < k1; k += 2) {
        float ca[2], cd[2];
#pragma unroll
        for (int i = 0; i < 2; i++) { ca[i] = na[i]; cd[i] = nd[i]; }
        const int kn = k + 2 < k1 ? k + 2 : k;
#pragma unroll
        for (int i = 0; i < 2; i++) { na[i] = pq[(2 * (kn + i) + 240) * PK_SPB]; nd[i] = pq[(2 * (kn + i)) * PK_SPB]; }
        if (cq == 0) ckf[k >> 1][cs] = ysq;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const float t = ca[i] * ca[i] - cd[i] * cd[i];
            const Quad4 r = pk_quad4(t);
            ysq = fmaxf(ysq + r.t0, 1.0f);
            ysq = fmaxf(ysq + r.t1, 1.0f);
            ysq = fmaxf(ysq + r.t2, 1.0f);
            ysq = fmaxf(ysq + r.t3, 1.0f);
        }
    }
    return ysq;
}
// xx = yy_lookup[0] = |rows 384 .. 863|^2 as inner_prod sums it: four interleaved partial sums combined ((s0 + s1) + s2) + s3
// (ref: src/pitch.rs:133-136, :225-244) -- one partial per quad lane
__device__ __forceinline__ float pk_chain_yy_start(const float *pbs, int cq)
{
    const float *pq = pbs + ((cq & 1) ? PK_ODD : 0) + (192 + (cq >> 1)) * PK_SPB;   // row 384 + 4 t + cq at pq[32 t]
    float sq = 0.0f;
    float nx[8];
#pragma unroll
    for (int i = 0; i < 8; i++) nx[i] = pq[(2 * i) * PK_SPB];
#pragma nounroll
    for (int t0 = 0; t0 < 120; t0 += 8) {
        float cur[8];
#pragma unroll
        for (int i = 0; i < 8; i++) cur[i] = nx[i];
        const int tn = t0 + 8 < 120 ? t0 + 8 : t0;
#pragma unroll
        for (int i = 0; i < 8; i++) nx[i] = pq[(2 * (tn + i)) * PK_SPB];
#pragma unroll
        for (int i = 0; i < 8; i++) sq += cur[i] * cur[i];
    }
    return ((quad_lane<0>(sq) + quad_lane<1>(sq)) + quad_lane<2>(sq)) + quad_lane<3>(sq);
}
// runs b0 .. b1 - 1 of twenty steps of yy_lookup (ref: src/pitch.rs:137-142): step j takes row 384 - j and drops row 864 - j; check point
// cky[m] = yy after step 5 m.  Lane cq of a quad prepares steps 4 k + 1 + cq.
__device__ __forceinline__ float pk_chain_yy(const float *pbs, int cq, int cs, float yy, int b0, int b1, float (*cky)[PK_SPB])
{
    const float *pq = pbs + ((cq & 1) ? 0 : PK_ODD) + (191 - (cq >> 1)) * PK_SPB;   // row 383 - 4 k - cq at pq[-32 k]
    float na[5], nc[5];
#pragma unroll
    for (int i = 0; i < 5; i++) { na[i] = pq[-(2 * (5 * b0 + i)) * PK_SPB]; nc[i] = pq[(240 - 2 * (5 * b0 + i)) * PK_SPB]; }
#pragma nounroll
    for (int bk = b0; bk < b1; bk++) {
        float ca[5], cc[5];
#pragma unroll
        for (int i = 0; i < 5; i++) { ca[i] = na[i]; cc[i] = nc[i]; }
        const int bn = bk + 1 < b1 ? bk + 1 : bk;
#pragma unroll
        for (int i = 0; i < 5; i++) { na[i] = pq[-(2 * (5 * bn + i)) * PK_SPB]; nc[i] = pq[(240 - 2 * (5 * bn + i)) * PK_SPB]; }
#pragma unroll
        for (int i = 0; i < 5; i++) {   // steps 20 bk + 4 i + 1 .. + 4: the run's check points fall behind step 5, 10, 15, 20
            const float t = ca[i] * ca[i] - cc[i] * cc[i];
            const Quad4 r = pk_quad4(t);
            yy = yy + r.t0;
            if (i == 1 && cq == 0) cky[4 * bk + 1][cs] = yy;
            yy = yy + r.t1;
            if (i == 2 && cq == 0) cky[4 * bk + 2][cs] = yy;
            yy = yy + r.t2;
            if (i == 3 && cq == 0) cky[4 * bk + 3][cs] = yy;
            yy = yy + r.t3;
            if (i == 4 && cq == 0) cky[4 * bk + 4][cs] = yy;
        }
    }
    return yy;
}

// sum_{j < 240} x[j] y[j] in order (ref: src/pitch.rs:296-363, one lag), rows PK_SPB floats apart: two register sets in turn, so that the
// rows of the next eight taps travel while these eight are summed (the compiler rotates a one-set prefetch back into "load, wait, use")
__device__ __forceinline__ float pk_dot240(const float *xp, const float *yp)
{
    float c = 0.0f;
    v2f xa[4], ya[4], xb[4], yb[4];
#define NNN_LD(X, Y, J) do { _Pragma("unroll") for (int i_ = 0; i_ < 4; i_++) { \
        X[i_] = mk2(xp[((J) + 2 * i_) * PK_SPB], xp[((J) + 2 * i_ + 1) * PK_SPB]); Y[i_] = mk2(yp[((J) + 2 * i_) * PK_SPB], yp[((J) + 2 * i_ + 1) * PK_SPB]); } } while (0)
#define NNN_ACC(X, Y) do { _Pragma("unroll") for (int i_ = 0; i_ < 4; i_++) { const v2f pr_ = pk_mul(X[i_], Y[i_]); c = sadd(c, pr_.x); c = sadd(c, pr_.y); } } while (0)
    NNN_LD(xa, ya, 0);
#pragma nounroll
    for (int j = 0; j < 224; j += 16) {
        NNN_LD(xb, yb, j + 8);
        NNN_ACC(xa, ya);
        NNN_LD(xa, ya, j + 16);
        NNN_ACC(xb, yb);
    }
    NNN_LD(xb, yb, 232);
    NNN_ACC(xa, ya);
    NNN_ACC(xb, yb);
#undef NNN_LD
#undef NNN_ACC
    return c;
}

constexpr int PK_SEG_FS = 120;
#ifndef NNN_PK_SEG_F1
#define NNN_PK_SEG_F1 44
#endif
constexpr int PK_SEG_F1 = NNN_PK_SEG_F1;   // groups of fine lags wave 5 has scanned when the survivors' exact sums are done; the rest beside find_best
static_assert(PK_SEG_F1 % 2 == 0 && PK_SEG_F1 <= PK_FINE_K, "");


// (defined behind the transforms, further down: the X transform of a one-frame call in rider blocks of k_pitch's launch)
template <bool HELD> __device__ __forceinline__ void xt_rider(const Buffers &b, const StepParams *sp, int rb, void *lds);

#ifndef NNN_PK_MINWAVES
#define NNN_PK_MINWAVES 4   // waves per SIMD: two blocks of 8 waves per CU, <= 128 registers
#endif
// `chain` != 0: one workgroup per (frame, quarter tile), work item = frame * blocks_per_frame + quarter tile.  Everything but the
// decision loop of remove_doubling is independent from frame to frame, so the frames of a group run side by side and a workgroup
// waits -- just before that loop -- for the flag its predecessor (same streams, previous frame: a lower work item) sets once its
// pitch and gain are in memory.  A workgroup takes its work item from a device-wide ticket counter when it STARTS (`tbase` = the
// counter's value before this launch), not from its block index: the holder of item i then knows that every item below i has been
// taken by a workgroup that is already running, so the wait always ends -- whatever order the hardware dispatches workgroups in
// (HIP promises none; in the observed in-order dispatch ticket and block index coincide).  `seq0` numbers the group's first frame;
// flag values are frame numbers, so a flag left by an earlier use of the scratch set never matches.  `chain` == 0: one workgroup
// per quarter tile loops over the frames.
// `lpc_here` != 0 (one-frame launches of a few thousand streams, the real-time tick): the LPC analysis runs here, on five of the block's
// waves ahead of the FIR, instead of as a launch of its own (k_lpc_wide) ahead of this one -- round 2's arrangement, which costs the
// block 9 us with six waves waiting; for a group of frames that was the kernel's worst phase, for a lone frame it is cheaper than the
// 14.5 us launch plus its gap on the call's critical path.  Same sums in the same order: bit-identical to k_lpc / k_lpc_wide.
// LPC: the instantiation that can run the LPC analysis (`lpc_here`): its autocorrelation holds 36 registers beside the prefetched window, which
// costs the frame loop of the groups' instantiation spills at the kernel's 128-register limit (round 6).
//
// The phases of a frame, who runs them, and what of PkLds they touch.  PkLds::u has three meanings in turn -- u.c (full coarse search; before it
// the scratch of the LPC analysis), u.a (certified coarse search), u.f (from the fine search on) -- and the bytes of ckf / cky first hold the bf16
// planes of streams 0 .. 7.  "dec" = the decision lanes (wave 0, lane = stream); R / W = reads / writes; every phase but the last ends at a block
// barrier, named by the stamp behind it.
//
//   phase                              runs on                            LDS                                                        ends
//   ---------------------------------  ---------------------------------  ---------------------------------------------------------  ---------------
//   (prologue, before the frame loop: ticket or block index -> frame, tile, quarter through u.f.any_refine and two barriers of its own; blocks of
//    padding or of held streams return; dec take last_period / last_gain, waves 0 .. 4 head_c0, every thread the first window: registers)
//   window -> LDS                      threads (stream, chunk), 432 of 512  W pb (the decimated window)                               barrier, stamp 1
//   LPC analysis (lpc_here only)
//     autocorrelation                  waves 0 .. 4, lanes 0 .. 15        R pb; W u.c.xc[0 .. 4] (`acs`)                             barrier
//     lpc_finish                       dec                                R acs; W u.c.xc[8 .. 12] (`firs`)                          barrier
//     taps                             every thread                       R firs -> fir[] (registers)                                (the next one)
//   FIR5 inputs                        every thread                       R pb (the five rows before the chunk) -> v[] (registers)   barrier
//   FIR5 in place, planes, energies    threads (stream, chunk)            W pb (pitch_buf from here on); R pb (own chunk);           barrier, stamp 4
//                                                                         W planes 0 .. 7 over ckf / cky, planes 8 .. 15 u.a.plane;
//                                                                         W u.a.bsum; threads 0 .. 81 clear u.a.mask / count / full
//   certified search (1) + (2)         waves 0 .. 4: streams w, w + 5,    R the planes (ckf / cky as planes 0 .. 7, u.a.plane),      barrier, stamp 5
//                                      w + 10; wave 6: stream 15, behind  u.a.bsum; W u.a.count / list / mask / full (LDS atomics)
//                                      its scan
//     beside it: coarse lags' scan     wave 7, lane = (stream, quad)      R pb; W u.a.denck
//                fine lags' scan, start  wave 5                           R pb; W nothing (the sum stays in chain_y)
//                yy_lookup, start      wave 6, ahead of its search        R pb; W nothing (chain_y) -- no check point is written while
//                                                                         ckf / cky hold planes
//   flag and count                     every thread                       R u.a.full, u.a.count -> full, nsurv (registers)           (full: barrier)
//   full search (`full` only)          lanes (stream, group) of waves     R pb; W u.c.xc                                             barrier, stamp 63
//                                      0 .. PK_XW - 1
//     beside it: coarse lags' energy   wave PK_XW, lanes 0 .. 15          R pb; W u.c.ysq  (u.c lies over u.a: denck, bsum, the
//                                                                         masks and the list are gone -- the full form needs none)
//   survivors' exact sums (3)          waves 0 .. 4 (not `full`),         R u.a.list / mask / denck, pb; W u.a.slotv / slotl / slotd  certified: barrier,
//                                      lane = survivor                                                                               stamp 27; full: none
//     beside it: fine lags' scan,      wave 5                             R pb; W ckf[0 .. PK_SEG_F1 / 2) (check points from here on:
//                first PK_SEG_F1 groups                                   the planes are dead)
//                yy_lookup, all of it  wave 6                             R pb; W cky (cky[0] = xx)
//                (wave 7 has nothing to do)
//   find_best_pitch, coarse lags       full: dec; certified: wave 0       full: R u.c.xc / ysq; certified: R u.a.mask / slot*        barrier, stamp 6
//                                                                         -> lo1, lo2 (registers of dec); then, behind wave 0's own
//                                                                         wave_lds_sync, dec W u.f.lo, u.f.any_refine = 0 (no other
//                                                                         wave reads u.c / u.a in this phase)
//     beside it: fine lags' scan, rest wave 5                             R pb; W ckf
//   fine cross-correlation             waves 0 .. 4, lane = (stream, q)   R u.f.lo, pb; W u.f.part[0 .. 9]                          barrier, stamp 7
//     beside it: the fine lags' energies  wave 5, q < 2                   R u.f.lo, ckf, pb; W u.f.ye
//   find_best_pitch, fine lags;        dec                                R cky[0], u.f.part[0 .. 9], u.f.ye; W u.f.cand[0 .. 24],   barrier, stamp 53
//   candidate table                                                       u.f.xx, u.f.t0 -> t0, xx (registers of dec)
//   yy_lookup at the candidates        lanes (stream, e) of waves 0 .. 5  R u.f.cand, cky, pb; W u.f.yy[0 .. 22]                     barrier, stamp 54
//   candidates' inner products         every wave                         R u.f.cand, pb; W u.f.part[0 .. 24]
//   next frame's window                every thread                       none (global -> win[], fir[])
//   predecessor's flag (chained), last pitch  dec                         W u.f.pprev, u.f.lgain
//   decision loop, per divisor         lanes (stream, k) of waves 0 .. 2  R u.f.part / cand / yy / t0 / xx / lgain / pprev;          barrier, stamp 58
//                                                                         W u.f.kpass / kxy / kyy / kg
//   decision loop, the choice          dec                                R u.f.kpass / kxy / kyy / kg / part[0] / yy[0] / cand;     barrier, stamp 55
//                                                                         W u.f.tsel, u.f.any_refine -> t, pg, gg (registers of dec)
//   +-1 refinement (any_refine only)   waves 0 .. 2                       R u.f.any_refine (every thread), u.f.tsel, pb;             barrier (if taken),
//                                                                         W u.f.part[32 .. 34]                                       stamp 56
//   final gain, period store, flag     dec                                R u.f.part; global: pitch, pgain, then the flag            none (stamp 57)
//
// So: while the search reads the planes, ckf / cky ARE planes 0 .. 7 and the scans' waves only sum (their check points start behind the barrier
// of stamp 5).  The scans run beside the certified search (their starts, and the whole coarse-lag scan), the survivors' exact sums, and -- wave
// 5's tail -- find_best_pitch over the coarse lags; nothing else.  In the full form no barrier stands between stamp 63 and stamp 6: there wave 5's
// first PK_SEG_F1 groups and the whole of wave 6's yy scan, too, run beside the decision lanes' find_best_pitch over all 147 lags (which reads u.c
// only; the scans write ckf / cky only).  Into the decision loop (the barrier of stamp 54) go, in registers of the
// decision lanes, t0, xx and last_period / last_gain (and on every thread the prefetched win / fir); in LDS u.f.cand, part[0 .. 24], yy, xx, t0,
// pprev, lgain and any_refine = 0; pb is still read by the refinement; ckf / cky are dead.
template <bool LPC, bool HELD = false>
__global__ void __launch_bounds__(PK_T, NNN_PK_MINWAVES) k_pitch(Buffers b, const StepParams *sp0, int g, int chain, int seq0, unsigned tbase, int lpc_here_,
                                                                 int riders)
{
    __shared__ PkLds L;
    const int lpc_here = LPC ? lpc_here_ : 0;
    if (riders > 0 && (int)blockIdx.x >= riders) {   // (one-frame launches only: chain == 0, the pitch blocks are blocks 0 .. riders - 1)
        xt_rider<HELD>(b, sp0, (int)blockIdx.x - riders, &L);
        return;
    }
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane0 = threadIdx.x & 63;
    int lane = lane0, s = lane & 15, q = lane >> 4;  // lane = (stream, chain)
    int item = (int)blockIdx.x;
    if (chain) {
        if (threadIdx.x == 0) L.u.f.any_refine = (int)(ticket_take(b.ticket) - tbase);
        __syncthreads();
        item = __builtin_amdgcn_readfirstlane(L.u.f.any_refine);
        __syncthreads();   // (the field is written again further down)
    }
    // Workgroup b runs on XCD b mod 8 (observed dispatch order; a speed matter only).  The four quarter-tile blocks of tile t are
    // sent to XCD t mod 8 -- the one whose L2 holds the tile's decimated history, written there by k_hp's block t: consecutive
    // block indices would spread them over four XCDs, each fetching the same lines.
    const int per = b.S_pad / PK_SPB;   // blocks per frame
    const int f_begin = chain ? item / per : 0, f_end = chain ? f_begin + 1 : g;
    int tile, sub_;
    xcd_tile_block(item - f_begin * per, b.NT, TILE / PK_SPB, tile, sub_);
    const int q0 = sub_ * PK_SPB;   // first stream of this block within its tile
    if (tile * TILE + q0 >= b.S) return;   // (a block whose streams are all padding -- the last tile of a batch that is not a multiple of 64 -- has nothing to do)
    // ... or all held (nnn_batch_hold_streams).  The mask is constant for a call: the blocks of these streams return in every frame of a
    // chained launch -- each after taking its ticket -- so none is ever waited for
    // (the block's sixteen bits of the tile's word as one 16-bit load: the 64-bit shift and mask cost the one-frame instantiation, which sits at
    // its register limit, four more spilled registers)
    static_assert(PK_SPB == 16, "the block's bits of the tile's word are read as one little-endian 16-bit value");
    if (HELD && b.live && ((const unsigned short *)b.live)[tile * (TILE / PK_SPB) + sub_] == 0) return;
    const int min_period = PITCH_MIN / 2, max_period = PITCH_MAX / 2;
    const bool dec_lane = wave == 0 && lane0 < PK_SPB;                // lane = stream decisions
    int last_period = 0;
    float last_gain = 0.0f;
    if (dec_lane && f_begin == 0) {
        last_period = NNN_TI(b.last_period, 1, tile, q0 + s)[0];
        last_gain = NNN_TI(b.last_gain, 1, tile, q0 + s)[0];
    }
    // (the head waves' sums travel with the window: asked for where they are used, their trip to memory stood on the critical path)
    const float head_c0 = (lpc_here == 2 && wave < 5 && lane0 < PK_SPB) ? b.lpc_head[((size_t)tile * 5 + wave) * TILE + q0 + lane0] : 0.0f;
    float win[PK_CH], fir[5];
    pk_window_load(b, sp0 + f_begin, tile, q0, (int)threadIdx.x, win, fir);
    for (int f = f_begin; f < f_end; f++) {
        lane = launder_v(lane0);   // keep the frame loop's addresses inside the loop (see launder_v)
        s = lane & 15;
        q = lane >> 4;
        const int sl = q0 + s;
        NNN_STAMP(b, 0);
        const int tid = 64 * wave + lane, col = tid & 15, ch = tid >> 4;
        const int qi = ((q & 1) << 1) | (q >> 1);   // inner-product partial of this lane: q = 0, 2 | 1, 3 over the wave's quarters
        const int chc = ch < PK_NCH ? ch : PK_NCH - 1;   // (idle threads shadow the last chunk's reads and store nothing)
        float *chE = L.pb + (chc * (PK_CH / 2)) * PK_SPB + col, *chO = chE + PK_ODD;   // this thread's chunk: rows 2m / 2m + 1 at ch?[16 m]
        // ---- the window -> LDS
        if (ch < PK_NCH) {
#pragma unroll
            for (int m = 0; m < PK_CH / 2; m++) { chE[m * PK_SPB] = win[2 * m]; chO[m * PK_SPB] = win[2 * m + 1]; }
        }
        __syncthreads();
        NNN_STAMP(b, 1);
        // (the autocorrelation and the Levinson recursion that stood here -- two waves busy for a fifth of the block's time, six waiting
        // -- are k_lpc's now: lane = stream, ahead of this launch; the FIR taps arrive with the window)
        if (lpc_here) {
            // ... except for a lone frame: one lag per wave on waves 0 .. 4, lane = stream; the window is in LDS (row r of stream s at
            // pk_at(r, s), row 0 already the frame's special first element)
            float *acs = &L.u.c.xc[0][0], *firs = &L.u.c.xc[8][0];   // [5][16] each, in space the coarse search takes later
            if (wave < 5 && lane < PK_SPB) {   // wave w: lag w of the block's 16 streams (lane = stream)
                const float *pbs = L.pb + lane;
                // (`lpc_here` == 2: k_hp2's head waves took the first LPC_HEAD_BLK blocks of every sum while the frame was being filtered)
                const int blk0 = lpc_here == 2 ? LPC_HEAD_BLK : 0;
                const float c0 = head_c0;
                float a;
                if (wave == 0) a = pk_autocorr<0>(pbs, blk0, c0);
                else if (wave == 1) a = pk_autocorr<1>(pbs, blk0, c0);
                else if (wave == 2) a = pk_autocorr<2>(pbs, blk0, c0);
                else if (wave == 3) a = pk_autocorr<3>(pbs, blk0, c0);
                else a = pk_autocorr<4>(pbs, blk0, c0);
                acs[wave * PK_SPB + lane] = a;
            }
            __syncthreads();
            if (dec_lane) {
                float ac[5], taps[5];
#pragma unroll
                for (int i = 0; i < 5; i++) ac[i] = acs[i * PK_SPB + s];
                lpc_finish(b, tile, sl, sp0[f].slot, ac, taps);
#pragma unroll
                for (int i = 0; i < 5; i++) firs[i * PK_SPB + s] = taps[i];
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 5; i++) fir[i] = firs[i * PK_SPB + col];
        }
        // ---- FIR5 with zero initial memory, in place (ref: src/pitch.rs:407-429): the chunk's inputs are still in the
        //      thread's registers, the five rows before it come from LDS before anyone overwrites them
        {
            float v[PK_CH + 5];
            {
                const int hb = chc > 0 ? 0 : 3 * PK_SPB;   // chunk 0 has no rows before it: read in range, use zeros
                const float h0 = chO[hb - 3 * PK_SPB], h1 = chE[hb - 2 * PK_SPB], h2 = chO[hb - 2 * PK_SPB], h3 = chE[hb - 1 * PK_SPB],
                            h4 = chO[hb - 1 * PK_SPB];
                v[0] = chc > 0 ? h0 : 0.0f; v[1] = chc > 0 ? h1 : 0.0f; v[2] = chc > 0 ? h2 : 0.0f; v[3] = chc > 0 ? h3 : 0.0f;
                v[4] = chc > 0 ? h4 : 0.0f;
#pragma unroll
                for (int u = 0; u < PK_CH; u++) v[5 + u] = win[u];
            }
            __syncthreads();   // every chunk has its inputs
            if (ch < PK_NCH) {
                // Two consecutive outputs are independent sums with the same coefficients: the halves of packed instructions (each half
                // rounds like the single instruction; products and sums in the reference's order, left to right).  Output pair m needs
                // the inputs as pairs in both alignments, VE[i] = (v[2i], v[2i+1]) and VO[i] = (v[2i+1], v[2i+2]): 10 packed
                // instructions per two outputs where scalar code issued 20 (round 5; the second alignment costs a register move per pair).
                const v2f N01 = mk2(fir[0], fir[1]), N23 = mk2(fir[2], fir[3]), N4 = mk2(fir[4], fir[4]);
                float *tap = b.taps ? NNN_TIF(b, xlp_ti, XLP, f, tile, q0 + col) + (size_t)(ch * PK_CH) * TILE : nullptr;
#pragma unroll
                for (int m = 0; m < PK_CH / 2; m++) {
                    const v2f VE0 = mk2(v[2 * m], v[2 * m + 1]), VO0 = mk2(v[2 * m + 1], v[2 * m + 2]);
                    const v2f VE1 = mk2(v[2 * m + 2], v[2 * m + 3]), VO1 = mk2(v[2 * m + 3], v[2 * m + 4]);
                    const v2f VE2 = mk2(v[2 * m + 4], v[2 * m + 5]), VO2 = mk2(v[2 * m + 5], v[2 * m + 6]);
                    // out = x + n0 m0 + n1 m1 + n2 m2 + n3 m3 + n4 m4, left to right (m0 = previous input, ...)
                    v2f o = pk_add(VO2, pk_mul_bx(N01, VE2));
                    o = pk_add(o, pk_mul_by(N01, VO1));
                    o = pk_add(o, pk_mul_bx(N23, VE1));
                    o = pk_add(o, pk_mul_by(N23, VO0));
                    o = pk_add(o, pk_mul_bx(N4, VE0));
                    if (tap) { tap[(size_t)(2 * m) * TILE] = o.x; tap[(size_t)(2 * m + 1) * TILE] = o.y; }
                    chE[m * PK_SPB] = o.x;
                    chO[m * PK_SPB] = o.y;
                }
            }
            if (ch < PK_NCH) {
                // for the certified coarse search: the chunk's 16 even rows -- the 4x-decimated signal -- as bf16 (to nearest) and their energy.
                // Read back from LDS: held in registers through the FIR they cost the kernel spills (it sits at its 128-register limit there).
                const float *ce = L.pb + launder_v((chc * (PK_CH / 2)) * PK_SPB + col);
                unsigned *pl = (unsigned *)((col < PK_SPB / 2 ? (unsigned short *)&L.ckf[0][0] : L.u.a.plane) + (col & 7) * PK_PLW + (PK_CH / 2) * ch);
                unsigned nz = 0;
                float bs = 0.0f;
#pragma unroll
                for (int m = 0; m < PK_CH / 2; m += 2) {
                    const float e0 = ce[m * PK_SPB], e1 = ce[(m + 1) * PK_SPB];
                    pl[m >> 1] = pk_bf16_rn(e0, e1);
                    bs += e0 * e0;
                    bs += e1 * e1;
                    nz |= (__float_as_uint(e0) | __float_as_uint(e1)) << 1;
                }
                // (a block with any nonzero value has a nonzero sum -- squares underflow; a NaN or an infinity stays what it is)
                L.u.a.bsum[col][ch] = (nz != 0 && bs < 0x1p-120f) ? 0x1p-120f : bs;
            }
            if (tid < PK_SPB * 5 + 2) (&L.u.a.mask[0][0])[tid] = 0u;   // the survivors' masks, count and the full-search flag
        }
        __syncthreads();
        NNN_STAMP(b, 4);
        // ---- coarse search (ref: src/pitch.rs:83-84 -> :296-363, :372-405).  find_best_pitch returns the two lags with the largest
        //      corr^2 / energy and nothing else of the 147 cross-correlations is ever used, so most of them need not be exact
        //      (round 6).  Certified search:
        //      (1) every correlation APPROXIMATELY, on the matrix cores: D[i][j] = sum_k A[i][k] B[k][j] with A[i][k] = x4[k - i]
        //          (zero outside 0 .. 239), B[k][j] = y4[k + 16 j] is lag i + 16 j -- eight v_mfma_f32_16x16x32_bf16 per stream, the
        //          operands the signal rounded to bf16 (the FIR left that plane in LDS).  Rigorous error, from the energies of the 16-value
        //          blocks the window covers: |approx - reference| <= e = PK_EPS sqrt(|x4|^2 W_j), W_j >= |y4[16 j .. 16 j + 255]|^2.
        //      (2) with the exact running energy den_L of every lag (the reference's own serial scan): lag L certainly scores at least
        //          lo_L^2 = (c_L - e)^2 / den_L (if c_L - e > 0) and at most hi_L^2 = (c_L + e)^2 / den_L.  Let T be the SECOND largest lo.
        //          A lag with hi_L < T is beaten by two lags whatever its exact value: it cannot be in the final pair, and -- being below
        //          both of them by more than the comparisons' own rounding -- it cannot change which of the others end up there
        //          (DESIGN.md section 4.1 has the argument).  Everything else SURVIVES: typically two to five lags per stream.
        //      (3) the survivors' sums exactly, in the reference's order, lane = (stream, lag); find_best_pitch over them in lag order.
        //      Blocks where that does not apply -- a stream with non-finite or extreme values, fewer than two certain lags and many
        //      candidates, parity taps that want all 147 values -- take the full search below: round 5's code, every lag exact.
        //      Roles: waves 0 .. 4 the search (streams wave, wave + 5, wave + 10 side by side, so that one's latencies are another's issue
        //      slots), waves 5, 6, 7 the three serial energy scans (see pk_chain_*), which run beside it in pieces cut at the search's
        //      barriers; wave 6, whose scan starts with the shortest sum, takes the sixteenth stream behind it.
        //      (2) does NOT wait for the coarse lags' energy scan: it bounds den_L from both sides with the block energies and the bf16
        //      plane (|den_L - (1 + |y4[L .. L + 239]|^2)| is the scan's own rounding, <= 2^-15 (1 + |y4|^2)); the scan's exact values are
        //      first needed by find_best_pitch over the survivors.
        const float *pE = L.pb + s, *pO = pE + PK_ODD;   // rows 2m / 2m + 1 of this lane's stream at p?[16 m]
        const int li = lane & 15, kg = lane >> 4;        // matrix fragments: row / column, k group
        const int cs = lane >> 2, cq = lane & 3;         // scan waves: stream, quad lane
        const float *pcs = L.pb + cs;
        const int wv = launder_s(wave);                  // (keeps this phase's wave-uniform addresses inside the frame loop, see launder_v)
        float chain_y = 0.0f;                            // scan waves: the running energy
        // the search for NS streams s0, s0 + 5, ... on the calling wave (NS a compile-time constant: waves 0 .. 4 take three streams each, wave 6 --
        // whose scan starts with the shortest sum -- the sixteenth behind it)
        auto search = [&](auto ns_, const int s0) {
            constexpr int NS = decltype(ns_)::value;
            f32x4 cacc[NS];                              // approximate correlations of the wave's streams
            // x4[u] sits at halfword 192 + u of the plane; a row of A reaches 15 halfwords before x4[0] (first k-step) and 31 behind x4[239]
            // (last k-step): masked.  Halfword e of lane (li, kg) is x4[32 t + 8 kg + e - li].
            unsigned m0[4], m7[4];
#pragma unroll
            for (int w = 0; w < 4; w++) {
                const int n0 = li - 8 * kg, n1 = 16 + li - 8 * kg;
                m0[w] = (2 * w >= n0 ? 0xffffu : 0u) | (2 * w + 1 >= n0 ? 0xffff0000u : 0u);
                m7[w] = (2 * w < n1 ? 0xffffu : 0u) | (2 * w + 1 < n1 ? 0xffff0000u : 0u);
            }
            const unsigned sh = (unsigned)(li & 1) * 16u;
            const char *pl[NS], *pa[NS];
#pragma unroll
            for (int u = 0; u < NS; u++) {
                const int sq = s0 + 5 * u;
                pl[u] = (const char *)((sq < PK_SPB / 2 ? (const unsigned short *)&L.ckf[0][0] : L.u.a.plane) + (sq & 7) * PK_PLW);
                pa[u] = pl[u] + ((384 + 16 * kg - 2 * li) & ~3);   // A: the word that holds halfword 192 + 8 kg - li
                pl[u] += 16 * kg + 32 * li;                        // B: halfword 8 kg + 16 li
                cacc[u] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            }
#pragma unroll
            for (int t = 0; t < 8; t++) {
#pragma unroll
                for (int u = 0; u < NS; u++) {
                    const uint4 bq = *(const uint4 *)(pl[u] + 64 * t);
                    const unsigned *d = (const unsigned *)(pa[u] + 64 * t);
                    const unsigned d0 = d[0], d1 = d[1], d2 = d[2], d3 = d[3], d4 = d[4];
                    uint4 aq = make_uint4(align_bits(d1, d0, sh), align_bits(d2, d1, sh), align_bits(d3, d2, sh), align_bits(d4, d3, sh));
                    if (t == 0) { aq.x &= m0[0]; aq.y &= m0[1]; aq.z &= m0[2]; aq.w &= m0[3]; }
                    if (t == 7) { aq.x &= m7[0]; aq.y &= m7[1]; aq.z &= m7[2]; aq.w &= m7[3]; }
                    cacc[u] = mfma_16x16x32_bf16(aq, bq, cacc[u]);
                }
            }
            NNN_STAMPW(b, 2, wave == 0);
            if (b.taps == 2) {   // (test mode: the cross-correlation tap keeps NaN where a lag was ruled out)
                for (int u = 0; u < NS; u++)
                    for (int i = lane; i < NLAG1; i += 64) NNN_TIF(b, xc1, NLAG1, f, tile, q0 + s0 + 5 * u)[(size_t)i * TILE] = __builtin_nanf("");
            }
            // ---- (2) who survives.  Element r of lane (li, kg) of D is row 4 kg + r, column li: lag 16 li + 4 kg + r.
            const int lj = li < 10 ? li : 9;   // (columns 10 .. 15 hold no lag: they follow column 9 and are masked)
            float chp[NS][4], clo[NS][4], m1[NS], m2[NS];
            unsigned cfl = 0;                  // bit u: stream u has nothing but zeros in x4; bit 4 + u: stream u is not ordinary
#pragma unroll
            for (int u = 0; u < NS; u++) {
                const int sq = s0 + 5 * u;
                const float *bsr = L.u.a.bsum[sq];
                // W_j = blocks j .. j + 15 (>= the energy of the 240-value window of every lag of column j); |x4|^2 = blocks 12 .. 26 = W_12
                float wub = 0.0f;
#pragma unroll
                for (int n = 0; n < 4; n++) { const int ix = li + 4 * kg + n; wub += ix < 27 ? bsr[ix] : 0.0f; }
                wub += wave_xor16(wub, lane);
                wub += wave_xor32(wub, lane);
                const float xxu = lane_value(wub, 12), wtot = lane_value(wub, 0) + lane_value(wub, 11);
                // the search is certified for ordinary values only: no NaN or infinity, no product of the comparisons in find_best_pitch
                // near the ends of the f32 range (|corr| <= sqrt(|x4|^2 W) <= 2^41, energies <= 2^41 + 1: corr^2 * energy < 2^124)
                const bool odd = !(wtot <= 0x1p41f) || !(xxu >= 0x1p-60f);
                const bool xzero = xxu == 0.0f;   // every x4 is zero: every correlation is zero (or NaN), none is > 0 -- no survivor
                cfl |= (xzero ? 1u : 0u) << u | ((odd && !xzero) ? 16u : 0u) << u;
                const float e = PK_EPS * fast_sqrt(xxu) * fast_sqrt(wub);   // (two roots: the product of two small energies would underflow)
                // den_L from both sides.  The window of lag 16 j + i is the tail of block j from value i on, blocks j + 1 .. j + 14 whole (their
                // f32 energies) and the first i values of block j + 15: the two partial blocks from the bf16 plane, this lane's quarter of each
                // as suffix / prefix sums, the other quarters' totals from the lanes that hold them.
                const unsigned short *pv = (sq < PK_SPB / 2 ? (const unsigned short *)&L.ckf[0][0] : L.u.a.plane) + (sq & 7) * PK_PLW + 16 * lj + 4 * kg;
                const uint2 av = *(const uint2 *)pv, cv = *(const uint2 *)(pv + 240);
                const float a0 = __uint_as_float(av.x << 16), a1 = __uint_as_float(av.x & 0xffff0000u), a2 = __uint_as_float(av.y << 16), a3 = __uint_as_float(av.y & 0xffff0000u);
                const float c0 = __uint_as_float(cv.x << 16), c1 = __uint_as_float(cv.x & 0xffff0000u), c2 = __uint_as_float(cv.y << 16), c3 = __uint_as_float(cv.y & 0xffff0000u);
                float sfx[4], pfx[4];
                sfx[3] = a3 * a3; sfx[2] = a2 * a2 + sfx[3]; sfx[1] = a1 * a1 + sfx[2]; sfx[0] = a0 * a0 + sfx[1];
                pfx[0] = 0.0f; pfx[1] = c0 * c0; pfx[2] = pfx[1] + c1 * c1; pfx[3] = pfx[2] + c2 * c2;
                const float qa = sfx[0], qc = pfx[3] + c3 * c3;
                const float qa1 = wave_xor16(qa, lane), qa2 = wave_xor32(qa, lane), qa3 = wave_xor32(qa1, lane);   // the quarter sums of lanes kg ^ 1, kg ^ 2, kg ^ 3
                const float qc1 = wave_xor16(qc, lane), qc2 = wave_xor32(qc, lane), qc3 = wave_xor32(qc1, lane);
                const float sa = ((kg ^ 1) > kg ? qa1 : 0.0f) + ((kg ^ 2) > kg ? qa2 : 0.0f) + ((kg ^ 3) > kg ? qa3 : 0.0f);   // the quarters behind this one
                const float sc = ((kg ^ 1) < kg ? qc1 : 0.0f) + ((kg ^ 2) < kg ? qc2 : 0.0f) + ((kg ^ 3) < kg ? qc3 : 0.0f);   // the quarters ahead of this one
                const float s14 = wub - bsr[lj] - bsr[lj + 15];
                const float slack = 0x1p-22f * wub + 0x1p-15f * (1.0f + wtot);   // the subtraction above; the serial scan's own rounding
                m1[u] = -INFINITY;
                m2[u] = -INFINITY;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int Lr = 4 * kg + r + 16 * li;
                    const bool valid = li < 10 && Lr < NLAG1;
                    const float pr = (sfx[r] + sa) + (pfx[r] + sc);   // the partial blocks' share, within 2^-6.98 (bf16 values squared)
                    const float dlo = fmaxf(1.0f + (s14 + pr * (1.0f - 0x1p-6f) - slack), 1.0f), dhi = 1.0f + (s14 + pr * (1.0f + 0x1p-6f) + slack);
                    const float ch = cacc[u][r] + e;
                    chp[u][r] = (valid && ch > 0.0f) ? ch * fast_rsq(dlo) : -1.0f;   // hi_L where the lag may be positive at all
                    clo[u][r] = valid ? (cacc[u][r] - e) * fast_rsq(dhi) : -INFINITY;
                    const float lo_ = fminf(m1[u], clo[u][r]);
                    m1[u] = fmaxf(m1[u], clo[u][r]);
                    m2[u] = fmaxf(m2[u], lo_);
                }
            }
            // the second largest lo of each stream: rows of 16 lanes by DPP, the four rows through scalars
#define NNN_TOP2(u, n1, n2) do { const float a1_ = (n1), a2_ = (n2), lo_ = fminf(m1[u], a1_); m1[u] = fmaxf(m1[u], a1_); m2[u] = fmaxf(lo_, fmaxf(m2[u], a2_)); } while (0)
#pragma unroll
            for (int u = 0; u < NS; u++) NNN_TOP2(u, row_partner<0>(m1[u]), row_partner<0>(m2[u]));
#pragma unroll
            for (int u = 0; u < NS; u++) NNN_TOP2(u, row_partner<1>(m1[u]), row_partner<1>(m2[u]));
#pragma unroll
            for (int u = 0; u < NS; u++) NNN_TOP2(u, row_partner<2>(m1[u]), row_partner<2>(m2[u]));
#pragma unroll
            for (int u = 0; u < NS; u++) NNN_TOP2(u, row_partner<3>(m1[u]), row_partner<3>(m2[u]));
#pragma unroll
            for (int u = 0; u < NS; u++) {
                const float b1 = lane_value(m1[u], 16), b2 = lane_value(m2[u], 16), c1 = lane_value(m1[u], 32), c2 = lane_value(m2[u], 32),
                            d1 = lane_value(m1[u], 48), d2 = lane_value(m2[u], 48);
                m1[u] = lane_value(m1[u], 0);
                m2[u] = lane_value(m2[u], 0);
                NNN_TOP2(u, b1, b2);
                NNN_TOP2(u, c1, c2);
                NNN_TOP2(u, d1, d2);
            }
#undef NNN_TOP2
            bool want_full = false;
#pragma unroll
            for (int u = 0; u < NS; u++) {
                const int sq = s0 + 5 * u;
                // two lags are certainly positive and certainly in the ordinary range: T = m2, less the rounding of this arithmetic, v_rsq_f32's
                // ulp and the margin of (2); else every lag that may be positive survives
                const bool two = m2[u] > 0x1p-40f;
                const float thr = two ? m2[u] * (1.0f - 0x1p-10f) : 0.0f;
                const bool xzero = (cfl >> u) & 1u;
                unsigned long long bal[4];
                unsigned tot = 0;
                bool keep[4];
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    keep[r] = !xzero && chp[u][r] > 0.0f && chp[u][r] >= thr;
                    bal[r] = wave_ballot(keep[r]);
                    tot += (unsigned)__builtin_popcountll(bal[r]);
                }
                if (tot != 0) {
                    unsigned base = 0;
                    if (lane == 0) base = lds_add_u32(&L.u.a.count, tot);
                    base = __float_as_uint(lane_value(__uint_as_float(base), 0));
                    want_full |= base + tot > (unsigned)PK_CAP;
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int Lr = 4 * kg + r + 16 * li;
                        const unsigned ix = base + lane_rank(bal[r], lane);
                        if (keep[r] && ix < (unsigned)PK_CAP) {
                            L.u.a.list[ix] = (unsigned short)((sq << 8) | Lr);
                            lds_or_u32(&L.u.a.mask[sq][Lr >> 5], 1u << (Lr & 31));
                        }
                        base += (unsigned)__builtin_popcountll(bal[r]);
                    }
                }
                want_full |= ((cfl >> (4 + u)) & 1u) != 0 || tot > (unsigned)PK_RMAX;
            }
            if (lane == 0 && (want_full || b.taps == 1)) L.u.a.full = 1u;
        };
        if (wv < 5) search(std::integral_constant<int, 3>(), wv);
        else if (wv == 7) {
            chain_y = pk_chain_coarse_start(pcs, cq);
            chain_y = pk_chain_coarse(pcs, cq, chain_y, 0, PK_COARSE_K, L.u.a.denck[cs]);
            NNN_STAMPW(b, 3, true);
        } else if (wv == 5) {
            chain_y = pk_chain_fine_start(pcs, cq, 1.0f, 0, PK_SEG_FS);
            NNN_STAMPW(b, 28, true);
        } else if (wv == 6) {
            chain_y = pk_chain_yy_start(pcs, cq);
            NNN_STAMPW(b, 29, true);
            search(std::integral_constant<int, 1>(), 15);
        }
        __syncthreads();   // (the planes are read: the scans' check points may take their place; the survivors are listed)
        NNN_STAMP(b, 5);
        const bool full = L.u.a.full != 0;           // block-uniform
        const unsigned nsurv = L.u.a.count;
        if (full) {
            __syncthreads();   // (everyone has read the flag: the full search's arrays take the space)
            // ---- full search: the cross-correlation of every lag on waves 0..2, the running energy of the coarse lags on wave 3
            const int grp = 4 * wave + q;
            if (grp < PK_NG) {
                // xcorr[L] = sum_j x4[j] y4[L + j], x4[j] = p[384 + 2j], y4[m] = p[2m] (the even rows, compact): a sequential sum
                // per lag (ref: src/pitch.rs:296-363).  Lags L0 .. L0 + 11 in six packed accumulators, L0 + 12 single.  The y window
                // w[i] = y4[L0 + j + i] is kept as pairs in both alignments, PE[t] = (w[2t], w[2t+1]) and PO[t] = (w[2t+1], w[2t+2]):
                // tap k multiplies pairs w[k+2n], w[k+2n+1], whichever alignment that is, with x4[j+k] from either half of its pair.
                const int L0 = PK_LC * grp;
                const float *yb = L.pb + L0 * PK_SPB + s, *xb = L.pb + 192 * PK_SPB + s;
                v2f acc2[PK_NP], PE[PK_NT], PO[PK_NT];
                float acc1 = 0.0f;
#pragma unroll
                for (int n = 0; n < PK_NP; n++) acc2[n] = mk2(0.0f, 0.0f);
#pragma unroll
                for (int t = 0; t < PK_NT - PK_JB / 2; t++) {
                    PE[t] = mk2(yb[(2 * t) * PK_SPB], yb[(2 * t + 1) * PK_SPB]);
                    PO[t] = mk2(yb[(2 * t + 1) * PK_SPB], yb[(2 * t + 2) * PK_SPB]);
                }
#pragma unroll 5   // (the window's register pairs come round after five steps: no moves at the back edge)
                for (int j = 0; j < 240; j += PK_JB) {
                    const float *yj = yb + j * PK_SPB, *xj = xb + j * PK_SPB;
                    v2f X[PK_JB / 2];
#pragma unroll
                    for (int t = 0; t < PK_JB / 2; t++) X[t] = mk2(xj[(2 * t) * PK_SPB], xj[(2 * t + 1) * PK_SPB]);
#pragma unroll
                    for (int t = PK_NT - PK_JB / 2; t < PK_NT; t++) {
                        PE[t] = mk2(yj[(2 * t) * PK_SPB], yj[(2 * t + 1) * PK_SPB]);
                        PO[t] = mk2(yj[(2 * t + 1) * PK_SPB], yj[(2 * t + 2) * PK_SPB]);
                    }
#pragma unroll
                    for (int k = 0; k < PK_JB; k++) {
                        const v2f xp2 = X[k >> 1];
#pragma unroll
                        for (int n = 0; n < PK_NP; n++) {
                            const v2f wp = (k & 1) ? PO[(k >> 1) + n] : PE[(k >> 1) + n];
                            acc2[n] = pk_add(acc2[n], (k & 1) ? pk_mul_by(xp2, wp) : pk_mul_bx(xp2, wp));
                        }
                        const float w1 = (k & 1) ? PO[(k >> 1) + PK_NP].x : PE[(k >> 1) + PK_NP].x;
                        acc1 = sadd(acc1, ((k & 1) ? xp2.y : xp2.x) * w1);
                    }
#pragma unroll
                    for (int t = 0; t < PK_NT - PK_JB / 2; t++) { PE[t] = PE[t + PK_JB / 2]; PO[t] = PO[t + PK_JB / 2]; }
                }
                float acc[PK_LC];
#pragma unroll
                for (int n = 0; n < PK_NP; n++) { acc[2 * n] = acc2[n].x; acc[2 * n + 1] = acc2[n].y; }
                acc[PK_LC - 1] = acc1;
#pragma unroll
                for (int i = 0; i < PK_LC; i++)   // (what find_best_pitch needs of a correlation: its square if it is positive)
                    if (L0 + i < NLAG1) L.u.c.xc[L0 + i][s] = acc[i] > 0.0f ? acc[i] * acc[i] : __builtin_nanf("");
                if (b.taps) {
                    float *o = NNN_TIF(b, xc1, NLAG1, f, tile, sl);
#pragma unroll
                    for (int i = 0; i < PK_LC; i++)
                        if (L0 + i < NLAG1) o[(size_t)(L0 + i) * TILE] = acc[i];
                }
            }
            if (wave == PK_XW && lane < PK_SPB) {
                // the running energy every coarse lag sees in find_best_pitch (ref: src/pitch.rs:83 -> :380-402): even rows only
                float ysq = 1.0f;
#pragma nounroll
                for (int j0 = 0; j0 < 240; j0 += 8) {
                    float v[8];
#pragma unroll
                    for (int i = 0; i < 8; i++) v[i] = pE[(j0 + i) * PK_SPB];
#pragma unroll
                    for (int i = 0; i < 8; i++) ysq += v[i] * v[i];
                }
#pragma nounroll
                for (int i0 = 0; i0 < NLAG1; i0 += 7) {
                    float a[7], d[7];
#pragma unroll
                    for (int i = 0; i < 7; i++) { a[i] = pE[(i0 + i + 240) * PK_SPB]; d[i] = pE[(i0 + i) * PK_SPB]; }
#pragma unroll
                    for (int i = 0; i < 7; i++) {
                        L.u.c.ysq[i0 + i][s] = ysq;
                        ysq += a[i] * a[i] - d[i] * d[i];
                        ysq = fmaxf(ysq, 1.0f);
                    }
                }
            }
            __syncthreads();
        }
        NNN_STAMP(b, 63);
        // ---- find_best_pitch over the coarse lags (ref: src/pitch.rs:372-405, call site :83-84): over the survivors' exact sums (certified
        //      search: waves 0 .. 4 and 7 make them, wave 0 scans) or over all 147 (full search: wave 0, a serial scan); beside it, on
        //      waves 5 and 6, the rest of the two energy scans whose results are looked up later in the frame
        int lo1 = 0, lo2 = 0;
        if (wv == 5) chain_y = pk_chain_fine(pcs, cq, cs, chain_y, 0, PK_SEG_F1, L.ckf);   // (the rest beside find_best, below)
        else if (wv == 6) {
            if (cq == 0) L.cky[0][cs] = chain_y;   // xx = yy_lookup[0]
            chain_y = pk_chain_yy(pcs, cq, cs, chain_y, 0, PK_YY_B, L.cky);
        } else if (wv != 7 && !full) {
            // (3) lane = (stream, lag) of the survivor list: xcorr[L] = sum_j x4[j] y4[L + j], x4[j] = p[384 + 2j], y4[m] = p[2m], a sequential
            //     sum (ref: src/pitch.rs:296-363), two taps per packed multiply, the adds in order
#pragma nounroll
            for (unsigned e0 = 64u * (unsigned)wv; e0 < nsurv; e0 += 64u * 5u) {
                const unsigned en = e0 + (unsigned)lane;
                if (en < nsurv) {
                    const unsigned ent = L.u.a.list[en];
                    const int se = (int)(ent >> 8), Le = (int)(ent & 255u);
                    const float *xp = L.pb + 192 * PK_SPB + se, *yp = L.pb + Le * PK_SPB + se;
                    const float c = pk_dot240(xp, yp);
                    // its place among the stream's survivors, in lag order
                    const unsigned *mk = L.u.a.mask[se];
                    int rk = 0;
#pragma unroll
                    for (int w = 0; w < 5; w++) {
                        const unsigned mw = mk[w], below = w < (Le >> 5) ? mw : (w == (Le >> 5) ? mw & ((1u << (Le & 31)) - 1u) : 0u);
                        rk += __builtin_popcount(below);
                    }
                    // the energy the lag saw in find_best_pitch: the scan's own steps from the check point below it (<= 3)
                    float dy = L.u.a.denck[se][Le >> 2];
                    {
                        const float *yq = L.pb + (Le & ~3) * PK_SPB + se;
                        float ra[3], rd[3];
#pragma unroll
                        for (int i = 0; i < 3; i++) { ra[i] = yq[(i + 240) * PK_SPB]; rd[i] = yq[i * PK_SPB]; }
#pragma unroll
                        for (int i = 0; i < 3; i++) {
                            const float yn = fmaxf(dy + (ra[i] * ra[i] - rd[i] * rd[i]), 1.0f);
                            dy = i < (Le & 3) ? yn : dy;
                        }
                    }
                    L.u.a.slotv[se][rk] = c;
                    L.u.a.slotl[se][rk] = Le;
                    L.u.a.slotd[se][rk] = dy;
                    if (b.taps) NNN_TIF(b, xc1, NLAG1, f, tile, q0 + se)[(size_t)Le * TILE] = c;
                }
            }
        }
        if (full) {
            if (wv == 5) chain_y = pk_chain_fine(pcs, cq, cs, chain_y, PK_SEG_F1, PK_FINE_K, L.ckf);
            if (dec_lane) {
                BestPitch bp;
                bp.init();
                float c[7], e[7];
#pragma unroll
                for (int i = 0; i < 7; i++) { c[i] = L.u.c.xc[i][s]; e[i] = L.u.c.ysq[i][s]; }
#pragma nounroll
                for (int i0 = 0; i0 < NLAG1; i0 += 7) {
                    float cn[7], en[7];   // the next seven lags travel while these are judged
                    const int i1 = i0 + 7 < NLAG1 ? i0 + 7 : i0;
#pragma unroll
                    for (int i = 0; i < 7; i++) { cn[i] = L.u.c.xc[i1 + i][s]; en[i] = L.u.c.ysq[i1 + i][s]; }
#pragma unroll
                    for (int i = 0; i < 7; i++) bp.update_sq(i0 + i, c[i], e[i]);
#pragma unroll
                    for (int i = 0; i < 7; i++) { c[i] = cn[i]; e[i] = en[i]; }
                }
                if (b.taps) {
                    int *o = (int *)NNN_TIF(b, best1, 2, f, tile, sl);
                    o[0] = bp.best;
                    o[TILE] = bp.second;
                }
                lo1 = 2 * bp.best - 2;
                lo2 = 2 * bp.second - 2;
                NNN_STAMP(b, 61);
            }
        } else {
            __syncthreads();   // (the survivors' sums of waves 0 .. 4, the coarse lags' energies of wave 7)
            NNN_STAMP(b, 27);
            if (wv == 5) chain_y = pk_chain_fine(pcs, cq, cs, chain_y, PK_SEG_F1, PK_FINE_K, L.ckf);
            if (wave == 0) {
                // find_best_pitch over the stream's survivors in lag order, with the energy each of them saw
                BestPitch bp;
                bp.init();
                int ns = 0;
#pragma unroll
                for (int w = 0; w < 5; w++) ns += lane < PK_SPB ? __builtin_popcount(L.u.a.mask[s][w]) : 0;
                float nc = 0.0f, nd = 1.0f;
                int nl = 0;
                if (ns > 0) { nl = L.u.a.slotl[s][0]; nc = L.u.a.slotv[s][0]; nd = L.u.a.slotd[s][0]; }
                for (int k = 0; wave_ballot(k < ns) != 0ull; k++) {
                    const int cl = nl;
                    const float cc = nc, cd = nd;
                    if (k + 1 < ns) { nl = L.u.a.slotl[s][k + 1]; nc = L.u.a.slotv[s][k + 1]; nd = L.u.a.slotd[s][k + 1]; }   // (the next one travels)
                    if (k < ns) bp.update(cl, cc, cd);
                }
                if (dec_lane) {
                    if (b.taps) {
                        int *o = (int *)NNN_TIF(b, best1, 2, f, tile, sl);
                        o[0] = bp.best;
                        o[TILE] = bp.second;
                    }
                    lo1 = 2 * bp.best - 2;
                    lo2 = 2 * bp.second - 2;
                }
                NNN_STAMP(b, 61);
            }
        }
        // (wave 0 alone read the search's arrays in this phase; the scans' waves write their check points only: its lanes may put the fine
        // search's windows into the space -- in the partial sums' layout -- before the barrier)
        if (wave == 0) wave_lds_sync();
        if (dec_lane) {
            L.u.f.lo[0][s] = lo1;
            L.u.f.lo[1][s] = lo2;
            if (s == 0) L.u.f.any_refine = 0;
        }
        __syncthreads();   // the coarse arrays are dead: their space takes the partial sums from here on
        NNN_STAMP(b, 6);
        // ---- fine cross-correlation at the <= 10 lags within +-2 of 2*best / 2*second (ref: src/pitch.rs:88-96): wave w
        //      takes lags lo1 + w and lo2 + w
        if (wave < 5) {
            const int la = L.u.f.lo[0][s] + wave, lb = L.u.f.lo[1][s] + wave;
            const bool va = la >= 0 && la < NLAG2, vb = lb >= 0 && lb < NLAG2;
            const int yr[2] = {va ? la : 0, vb ? lb : 0};
            float acc[2];
            pk_inner<2>(L.pb, s, qi, yr, acc);
            L.u.f.part[wave][qi][s] = acc[0];
            L.u.f.part[5 + wave][qi][s] = acc[1];
        } else if (wave == 5) {   // (beside it, on a wave the cross-correlation leaves idle)
            if (q < 2) {
                // the energy lags lo .. lo + 4 of window q saw: from the check point below the first of them, the scan's own
                // steps (at most 7 + 5; every row is requested before the first step is taken)
                const int lo = L.u.f.lo[q][s], first = lo > 0 ? lo : 0;
                const int i0 = (first < NLAG2 ? first : NLAG2 - 1) & ~(PK_CKF - 1);
                float y = L.ckf[i0 / PK_CKF][s], ev[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
                float ra[PK_CKF + 4], rd[PK_CKF + 4];
#pragma unroll
                for (int st = 0; st < PK_CKF + 4; st++) {
                    const int i = i0 + st < NLAG2 ? i0 + st : NLAG2 - 1;
                    ra[st] = L.pb[pk_at(i + 480, s)];
                    rd[st] = L.pb[pk_at(i, s)];
                }
#pragma unroll
                for (int st = 0; st < PK_CKF + 4; st++) {
#pragma unroll
                    for (int c = 0; c < 5; c++) ev[c] = (i0 + st == lo + c) ? y : ev[c];
                    y += ra[st] * ra[st] - rd[st] * rd[st];
                    y = fmaxf(y, 1.0f);
                }
#pragma unroll
                for (int c = 0; c < 5; c++) L.u.f.ye[5 * q + c][s] = ev[c];
            }
        }
        __syncthreads();
        NNN_STAMP(b, 7);
        // ---- find_best_pitch over the fine lags: xcorr is zero outside the two 5-lag windows, so only they can update the
        //      best pitch; replayed in increasing lag order with the energy each of them saw.  Then the candidate periods.
        Xc2 xc;
        int t0 = 0;
        float xx = 0.0f;
        if (dec_lane) {
            xx = L.cky[0][s];
            xc.lo1 = lo1;
            xc.lo2 = lo2;
            float ye[10];
#pragma unroll
            for (int c = 0; c < 10; c++) {
                const int lag = c < 5 ? lo1 + c : lo2 + (c - 5);
                const bool valid = lag >= 0 && lag < NLAG2;
                float v = L.u.f.part[c][0][s] + L.u.f.part[c][1][s] + L.u.f.part[c][2][s] + L.u.f.part[c][3][s];
                v = fmaxf(v, -1.0f);
                xc.v[c] = valid ? v : 0.0f;
                ye[c] = valid ? L.u.f.ye[c][s] : 0.0f;
            }
            if (b.taps) {
                float *o = NNN_TIF(b, xc2, 10, f, tile, sl);
#pragma unroll
                for (int c = 0; c < 10; c++) o[(size_t)c * TILE] = xc.v[c];
            }
            NNN_STAMP(b, 59);
            BestPitch bp;
            bp.init();
            const int loA = min(lo1, lo2), loB = max(lo1, lo2);
            const bool a_first = lo1 <= lo2;
#pragma unroll
            for (int u = 0; u < 10; u++) {
                const int i = u < 5 ? loA + u : loB + (u - 5);
                const bool on = i >= 0 && i < NLAG2 && (u < 5 || i > loA + 4);
                // the energy of the lower window's lags sits at ye[0..4] when lo1 <= lo2, at ye[5..9] otherwise
                const float e = (u < 5) == a_first ? ye[u < 5 ? u : u - 5] : ye[5 + (u < 5 ? u : u - 5)];
                // (lag i is the u-th of its window: no search needed; where the windows overlap the values are the same)
                const float cv = (u < 5) == a_first ? xc.v[u < 5 ? u : u - 5] : xc.v[5 + (u < 5 ? u : u - 5)];
                if (on) bp.update(i, cv, e);
            }
            int offset = 0;
            if (bp.best > 0 && bp.best < NLAG2 - 1) {
                float a = xc.at(bp.best - 1), bb = xc.at(bp.best), c = xc.at(bp.best + 1);
                if (c - a > 0.7f * (bb - a)) offset = 1;
                else if (a - c > 0.7f * (bb - c)) offset = -1;
            }
            const int psr = 2 * bp.best - offset;
            if (b.taps) NNN_TIF(b, psearch, 1, f, tile, sl)[0] = psr;
            // ---- remove_doubling: the candidates of the decision loop + the two neighbours of t0 (slots 23, 24): if the loop keeps
            //      t0 the final +-1 refinement needs no inner products of its own.  Divisors k >= 13 never get past the loop's
            //      `t1 < min_period` break (t0 <= 383: (2 t0 + 13) / 26 <= 29), so slots exist for k = 2 .. PK_KMAX = 12 only.
            NNN_STAMP(b, 60);
            t0 = (PITCH_MAX - psr) / 2;
            if (t0 > max_period - 1) t0 = max_period - 1;
        #pragma unroll
            for (int e = 0; e < PK_NSLOT; e++) {   // (unrolled: k is a constant in every copy)
                int t;
                if (e == 0) t = t0;
                else if (e >= PK_NE) t = e == PK_NE ? t0 - 1 : t0 + 1;
                else {
                    const int k = 2 + (e - 1) / 2;
                    const int t1 = (2 * t0 + k) / (2 * k);
                    if ((e - 1) & 1) {
                        const int sc = kSecondCheck[k];
                        t = (k == 2) ? ((t1 + t0 > max_period) ? t0 : t0 + t1) : (2 * sc * t0 + k) / (2 * k);
                    } else t = t1;
                }
                L.u.f.cand[e][s] = t;
            }

            L.u.f.xx[s] = xx;
            L.u.f.t0[s] = t0;
        }
        __syncthreads();
        NNN_STAMP(b, 53);
        // ---- yy_lookup at the candidate periods (ref: src/pitch.rs:138-142): one candidate per lane (s, q) of waves 0..5; from the
        //      check point below T, at most four of the scan's steps.  (Read by the decision loop, behind the next barrier.)
        {
            const int e = 4 * wave + q;
            if (e < PK_NE) {
                const int T = L.u.f.cand[e][s], m = T / PK_CKY;
                float y = L.cky[m][s];
                float ra[PK_CKY - 1], rc[PK_CKY - 1];
#pragma unroll
                for (int st = 1; st < PK_CKY; st++) {
                    const int j = PK_CKY * m + st, jc = j <= 384 ? j : 384;   // step j: row 384 - j enters, row 864 - j leaves
                    ra[st - 1] = L.pb[pk_at(384 - jc, s)];
                    rc[st - 1] = L.pb[pk_at(864 - jc, s)];
                }
#pragma unroll
                for (int st = 1; st < PK_CKY; st++) {
                    const float yn = y + (ra[st - 1] * ra[st - 1] - rc[st - 1] * rc[st - 1]);
                    y = PK_CKY * m + st <= T ? yn : y;
                }
                L.u.f.yy[e][s] = fmaxf(y, 0.0f);
            }
        }
        // ---- the candidates' inner products against p[384 ..]: wave w takes slots w, w + 8, w + 16 (wave 0 also slot 24)
        static_assert(PK_NSLOT == 25, "three slots per wave and one more");
        if (wave == 0) {
            int yr[4];
#pragma unroll
            for (int c = 0; c < 4; c++) yr[c] = max_period - L.u.f.cand[8 * c][s];
            float acc[4];
            pk_inner<4>(L.pb, s, qi, yr, acc);
#pragma unroll
            for (int c = 0; c < 4; c++) L.u.f.part[8 * c][qi][s] = acc[c];
        } else {
            int yr[3];
#pragma unroll
            for (int c = 0; c < 3; c++) yr[c] = max_period - L.u.f.cand[wave + 8 * c][s];
            float acc[3];
            pk_inner<3>(L.pb, s, qi, yr, acc);
#pragma unroll
            for (int c = 0; c < 3; c++) L.u.f.part[wave + 8 * c][qi][s] = acc[c];
        }
        // the next frame's window is requested here, behind the candidates' inner products (round 6; round 5: ahead of them; until then behind
        // the FIR): its 32 registers are free through the cross-correlation and the searches, and the ~8 us left of the frame still cover the
        // trip (k_pitch -2.6 %)
        pk_window_load(b, sp0 + f + 1, tile, q0, f + 1 < f_end ? tid : PK_T, win, fir);   // (the group's last frame: nothing to load, and no old value kept)
        if (dec_lane) {
            if (chain && f > 0) {
                // the previous frame of these streams is another workgroup's: wait for its flag, then take its pitch and gain
                const int *flag = (const int *)NNN_TIF(b, pflag, 1, f - 1, tile, q0);
                // (the ticket order guarantees the wait ends; the limit is wall time on the constant clock, not a spin count, so that a
                // predecessor slowed by a shared GPU or a stalled queue is waited for: giving up invalidates the streams' state for good)
                const long long t_wait = realtime_ticks();
                unsigned spins = 0;
                bool lost = false;
                while (flag_read(flag) != seq0 + f - 1 && !lost) {
                    chain_pause();
                    if ((++spins & 255u) == 0 && realtime_ticks() - t_wait > b.handoff_ticks) lost = true;
                }
                if (lost) *b.fault = 1;   // never seen (cannot happen, see the ticket order above): reported to the host, not hung on
                last_period = NNN_TIF(b, pitch, 1, f - 1, tile, sl)[0];
                last_gain = NNN_TIF(b, pgain, 1, f - 1, tile, sl)[0];
            }
            L.u.f.pprev[s] = last_period / 2;
            L.u.f.lgain[s] = last_gain;
        }
        __syncthreads();
        NNN_STAMP(b, 54);
        // ---- decision loop (ref: src/pitch.rs:150-206).  Whether divisor k replaces the best candidate depends on t0, the previous
        //      frame and k's own inner products, not on the other divisors: lane (stream, k) judges k = 2 .. 12 on three waves, the
        //      stream's lane then takes the last k that passed (the loop's break at the first t1 < min_period cuts a suffix: t1
        //      falls with k).
        if (wave < 3) {
            const int k = 2 + 4 * wave + q;
            if (k <= PK_KMAX) {
                auto ipv = [&](int e) { return L.u.f.part[e][0][s] + L.u.f.part[e][1][s] + L.u.f.part[e][2][s] + L.u.f.part[e][3][s]; };
                const int e1 = 1 + 2 * (k - 2), e2 = e1 + 1;
                const int t1 = L.u.f.cand[e1][s], t0s = L.u.f.t0[s];
                const float xxs = L.u.f.xx[s], lg = L.u.f.lgain[s];
                const float g0 = pitch_gain(ipv(0), xxs, L.u.f.yy[0][s]);
                const float xy = (ipv(e1) + ipv(e2)) / 2.0f;
                const float yy = (L.u.f.yy[e1][s] + L.u.f.yy[e2][s]) / 2.0f;
                const float g1 = pitch_gain(xy, xxs, yy);
                int d = t1 - L.u.f.pprev[s];
                if (d < 0) d = -d;
                float cont;
                if (d <= 1) cont = lg;
                else if (d <= 2 && 5 * k * k < t0s) cont = lg / 2.0f;
                else cont = 0.0f;
                float thresh;
                if (t1 < 3 * min_period) thresh = fmaxf(0.85f * g0 - cont, 0.4f);
                else if (t1 < 2 * min_period) thresh = fmaxf(0.9f * g0 - cont, 0.5f);
                else thresh = fmaxf(0.7f * g0 - cont, 0.3f);
                L.u.f.kpass[k][s] = (t1 >= min_period && g1 > thresh) ? 1 : 0;
                L.u.f.kxy[k][s] = xy;
                L.u.f.kyy[k][s] = yy;
                L.u.f.kg[k][s] = g1;
            }
        }
        __syncthreads();
        NNN_STAMP(b, 58);
        int t = 0;
        float pg = 0.0f, gg = 0.0f;
        if (dec_lane) {
            auto ipv = [&](int e) { return L.u.f.part[e][0][s] + L.u.f.part[e][1][s] + L.u.f.part[e][2][s] + L.u.f.part[e][3][s]; };
            t = t0;
            float best_xy = ipv(0), best_yy = L.u.f.yy[0][s];
            gg = pitch_gain(best_xy, xx, best_yy);
            int kw = 0;
#pragma unroll
            for (int k = 2; k <= PK_KMAX; k++) kw = L.u.f.kpass[k][s] ? k : kw;
            if (kw) {
                best_xy = L.u.f.kxy[kw][s];
                best_yy = L.u.f.kyy[kw][s];
                gg = L.u.f.kg[kw][s];
                t = L.u.f.cand[1 + 2 * (kw - 2)][s];
            }
            best_xy = fmaxf(best_xy, 0.0f);
            pg = (best_yy <= best_xy) ? 1.0f : best_xy / (best_yy + 1.0f);
            L.u.f.tsel[s] = t;
            if (t != t0) L.u.f.any_refine = 1;
        }
        __syncthreads();
        NNN_STAMP(b, 55);
        // ---- final +-1 refinement: the inner products at t - 1, t, t + 1 (the same sums whichever way they are obtained)
        const bool refine = L.u.f.any_refine != 0;   // block-uniform
        if (refine) {
            if (wave < 3) {
                const int yr[1] = {max_period - (L.u.f.tsel[s] + wave - 1)};
                float acc[1];
                pk_inner<1>(L.pb, s, qi, yr, acc);
                L.u.f.part[32 + wave][qi][s] = acc[0];
            }
            __syncthreads();
        }
        NNN_STAMP(b, 56);
        if (dec_lane) {
            auto ipv = [&](int e) { return L.u.f.part[e][0][s] + L.u.f.part[e][1][s] + L.u.f.part[e][2][s] + L.u.f.part[e][3][s]; };
            float x3[3];
            if (t == t0) { x3[0] = ipv(PK_NE); x3[1] = ipv(0); x3[2] = ipv(PK_NE + 1); }
            else { x3[0] = ipv(32); x3[1] = ipv(33); x3[2] = ipv(34); }
            int offset = 0;
            if (x3[2] - x3[0] > 0.7f * (x3[1] - x3[0])) offset = 1;
            else if (x3[0] - x3[2] > 0.7f * (x3[1] - x3[2])) offset = -1;
            pg = fminf(pg, gg);
            int res = 2 * t + offset;
            if (res < PITCH_MIN) res = PITCH_MIN;
            NNN_TIF(b, pitch, 1, f, tile, sl)[0] = res;
            NNN_TIF(b, pgain, 1, f, tile, sl)[0] = pg;
            last_period = res;
            last_gain = pg;
            if (chain) {
                __threadfence();   // every stream's pitch and gain before the flag
                if (lane0 == 0 && seq0 + f != b.dbg_withhold) flag_publish((int *)NNN_TIF(b, pflag, 1, f, tile, q0), seq0 + f);
            }
        }
        NNN_STAMP(b, 57);
        // (the next frame's first writes to anything this frame still reads sit behind barriers wave 0 takes part in)
    }
    if (dec_lane && f_end == g) {
        NNN_TI(b.last_period, 1, tile, q0 + s)[0] = last_period;
        NNN_TI(b.last_gain, 1, tile, q0 + s)[0] = last_gain;
    }
}

}  // namespace nnn
