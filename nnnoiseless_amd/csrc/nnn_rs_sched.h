// nnn_rs_sched.h -- what the resampler (nnn_resample.hip) and the rate adapter (nnn_rate.hip) share: the position sequence of the reference's
// Resample loop with the tap weights of dasp_interpolate 0.11.0's Sinc<[f32; 16]> (one schedule entry and sixteen f64 weights per output
// sample, a pure function of the position, idx, credit and the sample count), the bound of its output count, and the fold of one output.
// ref: src/nnnoiseless.rs:106-131 (Resample<RS>); the interpolator is restated from its published source and unpinned (include/nnn_resample.h).
#pragma once

#include <math.h>

constexpr int RS_TAPS = 16, RS_DEPTH = RS_TAPS / 2;

struct RsOut {   // per output sample of a call, shared by all streams
    int consumed;   // source samples of this call pushed before it
    int idx, nd;    // interpolator idx and max_depth at that point
    int pad;
};

struct RsPos {   // the loop's state between calls
    double pos = 0.0;
    int idx = 0;
    long credit = 0;   // source samples already pushed on behalf of the next output (they arrived early)
};

// Upper bound of the output samples n_in more source samples can produce.
static inline long rs_max_output(double ratio, long n_in) { return (long)ceil(((double)n_in + 2.0) / ratio) + 2; }

// The position sequence of Resample::next_sample (src/nnnoiseless.rs:107-120) and the weights of Sinc::interpolate for a call of n_in source
// samples at state `s`: sink(entry, w[16]) once per output the samples complete, at most cap_out of them; `s` becomes the state behind the
// call; returns the count.
template <class Sink> static inline long rs_schedule(double ratio, RsPos &s, long n_in, long cap_out, Sink &&sink)
{
    const double pi = 3.14159265358979323846;
    double pos = s.pos;
    int idx = s.idx;
    long consumed = 0, credit = s.credit, n = 0;
    while (n < cap_out) {
        double p = pos + ratio;
        long need = 0;
        while (p >= 1.0) { p -= 1.0; need++; }
        const long need_now = need - credit;    // `credit` of them went into the ring with an earlier call
        if (consumed + need_now > n_in) break;  // this output waits for the next call's samples
        pos = p;
        consumed += need_now;
        credit = 0;
        for (long k = 0; k < need_now && idx < RS_DEPTH; k++) idx++;   // Sinc::next_source_frame
        const int nl = idx, nr = idx + 1, rightmost = nl + RS_DEPTH, leftmost = nr - RS_DEPTH;
        const int nd = rightmost >= RS_TAPS ? RS_TAPS - RS_DEPTH : (leftmost < 0 ? RS_DEPTH + leftmost : RS_DEPTH);
        const RsOut o{(int)consumed, idx, nd, 0};
        double w[RS_TAPS];
        const double phil = pos, phir = 1.0 - pos;
        for (int k = 0; k < RS_DEPTH; k++) {
            double a = pi * (phil + (double)k);
            double first = a == 0.0 ? 1.0 : sin(a) / a, second = 0.5 + 0.5 * cos(a / (double)RS_DEPTH);
            w[2 * k] = first * second;
            a = pi * (phir + (double)k);
            first = a == 0.0 ? 1.0 : sin(a) / a;
            second = 0.5 + 0.5 * cos(a / (double)RS_DEPTH);
            w[2 * k + 1] = first * second;
        }
        sink(o, (const double *)w);
        n++;
    }
    // Source samples of this call beyond those its completed outputs pulled belong to the next output, whose other samples have
    // not arrived.  The reference pulls a sample only inside the loop of the output that needs it; pushing these now is the same
    // thing (a push only moves the ring, and the ring is looked at when that output is interpolated): they are counted as
    // `credit` against that output's need, and the position keeps its value.
    const long early = n_in - consumed;
    for (long k = 0; k < early && idx < RS_DEPTH; k++) idx++;
    s.credit = credit + early;
    s.pos = pos;
    s.idx = idx;
    return n;
}

// One output sample: the fold of Sinc::interpolate.  `e` points at the ring as it stands (frames[i] = e[i], i < 16, oldest first);
// w[2 n] / w[2 n + 1] = the left / right tap weight of step n (f64), nd = max_depth, idx = the interpolator's idx.  FLAT: the eight steps laid out flat (a caller that holds the weights in registers needs constant
// indices); otherwise the loop as k_resample has always had it.
template <bool FLAT = false> __device__ __forceinline__ float sinc_fold(const float *e, const double *w, int nd, int idx)
{
    float v = 0.0f;
    auto step = [&](int n) {
        v += (float)(w[2 * n] * (double)e[(idx - n) & (RS_TAPS - 1)]);              // frames[nl - n]
        v += (float)(w[2 * n + 1] * (double)e[(idx + 1 + n) & (RS_TAPS - 1)]);    // frames[nr + n] (the ring index wraps)
    };
    if (FLAT) {
#pragma unroll
        for (int n = 0; n < RS_DEPTH; n++)
            if (n < nd) step(n);
    } else {
        for (int n = 0; n < nd; n++) step(n);
    }
    return v;
}
