// nnn_kernels.hip -- CDNA4 (gfx950) kernels for the batched nnnoiseless process_frame path.
//
// Compiled with -ffp-contract=off: everything upstream of the integer pitch index must round
// exactly like the scalar reference (which never fuses a*b+c); fmaf() is written explicitly
// where fusing is allowed (FFT, RNN mat-vecs, band sums: tolerance-only quantities).
//
// Mapping rule: a stage whose result feeds the pitch index runs lane = stream on
// the tile-interleaved (TI) layout, so every lane executes the reference's scalar recurrence in the
// reference's summation order at full lane utilisation, with extra parallelism (lag chunks, sample
// chunks, neuron blocks) spread over waves.  Stages with data-dependent addressing or a 960-point
// transform run wave = stream on the stream-major (SM) layout with the stream's data staged in LDS.
//
// Reference citations are into jneem/nnnoiseless v0.5.1.
//
// One file per stage, in pipeline order; definitions keep that order in every unit that includes this file.  nnn_hp.hip is also compiled on
// its own (see the note at k_hp2).
#pragma once
#include "nnn_common.hip"
#include "nnn_hp.hip"
#include "nnn_lpc.hip"
#include "nnn_pitch.hip"
#include "nnn_fft.hip"
#include "nnn_features.hip"
#include "nnn_rnn.hip"
#include "nnn_rnn_wf.hip"
#include "nnn_vad.hip"
#include "nnn_net.hip"
#include "nnn_synth.hip"
#include "nnn_split.hip"

namespace nnn {

// the activation functions on their own, for the direct known-answer sweep of the parity tests (ref: src/util.rs:29-53)
__global__ void k_activation_kat(const float *tansig, const float *x, float *y, int act, int n)
{
    __shared__ float tab[201];
    for (int i = threadIdx.x; i < 201; i += blockDim.x) tab[i] = tansig[i];
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = activate(act, x[i], tab);
}

// Per-frame launch parameters of a call (one thread per frame): entry t describes frame t of the call (v = frame 0).
__global__ void k_fill_params(StepParams *tab, StepParams v, int n, int nslot)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    tab[t] = step_params_at(v, t, nslot);
}

}  // namespace nnn
