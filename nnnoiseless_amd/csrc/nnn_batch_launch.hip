// nnn_batch_launch.hip -- a device call: the three plan functions (plan_group, plan_call, plan_schedule), the launch switch
// (launch_stage) and process_frames, which enqueues the planned stream and event graph; the two *_device entry points.
// Needs nnn_batch_core.hip (Paths, GroupPlan, struct nnn_batch, grow, report_fault) and call_begin / call_end of nnn_batch_streams.hip.
#pragma once

// ---- one group of frames ------------------------------------------------------------------------
struct Launcher {
    nnn_batch *h;
    hipStream_t st;
    bool prof;
    template <class K, class... A> void go(int id, K kern, dim3 grid, dim3 block, size_t lds, A... args)
    {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (prof) {
            hipEventCreate(&e0);
            hipEventCreate(&e1);
            hipEventRecord(e0, st);
        }
        hipLaunchKernelGGL(kern, grid, block, lds, st, args...);
        if (prof) {
            hipEventRecord(e1, st);
            h->evp.push_back(e0);
            h->evp.push_back(e1);
            h->evp_kernel.push_back(id);
        }
    }
};

// Per-group DAG: hp -> pitch -> fft_xp -> rnn -> synth.  Four stages carry state from group to group -- the
// biquad (hp), the last pitch (pitch), GRU / cepstral / last-gain state (rnn), the overlap memory (synth).

// The LPC analysis of a group's frames as a launch of its own behind the high-pass (lane = stream, frames side by side): launches too
// small to fill the GPU spread the five lags of a stream over five waves (k_lpc_wide); k_lpc takes as many frames per wave as still
// leave two waves per SIMD (the frames per wave; 0 = k_lpc_wide).  The denoiser (plan_group) and the training rows launch it so.
static int lpc_launch(const nnn_batch *h, int g)
{
    const Paths &p = h->paths;
    const unsigned NT = (unsigned)h->NT, ug = (unsigned)g;
    if (p.lpc_wide >= 0 ? p.lpc_wide != 0 : NT * ug < 512u) return 0;
    int fc = LPC_FC;
    while (fc > 1 && NT * ((ug + fc - 1) / fc) < 2048u) fc /= 2;
    if (p.lpc_fc > 0) fc = p.lpc_fc < LPC_FC ? p.lpc_fc : LPC_FC;
    return fc;
}
// k_pitch's frames side by side, chained through flags, while one frame's workgroups cannot fill the GPU (below 16384 streams; measured
// at 4096: 46.8 -> 32.8 us per frame; at 65536, where the frame loop's prefetch of the next window matters instead: 468 -> 515)
static bool pitch_chained(const nnn_batch *h, int g)
{
    const int pc = h->paths.pitch_chain;
    return pc > 0 && g > 1 && (pc > 1 || (unsigned)h->S_pad / PK_SPB < 1024u);
}

// Everything a group of g frames runs, into p.  Reads the batch only.
static void plan_group(const nnn_batch *h, int g, GroupPlan &p)
{
    const Paths &k = h->paths;
    p.g = g;
    // The back end.  One-frame groups by default: there the unfused chain's three launches and the round trip of the spectra through
    // HBM buy nothing -- the layer-pipelined RNN has no second frame to pipeline.  Measured on one MI355X
    // (scripts/back_ab.py, profiles/r4_back_ab.txt), one frame per call: fused 143 us against 162 (unfused) and 148 (RNN stretch alone)
    // at 4096 streams, level with the RNN stretch alone at 8192, behind it from 16 384 streams up (a block of sixteen waves that holds a
    // compute unit through three stretches fills the GPU worse than three launches of small blocks once there are several rounds of
    // them); 24-frame groups: the layer-pipelined RNN between k_fft_xp and k_synth stays ahead of both (65.5 against 59.7 M frames/s at
    // 65 536 streams).
    const int m = k.back_mode >= 0 ? k.back_mode : g > 1 ? 0 : ((h->S_pad <= 8192 && !h->beside_others) ? 1 : 3);
    const bool fused = m == 1 || m == 2, all_g = m == 2 || m == 4;
    p.back = m == 0 || (g > 1 && !all_g) ? BACK_UNFUSED : (fused ? BACK_FUSED : BACK_RNN_ALONE);
    for (const nnn_batch::ModelGroup &G : h->groups)
        if ((fused ? G.back_lds : G.rnn16_lds) == 0) p.back = BACK_UNFUSED;   // (a model outside the kernel's shape class)
    // k_hp on two waves per tile (recurrence | everything else, k_hp2): for launches that leave SIMDs empty; groups: two tiles per block
    const bool split = k.hp_split >= 0 ? k.hp_split != 0 : h->NT <= 256;
    p.hp = !split ? 0 : ((k.hp_tpb ? k.hp_tpb == 2 : (g > 1 && h->NT >= 8)) ? 2 : 1);
    p.floor = h->n_floored > 0;   // (nnn_batch_set_gain_floor; the host's count is as the device's rows will be when the launch runs, like the mask's)
    p.link = h->link_ch > 1;   // (nnn_batch_set_channel_link: the argument blocks carry the setting, Buffers::link)
    p.held = h->n_held > 0;   // (the host's copy of the mask is as the device's will be when the launch runs: hold and resume are enqueued in call order)
    // One-frame groups of batches whose pitch launch is a single round of workgroups (two 8-wave blocks per compute unit) run the LPC
    // analysis inside k_pitch: one launch fewer on the critical path of a real-time tick (measured per one-frame call: -6 us at 4096
    // streams, level at 8192, +9 us at 16 384).  With k_hp2, the part of its sums that needs none of the new frame rides in the
    // high-pass launch (the head: another -5 us at 4096, -6 at 8192, still +10 at 16 384).
    p.lpc_in_pitch = g == 1 && h->S_pad <= (split ? 8192 : 6144) && k.lpc_wide < 0 && k.lpc_fc == 0;
    p.head = p.lpc_in_pitch && split && k.lpc_head != 0;
    p.lpc_fc = p.lpc_in_pitch ? 0 : lpc_launch(h, g);
    p.chain = pitch_chained(h, g);
    // one-frame groups through the fused back end on small batches: its X transform rides in k_pitch's launch
    p.riders = g == 1 && p.back == BACK_FUSED && (k.x_rides >= 0 ? k.x_rides != 0 : h->S_pad <= 8192);
    // The RNN kernel of each resident model.  The layer-pipelined kernel spends g + 4 ticks on g frames: for a lone frame on a batch of
    // many block rounds the plain kernel's eleven phases are shorter (one frame per call at 16 384 / 32 768 / 65 536 streams: +6 / +7 /
    // +7 %; at 4096 streams, one round of blocks, the pipelined kernel stays 8 % ahead).  Same bits either way.
    // ... and with other batches ticking beside this one (g_call_mark) the lone frame's kernel is chosen for their sake too (k_rnn_wf holds
    // every compute unit for its five ticks: eight 4096-stream batches ticking side by side 40.2 -> 43.4 M frames/s with k_rnn, a lone batch -8 %)
    for (size_t i = 0; i < h->groups.size(); i++) {
        const nnn_batch::ModelGroup &G = h->groups[i];
        const int min_g = k.wf_min_g > 0 ? k.wf_min_g : ((G.ntiles * (TILE / WF_ROWS) >= 1024 || h->beside_others) ? 2 : 1);
        p.rnn[i] = p.back == BACK_RNN_ALONE ? RK_BACK : !(G.wf && g >= min_g) ? RK_PLAIN : G.shape_builtin ? RK_WF_BUILTIN : RK_WF_ANY;
    }
}

// The kernels launched with more dynamic LDS than a function may have by default -- every k_rnn, k_rnn_wf and k_back instantiation, k_vad, k_net.
// launch_stage takes them from these tables and nowhere else, and creation raises the limit of every kernel in them to the hardware's
// 160 KB (raise_lds_limits): an instantiation cannot be launched without having had its limit raised.
using RnnWfKernel = decltype(&k_rnn_wf<WfShapeAny>);
using BackKernel = decltype(&k_back<true, BkShapeBuiltin>);
using RnnPlainKernel = decltype(&k_rnn<false>);
static const RnnPlainKernel kRnnKernels[2] = {k_rnn<false>, k_rnn<true>};   // [channels linked]
static const auto kVadKernel = &k_vad;
static const auto kNetKernel = &k_net;   // (launched by nnn_batch_network_device, nnn_batch_network.hip)
static const RnnWfKernel kRnnWfKernels[2] = {k_rnn_wf<WfShapeAny>, k_rnn_wf<BkShapeBuiltin>};   // [the model is of the built-in shape class]
#define NNN_BK(F, XR, HELD, FLOOR) {k_back<F, BkShapeBuiltin, XR, HELD, FLOOR, false>, k_back<F, BkShapeBuiltin, XR, HELD, FLOOR, true>}
static const BackKernel kBackFused[2][2][2][2] = {   // [X rides in k_pitch][some stream held][some stream floored][channels linked]
    {{NNN_BK(true, false, false, false), NNN_BK(true, false, false, true)}, {NNN_BK(true, false, true, false), NNN_BK(true, false, true, true)}},
    {{NNN_BK(true, true, false, false), NNN_BK(true, true, false, true)}, {NNN_BK(true, true, true, false), NNN_BK(true, true, true, true)}}};
static const BackKernel kBackRnnAlone[2][2][2] = {   // [some stream held][some stream floored][channels linked]
    {NNN_BK(false, false, false, false), NNN_BK(false, false, false, true)},
    {NNN_BK(false, false, true, false), NNN_BK(false, false, true, true)}};
#undef NNN_BK
static std::vector<const void *> big_lds_kernels()
{
    std::vector<const void *> v;
    for (RnnPlainKernel k : kRnnKernels) v.push_back((const void *)k);
    for (RnnWfKernel k : kRnnWfKernels) v.push_back((const void *)k);
    for (const auto &by_held : kBackFused)
        for (const auto &by_floor : by_held)
            for (const auto &by_link : by_floor)
                for (BackKernel k : by_link) v.push_back((const void *)k);
    for (const auto &by_floor : kBackRnnAlone)
        for (const auto &by_link : by_floor)
            for (BackKernel k : by_link) v.push_back((const void *)k);
    v.push_back((const void *)kVadKernel);
    v.push_back((const void *)kNetKernel);
    return v;
}

// stage `s` of the group planned in p, in scratch sets set0 .. set0 + p.g - 1, parameters at sp0[0..g), on stream `st`.
// plain_out: the parameter table sp0 points into was filled for f32 mono audio (k_synth's plain-format instantiation ignores the table's
// fmt / channels, so the caller states the format of the very call that fills the table, not a field of the batch)
static void launch_stage(nnn_batch *h, int s, int set0, const GroupPlan &p, const StepParams *sp0, hipStream_t st, bool prof, bool plain_out, const StepParams *call = nullptr, int fill = 0,
                         const SplitIo *io = nullptr)
{
    const int g = p.g;
    if (g <= 0) return;   // (never a launch with an empty grid)
    const unsigned NT = (unsigned)h->NT, Sp = (unsigned)h->S_pad, ug = (unsigned)g;
    const Buffers &b = h->b[set0];
    Launcher L{h, st, prof};
    switch (s) {
    case ST_HP:
        // (`fill`: this is the first launch of a call whose parameter table is k_hp's to fill, see k_hp)
        if (p.hp == 2)
            L.go(K_HP, p.held ? k_hp2<2, true> : k_hp2<2, false>, dim3((NT + 1) / 2 + (p.head ? (5 * NT + 3) / 4 : 0)), dim3(256), 0, b, sp0, g, call ? *call : StepParams{}, call ? fill : 0, p.head ? 1 : 0);
        else if (p.hp == 1)
            L.go(K_HP, p.held ? k_hp2<1, true> : k_hp2<1, false>, dim3(NT + (p.head ? (5 * NT + 1) / 2 : 0)), dim3(128), 0, b, sp0, g, call ? *call : StepParams{}, call ? fill : 0, p.head ? 1 : 0);
        else L.go(K_HP, p.held ? k_hp<true> : k_hp<false>, dim3(NT), dim3(64), 0, b, sp0, g, call ? *call : StepParams{}, call ? fill : 0);
        if (p.lpc_in_pitch) break;   // (k_pitch does it on its way, see there)
        if (!p.lpc_fc) L.go(K_LPC, k_lpc_wide, dim3(NT * ug), dim3(320), 0, b, sp0, g);
        else L.go(K_LPC, k_lpc, dim3(NT * ((ug + p.lpc_fc - 1) / p.lpc_fc)), dim3(64), 0, b, sp0, g, p.lpc_fc);
        break;
    case ST_PITCH: {
        // (flag values are frame numbers (> 0))
        const int chain = p.chain ? 1 : 0, seq0 = (int)(h->frame_count & 0x3fffffffu) + 1;
        const unsigned grid = Sp / PK_SPB * (chain ? ug : 1u);
        if (p.lpc_in_pitch)
            L.go(K_PITCH, p.held ? k_pitch<true, true> : k_pitch<true, false>, dim3(grid + (p.riders ? Sp / 8 : 0u)), dim3(PK_T), 0, b, sp0, g, chain, seq0, h->tickets, p.head ? 2 : 1, p.riders ? (int)grid : 0);
        else
            L.go(K_PITCH, p.held ? k_pitch<false, true> : k_pitch<false, false>, dim3(grid + (p.riders ? Sp / 8 : 0u)), dim3(PK_T), 0, b, sp0, g, chain, seq0, h->tickets, 0, p.riders ? (int)grid : 0);
        if (chain) h->tickets += grid;   // (launches of one batch's pitch stage are ordered among themselves: a stateful stage)
        break;
    }
    case ST_FFT:
        if (p.back == BACK_FUSED) {   // the fused back end takes the place of this stage and the two behind it: one launch per resident model
            for (const nnn_batch::ModelGroup &G : h->groups)   // (riders: its X transform done by k_pitch's rider blocks, see xt_rider)
                L.go(K_BACK, kBackFused[p.riders][p.held][p.floor][p.link], dim3((unsigned)(G.ntiles * (TILE / BK_ROWS))), dim3(BK_T), G.back_lds, b, sp0, G.acts, G.wq, G.fpar, G.tile0, g);
            break;
        }
        L.go(K_FFT_XP, k_fft_xp, dim3(Sp * ug / FFT_SPB), dim3(64 * FFT_SPB), 0, b, sp0, g);
        break;
    case ST_RNN:
        if (p.back == BACK_FUSED) break;
        for (size_t i = 0; i < h->groups.size(); i++) {   // one launch per resident model (a run of whole tiles)
            const nnn_batch::ModelGroup &G = h->groups[i];
            if (p.rnn[i] == RK_BACK)
                L.go(K_RNN, kBackRnnAlone[p.held][p.floor][p.link], dim3((unsigned)(G.ntiles * (TILE / BK_ROWS))), dim3(BK_T), G.rnn16_lds, b, sp0, G.acts, G.wq, G.fpar, G.tile0, g);
            else if (p.rnn[i] == RK_WF_BUILTIN || p.rnn[i] == RK_WF_ANY)
                L.go(K_RNN, kRnnWfKernels[p.rnn[i] == RK_WF_BUILTIN], dim3((unsigned)(G.ntiles * (TILE / WF_ROWS))), dim3(64 * WF_WAVES), G.wf_lds, b, G.plan, G.wp,
                     G.wq, G.fpar, G.tile0, g);
            else
                L.go(K_RNN, kRnnKernels[p.link], dim3((unsigned)(G.ntiles * (TILE / G.rows))), dim3(64 * RNN_WAVES), G.rnn_lds, b, G.plan, G.wq, G.fpar,
                     G.tile0, G.rows, g);
        }
        break;
    case ST_SYN:
        if (p.back == BACK_FUSED) break;
        if (plain_out) L.go(K_SYNTH, k_synth<true>, dim3(Sp / FFT_SPB), dim3(64 * FFT_SPB), 0, b, sp0, g);
        else L.go(K_SYNTH, k_synth<false>, dim3(Sp / FFT_SPB), dim3(64 * FFT_SPB), 0, b, sp0, g);
        break;
    // the split calls' boundary launches (io: the caller's rows).  Not in the timing table: untimed, like the training rows' k_features.
    case ST_FEAT:
        hipLaunchKernelGGL(k_features, dim3(NT), dim3(64 * FEAT_WAVES), 0, st, b, g);
        hipLaunchKernelGGL(k_features_out, dim3(NT * ug), dim3(FOUT_T), 0, st, b, io->features, io->silence, g);
        break;
    case ST_GAINS:
        hipLaunchKernelGGL(k_gains_in, dim3(NT), dim3(GIN_T), 0, st, b, io->gains, io->vad, g);
        break;
    // the VAD calls' launches, untimed like the split calls' (the caller's VAD rows travel in the parameter table, as a processing call's do)
    case ST_FFT_FEAT:
        if (b.taps) hipLaunchKernelGGL(k_fft_xp, dim3(Sp * ug / FFT_SPB), dim3(64 * FFT_SPB), 0, st, b, sp0, g);   // (so that the X and P taps exist)
        else hipLaunchKernelGGL(k_fft_feat, dim3(Sp * ug / FFT_SPB), dim3(64 * FFT_SPB), 0, st, b, sp0, g);
        break;
    case ST_VAD:
        hipLaunchKernelGGL(k_features, dim3(NT), dim3(64 * FEAT_WAVES), 0, st, b, g);
        for (const nnn_batch::ModelGroup &G : h->groups)   // one launch per resident model, as the RNN's
            hipLaunchKernelGGL(kVadKernel, dim3((unsigned)(G.ntiles * (TILE / G.vad_rows))), dim3(64 * RNN_WAVES), G.vad_lds, st, b, sp0, G.plan, G.wq,
                               G.fpar, G.tile0, G.vad_rows, G.vad_mb, g);
        break;
    }
}

static int drain_profile(nnn_batch *h)
{
    for (size_t i = 0; i < h->evp_kernel.size(); i++) {
        float ms = 0.0f;
        HIPCHK(hipEventSynchronize(h->evp[2 * i + 1]));
        HIPCHK(hipEventElapsedTime(&ms, h->evp[2 * i], h->evp[2 * i + 1]));
        h->k_ms[h->evp_kernel[i]] += ms;
        h->k_launches[h->evp_kernel[i]] += 1;
        hipEventDestroy(h->evp[2 * i]);
        hipEventDestroy(h->evp[2 * i + 1]);
    }
    h->evp.clear();
    h->evp_kernel.clear();
    return 0;
}

struct CallPlan {             // what a call decides before it launches anything (plan_call, which reads the batch only)
    std::vector<int> sizes;   // frames of each group
    bool pipe;                // spread over the internal streams (otherwise the groups' stages back to back on the caller's stream)
    int sched, lanes;         // the schedule of a pipelined call
    bool fold_fill, early_hp, hp_after;   // see plan_call
    bool idle;                // every stream is held (nnn_batch_hold_streams): the call moves the frame counter and launches nothing
};
static CallPlan plan_call(const nnn_batch *h, int n_frames, hipStream_t st)
{
    const Paths &k = h->paths;
    CallPlan c;
    // group sizes.  A pipelined call (32 frames or more) is cut into an even number of near-equal groups of at most GROUP frames --
    // its groups alternate between two lanes, so an odd count leaves one lane a group short (three groups of 16 for the bench's
    // 48-frame call: 55.5 M frames/s at 4096 streams; two of 24: 57.2 M) -- everything else into full groups of GROUP frames, the
    // remainder last (round 2a's smaller groups at the ends of a pipelined call measured 6 % slower).
    constexpr int PIPE_MIN = 32;
    // (from 16 384 streams up every kernel fills the GPU on its own and a launch beside it only costs it cache: one stream, in order,
    // unless a schedule was asked for -- 32 768 streams: 65.9 M frames/s against 64.8 with the high-pass on a stream of its own)
    // (the automatic schedule pipelines up to 16 384 streams: measured in round 4 with the high-pass held back behind the previous group's
    // pitch kernel, see hp_after -- 16 384: 64.2-65.5 -> 66.4-66.9 M frames/s; 32 768 and 65 536 lose 1-2 % pipelined)
    // Round 6: above 16 384 streams the automatic schedule overlaps kernels again.  k_pitch issues a fifth fewer instructions than in round 5 and
    // waits more (certified search), and every kernel of a big batch ends in a tail of half-empty compute units -- twelve tails per 48-frame
    // call; with two groups in flight another stage's blocks fill them.  Measured on one box, interleaved (scripts/gpu_sched_r6.sh,
    // profiles/r6_sched_sweep.txt), against one stream in order: 65 536 x 48 stages +2.6 % (lanes 2: +1.0), 65 536 x 96 lanes 2 +2.3 % (stages
    // -0.3), 32 768 x 96 lanes 2 +1.9 % (stages +0.4), 32 768 x 48 stages +1.0 % (lanes 2: -0.4): one stream per stage for calls of two
    // groups, two lanes for longer ones.  Costs the second block of scratch sets and the longer ring (650 against 360 KB per stream).
    const bool auto_big = k.sched_auto && h->S_pad > AUTO_BIG;
    c.idle = h->n_held == h->S;
    c.pipe = !c.idle && k.use_pipeline && k.sched != SCHED_SEQ && !h->profiling && n_frames >= PIPE_MIN && !(auto_big && h->depth < 2);
    if (c.pipe) {
        int n = 2;
        while ((n_frames + n - 1) / n > h->gmax) n += 2;
        // (a batch sized for one-frame groups and an odd frame count: the even count overshoots the frames -- never an empty group)
        if (n > n_frames) n = n_frames;
        for (int i = 0; i < n; i++) c.sizes.push_back(n_frames / n + (i < n_frames % n ? 1 : 0));
    } else {
        for (int rem = n_frames; rem > 0; rem -= c.sizes.back()) c.sizes.push_back(rem < h->gmax ? rem : h->gmax);
    }
    c.sched = auto_big ? (c.sizes.size() <= 2 ? SCHED_STAGES : SCHED_LANES) : k.sched;
    c.lanes = auto_big ? 2 : k.n_lanes;
    // the per-frame parameter table: a launch of its own ahead of a pipelined call's streams; otherwise the call's first kernel (k_hp of
    // the first group) fills it on its way (a one-frame call is a handful of launches of 15-35 us: one fewer is 4 % of it)
    c.fold_fill = (!c.pipe && !h->profiling) || c.idle;   // (idle: no table at all)
    // The next call's high-pass chain may start before this stream has seen the previous call drain, when the caller has
    // promised that inputs are final at call time (nnn_batch_set_inputs_ready): it depends on the previous call only through
    // its own stream (biquad state) and the history-ring slots it overwrites (synthesis events of the groups that read them).
    // (never for the library's own host-buffer calls: their input is an upload enqueued just before on the caller's stream or on
    // a copy stream, final only in that stream's order -- the promise is about buffers the CALLER filled)
    c.early_hp = c.pipe && k.inputs_ready && !h->host_call && h->prev_pipe && h->prev_st == st && c.sched == SCHED_LANES && h->pool[0];
    // The high-pass of group k may start as soon as the ring slots it overwrites are free -- with the pitch kernel of group k - 1, and the
    // two slow each other (10.8 in HISTORY.md).  From 8192 streams up a group is long enough for the chain to wait until that pitch
    // kernel is done and still finish before group k needs it: 8192 x 48: 61.3 -> 63.9 M frames/s, 16 384: +2-3 %; at 4096 streams the
    // window is too short (57.5 -> 56.3).
    c.hp_after = c.sched == SCHED_LANES && c.lanes == 1 && h->S_pad >= 8192;
    return c;
}

// A call's launches in the order they are enqueued, with the stream each goes on and the events it waits for and records
// (plan_schedule, which reads the batch only; process_frames enqueues it, nnn_batch_debug_schedule shows it to the tests)
constexpr int MAX_WAITS = 1 + 1 + 1;   // the most a node has, pitch: the high-pass of its group, the pitch of the group before, the scratch-set block's previous user
static_assert(MAX_WAITS >= 1 + 1, "hp: the pitch kernel before it (hp_after) and the ring edge; rnn, synth: previous stage and previous group; fft_xp: previous stage");
enum WaitOrigin { W_THIS = 0, W_PREV = 1, W_DONE = 2 };   // ev[this call's parity], ev[prev_par], ev_done[this call's parity] (= of the call two back)
enum FillWhere { FILL_FOLDED = 0, FILL_CALLER = 1, FILL_POOL0 = 2 };   // k_fill_params: no launch (k_hp does it, or an idle call), caller's stream, pool[0]
struct Wait { int origin, stage, group; };   // the event's slot is group % EVR (W_DONE: no stage or group)
struct Node {
    int stage, group, frames, first;   // frames of the group, its first frame within the call
    int stream;                        // index into nnn_batch::pool, -1 = the caller's stream
    bool first_use;                    // the stream's first launch of the call: waits for ev_in (everything before the call)
    bool record;                       // records ev[parity][stage][group % EVR]: it has a consumer on another stream
    bool fill;                         // the launch that fills the parameter table on its way (FILL_FOLDED)
    int n_waits;
    Wait waits[MAX_WAITS];
};
struct Schedule {
    std::vector<Node> nodes;
    int fill = FILL_FOLDED;
    bool fill_after_done = false;      // FILL_POOL0: behind ev_done[parity], the table's previous user
    int last_syn = -1;                 // the group whose synthesis event the caller's stream waits for at the end (-1: it ran there)
};

// A call is cut into groups of up to GROUP frames; group k uses scratch-set block (group_count mod depth).  Short calls
// (and profiling) run the groups' stages back to back on the caller's stream.  Longer calls spread over the batch's
// internal streams so that independent stages overlap (at 4096 streams a lone stage cannot fill the GPU):
//   lanes   the high-pass chain on its own stream, running ahead as far as the history rings allow; stages pitch .. synth of
//           group k on lane stream k mod n_lanes
//   stages  one stream per stage: hp | pitch | fft_xp | rnn | synth; every stream is a chain of groups
// An edge of the DAG whose ends share a stream needs nothing (streams are in-order); the others are an event record + wait.
// Edges: previous stage of the same group; the same stage of the previous group for the four stateful stages; the scratch-set
// block's previous user (synth of group k - depth, before pitch of group k); the history rings (synth of the group holding the
// newest frame whose history slots group k's high-pass overwrites).  Everything before this call is ordered by the caller's
// stream, which every internal stream waits for at its first use and which waits for the last synth at the end.
// The schedule of the batch's NEXT call (parity of call_count + 1), cut and set as `cp` says.
static Schedule plan_schedule(const nnn_batch *h, const CallPlan &cp)
{
    Schedule sc;
    const int n_groups = (int)cp.sizes.size(), par = (int)((h->call_count + 1) & 1);
    sc.fill = cp.early_hp ? FILL_POOL0 : (cp.fold_fill ? FILL_FOLDED : FILL_CALLER);
    sc.fill_after_done = cp.early_hp && h->have_done[par];   // the table's previous user (two calls back)
    if (cp.idle) return sc;
    // index into h->pool; -1 = the caller's stream (lane 0 of the lanes schedule, the synthesis chain of the stages one, every launch of a
    // call that is not pipelined)
    auto stream_of = [&](int s, int k) -> int {
        if (!cp.pipe) return -1;
        if (cp.sched == SCHED_STAGES) return s == ST_HP ? 0 : (s == ST_PITCH ? 1 : (s == ST_FFT ? 2 : (s == ST_RNN ? 3 : -1)));
        return s == ST_HP ? 0 : (k % cp.lanes) - (k % cp.lanes == 0 ? 1 : 0);
    };
    // which (stage, group) nodes have a consumer on another stream: only those record an event
    auto consumers_elsewhere = [&](int s, int k) {
        const int me = stream_of(s, k);
        if (s + 1 < ST_COUNT && stream_of(s + 1, k) != me) return true;
        if ((s == ST_HP || s == ST_PITCH || s == ST_RNN || s == ST_SYN) && k + 1 < n_groups && stream_of(s, k + 1) != me) return true;
        if (s == ST_SYN) return true;   // scratch-set / ring edges and the end of the call
        if (cp.hp_after && s == ST_PITCH) return true;
        return false;
    };
    bool used[NSTREAMS] = {cp.early_hp};   // (pool[0] of an early_hp call starts with the table's fill: no wait for the caller's stream on that one)
    const int pn = (int)h->prev_first.size();   // groups of the previous call
    sc.nodes.reserve((size_t)n_groups * ST_COUNT);
    for (int k = 0, t = 0; k < n_groups; t += cp.sizes[k++]) {
        const int g = cp.sizes[k];
        for (int s = 0; s < ST_COUNT; s++) {
            Node n = {};
            const int si = stream_of(s, k);
            n.stage = s, n.group = k, n.frames = g, n.first = t, n.stream = si;
            n.first_use = si >= 0 && !used[si];   // everything before the call comes first
            if (si >= 0) used[si] = true;
            n.fill = cp.fold_fill && k == 0 && s == ST_HP;
            n.record = cp.pipe && consumers_elsewhere(s, k);
            auto wait = [&](int origin, int ds, int dk) { n.waits[n.n_waits++] = Wait{origin, ds, dk}; };
            auto wait_for = [&](int ds, int dk) {
                if (dk < 0 || dk < k - EVR + 1) return;   // before this call (ordered by ev_in) or long retired
                if (stream_of(ds, dk) != si) wait(W_THIS, ds, dk);
            };
            if (s > 0) wait_for(s - 1, k);
            if (s == ST_HP || s == ST_PITCH || s == ST_RNN || s == ST_SYN) wait_for(s, k - 1);
            if (s == ST_PITCH) wait_for(ST_SYN, k - h->depth);
            if (s == ST_HP && cp.hp_after) {   // behind the previous group's pitch kernel (the previous call's last one for the first group)
                if (k > 0) wait_for(ST_PITCH, k - 1);
                else if (cp.early_hp && pn > 0) wait(W_PREV, ST_PITCH, pn - 1);
            }
            if (s == ST_HP && cp.pipe) {
                // slots written now held frames (newest of this group) - nslot and older; their last readers are the
                // frames up to 3 later
                const int need = t + g - 1 + 3 - h->nslot;
                int dk = -1;   // the group of this call that holds frame `need` (none: it precedes the call)
                for (int j = 0; j < k; j++)
                    if (sc.nodes[(size_t)j * ST_COUNT].first <= need) dk = j;
                wait_for(ST_SYN, dk);
                if (cp.early_hp && need < 0) {
                    // the frame lies in the previous call: the synthesis of its group there; older still: the call before that
                    const long long pf = (long long)h->frame_count + need - (long long)h->prev_frame0;
                    int pj = -1;
                    for (int j = 0; j < pn; j++)
                        if (h->prev_first[j] <= pf) pj = j;
                    if (pf >= 0 && pj >= 0 && pn - pj < EVR) wait(W_PREV, ST_SYN, pj);
                    else if (h->have_done[par]) wait(W_DONE, 0, 0);   // (this parity's last call = the one before the previous one)
                }
            }
            sc.nodes.push_back(n);
        }
    }
    if (stream_of(ST_SYN, n_groups - 1) >= 0) sc.last_syn = n_groups - 1;
    return sc;
}
static hipEvent_t wait_event(const nnn_batch *h, int par, const Wait &w)
{
    return w.origin == W_DONE ? h->ev_done[par] : h->ev[w.origin == W_PREV ? h->prev_par : par][w.stage][w.group % EVR];
}

// Common body of the process entry points: strides in BYTES, `drop` leading frames of the call produce no audio.
static int process_frames(nnn_batch *h, const void *d_in, void *d_out, float *d_vad, int n_frames, int fmt, int channels,
                          long long group_stride, long long frame_stride, int drop, void *hip_stream)
{
    HIPCHK(hipSetDevice(h->device));
    if (int rc = report_fault(h)) return rc;   // an earlier call's hand-off failure (seen as soon as the device has written it)
    const bool plain_out = fmt == PCM_F32 && channels == 1;
    {
        const uint64_t mask = (1ull << 44) - 1;
        const uint64_t now = (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now().time_since_epoch()).count() & mask;
        const uint64_t prev = g_call_mark[h->device].exchange((h->id << 44) | now, std::memory_order_relaxed);
        if ((prev >> 44) != h->id && (prev >> 44) != 0 && now - (prev & mask) < 5000) h->other_seen_us = now | (1ull << 63);
        h->beside_others = (h->other_seen_us >> 63) && now - (h->other_seen_us & mask) < 20000;
        if (h->beside_others) {   // once per process: the host's queue setting decides whether batches side by side overlap at all
            static std::atomic<bool> told{false};
            if (!getenv("GPU_MAX_HW_QUEUES") && !told.exchange(true))
                fprintf(stderr, "nnnoiseless_mi355x: several batches are being driven side by side on device %d and GPU_MAX_HW_QUEUES is not set; "
                                "the HIP runtime then maps their streams onto 4 hardware queues and they largely serialise "
                                "(export GPU_MAX_HW_QUEUES=8 before the process starts -- INTEGRATION.md; any value of the variable silences this note)\n", h->device);
        }
    }
    hipError_t e;
    hipStream_t st = call_begin(h, hip_stream, e);
    if (e != hipSuccess) return fail("hipStreamWaitEvent(st, h->ev_last, 0) failed: %s", hipGetErrorString(e));
    StepParams v0;
    v0.in = (const char *)d_in;
    v0.out = (char *)d_out;
    v0.vad = d_vad;
    v0.group_stride = group_stride;
    v0.frame_stride = frame_stride;
    v0.fmt = fmt;
    v0.channels = channels;
    v0.discard = drop;
    v0.slot = (int)(h->frame_count % h->nslot);
    v0.n_streams = h->S;
    v0.log = h->frame_log_left ? h->frame_log : nullptr;
    v0.log_frames = (int)(h->frame_log_left < (size_t)n_frames ? h->frame_log_left : (size_t)n_frames);
    if (v0.log) {
        h->frame_log += (size_t)v0.log_frames * h->S * FRAME_LOG_WORDS;
        h->frame_log_left -= (size_t)v0.log_frames;
    }
    if ((size_t)n_frames > h->sp_tab.cap) {
        const size_t cap = n_frames < 64 ? 64 : (size_t)n_frames;
        if (int rc = grow(h, true, h->sp_tab, 2 * cap * sizeof(StepParams), cap)) return rc;
        h->prev_pipe = false;
    }
    const CallPlan cp = plan_call(h, n_frames, st);
    const Schedule sc = plan_schedule(h, cp);
    const int n_groups = (int)cp.sizes.size();
    h->call_count += 1;
    const int par = (int)(h->call_count & 1);
    StepParams *const tab = h->sp_tab.p + (size_t)par * h->sp_tab.cap;   // this call's parameter table
    const uint64_t frame0 = h->frame_count;
    bool ok = true;
    if (sc.fill != FILL_FOLDED) {
        hipStream_t fs = sc.fill == FILL_POOL0 ? h->pool[0] : st;
        if (sc.fill_after_done) ok &= hipStreamWaitEvent(fs, h->ev_done[par], 0) == hipSuccess;
        hipLaunchKernelGGL(k_fill_params, dim3((n_frames + 63) / 64), dim3(64), 0, fs, tab, v0, n_frames, h->nslot);
    }
    if (cp.pipe) ok &= hipEventRecord(h->ev_in, st) == hipSuccess;
    size_t i = 0;
    for (int k = 0; k < n_groups; k++) {   // (an idle call has groups and no nodes)
        const int g = cp.sizes[k], set0 = (int)(h->group_count % h->depth) * h->gmax;
        plan_group(h, g, h->plan);
        for (; i < sc.nodes.size() && sc.nodes[i].group == k; i++) {
            const Node &n = sc.nodes[i];
            if (n.stream >= 0 && !h->pool[n.stream]) ok &= hipStreamCreateWithFlags(&h->pool[n.stream], hipStreamNonBlocking) == hipSuccess;
            hipStream_t ss = n.stream < 0 ? st : h->pool[n.stream];
            if (n.first_use) ok &= hipStreamWaitEvent(ss, h->ev_in, 0) == hipSuccess;
            for (int w = 0; w < n.n_waits; w++) ok &= hipStreamWaitEvent(ss, wait_event(h, par, n.waits[w]), 0) == hipSuccess;
            launch_stage(h, n.stage, set0, h->plan, tab + n.first, ss, h->profiling, plain_out, n.fill ? &v0 : nullptr, n_frames);
            if (n.record) ok &= hipEventRecord(h->ev[par][n.stage][k % EVR], ss) == hipSuccess;
        }
        h->group_count += 1;
        h->frame_count += g;
        h->last_set = set0 + g - 1;
    }
    if (sc.last_syn >= 0) ok &= hipStreamWaitEvent(st, h->ev[par][ST_SYN][sc.last_syn % EVR], 0) == hipSuccess;
    // a pipelined call: the next call's high-pass chain may be started before it has drained (plan_call's early_hp)
    h->prev_pipe = cp.pipe;
    if (cp.pipe) {
        h->prev_st = st;
        h->prev_frame0 = frame0;
        h->prev_par = par;
        h->prev_first.clear();
        for (int k = 0; k < n_groups; k++) h->prev_first.push_back(sc.nodes[(size_t)k * ST_COUNT].first);
    }
    ok &= hipEventRecord(h->ev_done[par], st) == hipSuccess;
    h->have_done[par] = true;
    ok &= call_end(h, st) == hipSuccess;
    if (!ok) return fail("stream/event call failed while enqueueing frames: %s", hipGetErrorString(hipGetLastError()));
    HIPCHK(hipGetLastError());
    if (h->profiling) {
        HIPCHK(hipStreamSynchronize(st));
        return drain_profile(h);
    }
    return 0;
}

static int check_layout(const nnn_batch *h, const nnn_pcm_layout *L)
{
    if (!L) return fail("null layout");
    if (L->format != NNN_PCM_F32 && L->format != NNN_PCM_I16 && L->format != NNN_PCM_F32_UNIT) return fail("unknown sample format %d", L->format);
    if (L->channels < 1 || h->S % L->channels) return fail("n_streams (%d) is not a multiple of channels (%d)", h->S, L->channels);
    if (L->frame_stride < (size_t)FRAME * L->channels) return fail("frame_stride smaller than one frame of all channels");
    return 0;
}

extern "C" int nnn_batch_process_device(nnn_batch *h, const float *d_in, float *d_out, float *d_vad, int n_frames,
                                        size_t stream_stride, size_t frame_stride, void *hip_stream)
{
    if (!h) return fail("null batch");
    if (int rc = refuse_pending(h, "nnn_batch_process_device")) return rc;
    if (n_frames <= 0) return 0;
    if (!d_in || !d_out) return fail("null buffer");
    if (n_frames > 1 && frame_stride < (size_t)FRAME) return fail("frame_stride smaller than one frame");
    return process_frames(h, d_in, d_out, d_vad, n_frames, PCM_F32, 1, (long long)stream_stride * 4, (long long)frame_stride * 4, 0,
                          hip_stream);
}

extern "C" int nnn_batch_process_pcm_device(nnn_batch *h, const void *d_in, void *d_out, float *d_vad, int n_frames,
                                            const nnn_pcm_layout *L, void *hip_stream)
{
    if (!h) return fail("null batch");
    if (int rc = refuse_pending(h, "nnn_batch_process_pcm_device")) return rc;
    if (n_frames <= 0) return 0;
    if (!d_in || !d_out) return fail("null buffer");
    if (int rc = check_layout(h, L)) return rc;
    const long long e = pcm_elem_bytes(L->format);
    const int drop = (L->discard_first && h->frame_count == 0) ? 1 : 0;
    return process_frames(h, d_in, d_out, d_vad, n_frames, L->format, L->channels, (long long)L->group_stride * e,
                          (long long)L->frame_stride * e, drop, hip_stream);
}
