// nnn_batch_create.hip -- creation (decide, then act: plan_model_group, then one function per step), destruction, the small accessors,
// synchronize and reset.
// Needs nnn_batch_core.hip, hold_release_all of nnn_batch_streams.hip and big_lds_kernels of nnn_batch_launch.hip.
#pragma once

// Tables.  Window and DCT follow the reference exactly (f64 math, f32 storage; src/lib.rs:107-127);
// the tanh table is tanh(0.04 i) to six decimals with upstream's three off-by-one entries
// (src/util.rs:3-27).
static void make_tables(std::vector<float> &window, std::vector<float> &dct, std::vector<float2> &tw,
                        std::vector<float> &tansig, std::vector<float> &bin_frac, std::vector<int> &bin_band, float &wnorm)
{
    const double pi = 3.14159265358979323846;
    window.resize(WINDOW);
    for (int i = 0; i < FRAME; i++) {
        double s = sin(0.5 * pi * ((double)i + 0.5) / (double)FRAME);
        float w = (float)sin(0.5 * pi * s * s);
        window[i] = w;
        window[WINDOW - 1 - i] = w;
    }
    float acc = 0.0f;
    for (int i = 0; i < WINDOW; i++) acc += window[i] * window[i];
    wnorm = 1.0f / acc;
    dct.resize(NB * NB);
    for (int i = 0; i < NB; i++)
        for (int j = 0; j < NB; j++) {
            float v = (float)cos(((double)i + 0.5) * (double)j * pi / (double)NB);
            if (j == 0) v *= sqrtf(0.5f);
            dct[i * NB + j] = v;
        }
    tw.resize(WINDOW);
    for (int k = 0; k < WINDOW; k++) {
        tw[k].x = (float)cos(-2.0 * pi * k / (double)WINDOW);
        tw[k].y = (float)sin(-2.0 * pi * k / (double)WINDOW);
    }
    tansig.resize(201);
    for (int i = 0; i <= 200; i++) tansig[i] = (float)(floor(tanh(0.04 * (double)i) * 1e6 + 0.5) / 1e6);
    tansig[70] = 0.992631f;
    tansig[170] = 0.999997f;
    tansig[190] = 1.000000f;
    const int *E = kEbandHost;
    bin_frac.assign(400, 0.0f);
    bin_band.assign(400, 0);
    for (int i = 0; i < NB - 1; i++) {
        int band_size = (E[i + 1] - E[i]) << 2;
        for (int j = 0; j < band_size; j++) {
            bin_frac[(E[i] << 2) + j] = (float)j / (float)band_size;  // src/lib.rs:73
            bin_band[(E[i] << 2) + j] = i;
        }
    }
}

extern "C" void nnn_batch_destroy(nnn_batch *h)
{
    if (!h) return;
    NNN_RT_LOCK;
    hipSetDevice(h->device);
    hipDeviceSynchronize();
    for (int p = 0; p < 2; p++) {
        for (int s = 0; s < ST_COUNT; s++)
            for (int i = 0; i < EVR; i++)
                if (h->ev[p][s][i]) hipEventDestroy(h->ev[p][s][i]);
        if (h->ev_done[p]) hipEventDestroy(h->ev_done[p]);
    }
    if (h->ev_in) hipEventDestroy(h->ev_in);
    if (h->ev_last) hipEventDestroy(h->ev_last);
    for (hipEvent_t e : h->evp) hipEventDestroy(e);
    for (void *p : h->allocs) hipFree(p);
    if (h->fault_host) hipHostFree((void *)h->fault_host);
    h->sp_tab.release();
    for (hipEvent_t e : h->ev_up) hipEventDestroy(e);
    for (hipEvent_t e : h->ev_run) hipEventDestroy(e);
    if (h->copy_in) hipStreamDestroy(h->copy_in);
    if (h->copy_out) hipStreamDestroy(h->copy_out);
    h->stage.release();
    h->stage_vad.release();
    h->split_stage.release();
    h->zc_host.release();
    if (h->ss_dims) hipFree(h->ss_dims);
    if (h->ss_flag) hipFree(h->ss_flag);
    if (h->ss_bad_host) hipHostFree((void *)h->ss_bad_host);
    h->ss_idx.release();
    h->ss_idx_pin.release();
    if (h->ev_ss_idx) hipEventDestroy(h->ev_ss_idx);
    h->ss_stage.release();
    h->fl_stage.release();
    h->fl_pin.release();
    if (h->ev_fl) hipEventDestroy(h->ev_fl);
    delete[] h->plan.rnn;
    for (int i = 0; i < NSTREAMS; i++)
        if (h->pool[i]) hipStreamDestroy(h->pool[i]);
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
}

constexpr size_t kLdsMax = 160 * 1024;
// below this many RNN blocks a launch leaves compute units idle and the per-block chain dominates
// (measured at 1024 / 4096 / 16384 streams, profiles/r1_e_rnn_rows.txt)
constexpr int RNN_SMALL_BATCH_BLOCKS = 128;

// The kernel decisions of one resident model -- a run of `ntiles` whole tiles whose packed model is `pl` -- as the ModelGroup fields rows,
// rnn_lds, wp, wf_lds, shape_builtin, back_lds, rnn16_lds, acts and wf.  Reads its arguments only and touches no device, like plan_group and
// plan_call.  rows = 0: the model fits no RNN kernel (creation fails).
static nnn_batch::ModelGroup plan_model_group(const RnnPlan &pl, int ntiles, const Paths &paths)
{
    nnn_batch::ModelGroup G;
    G.plan = pl;
    G.ntiles = ntiles;
    // rows per block: the most that fit the LDS; fewer (more, shorter blocks) while the launch cannot fill the GPU
    G.rows = 0;
    for (int rows = 32; rows >= 16 && !G.rows; rows /= 2)   // (64 rows never fit: the states stay in LDS for a whole group)
        if ((size_t)rnn_lds(G.plan, rows).total <= kLdsMax) G.rows = rows;
    if (!G.rows) return G;
    while (G.rows > 16 && G.ntiles * (TILE / G.rows) < RNN_SMALL_BATCH_BLOCKS) G.rows /= 2;
    if (paths.rnn_rows && (size_t)rnn_lds(G.plan, paths.rnn_rows).total <= kLdsMax) G.rows = paths.rnn_rows;
    G.rnn_lds = (size_t)rnn_lds(G.plan, G.rows).total;
    // k_vad (the VAD calls): the most rows whose operands fit half the LDS -- two blocks per compute unit, which its 99 registers (four
    // waves per SIMD) allow -- failing that the LDS, and whose GRU units fit the eight waves.  The built-in shape class: a whole tile per
    // block.  Wherever k_rnn fits, 16 rows of this do; if none did, vad_rows stays 0 and the VAD calls alone refuse (vad_check).
    for (int half = 2; half >= 1 && !G.vad_rows; half--)
        for (int rows = TILE; rows >= 16 && !G.vad_rows; rows /= 2)
            if ((size_t)vad_lds(vad_plan_view(G.plan), rows).total <= kLdsMax / half && vad_gru_mb(G.plan, rows)) G.vad_rows = rows;
    if (G.vad_rows) {
        G.vad_mb = vad_gru_mb(G.plan, G.vad_rows);
        G.vad_lds = (size_t)vad_lds(vad_plan_view(G.plan), G.vad_rows).total;
    }
    // k_net (the network calls): 16 rows per block unless NNN_RNN_ROWS says otherwise -- two blocks per compute unit (114 registers, 48 KB
    // of LDS each for the built-in class) beat one block of 32 rows at every size measured.  Its LDS is k_rnn's
    // minus 1152 bytes per row, so whatever fits there fits here.
    G.net_rows = paths.rnn_rows && (size_t)net_lds(G.plan, paths.rnn_rows).total <= kLdsMax ? paths.rnn_rows : 16;
    G.net_lds = (size_t)net_lds(G.plan, G.net_rows).total;
    // models of the built-in shape class run the layer-pipelined kernel (its fixed wave roles cover 2 / 2 / 3 / 6 neuron
    // blocks in the input dense / vad / noise / denoise layers)
    G.wp = wf_plan_of(G.plan);   // (strides of its per-layer matrices)
    G.wf_lds = (size_t)wf_lds(G.wp).total;
    // the fused back end / its RNN stretch alone: layers of up to 8 neuron blocks (two units per wave) whose operands fit the LDS
    // (compiled for the built-in model's shape class; any other model takes the unfused kernels).  The packer laid the model out by
    // rnn_plan_for of its four layer sizes, the kernels of the class read by rnn_plan_for of the class's: the same sizes, the same format
    {
        constexpr RnnPlan cls = BkShapeBuiltin::plan();
        const bool shape_ok = pl.dense.n == cls.dense.n && pl.vad.n == cls.vad.n && pl.noise.n == cls.noise.n && pl.dn.n == cls.dn.n;
        G.shape_builtin = shape_ok;
        const size_t fb = (size_t)back_lds(G.plan, true).total, rb = (size_t)back_lds(G.plan, false).total;
        G.back_lds = shape_ok && fb <= kLdsMax ? fb : 0;
        G.rnn16_lds = shape_ok && rb <= kLdsMax ? rb : 0;
        G.acts = BkActs{G.plan.dense.act, G.plan.vad.act, G.plan.noise.act, G.plan.dn.act, G.plan.out.act, G.plan.act_vo};
    }
    G.wf = !paths.rnn_rows && G.plan.dense.nb <= 2 && G.plan.vad.nb <= 2 && G.plan.noise.nb <= 3 && G.plan.dn.nb <= 6 && G.plan.vad.rec.ksteps <= WF_KS_REC &&
           G.plan.noise.rec.ksteps <= WF_KS_REC && G.plan.dn.rec.ksteps <= WF_KS_REC && G.wf_lds <= kLdsMax;   // (k_rnn_wf's wave roles)
    return G;
}

// The steps of creation, in the order create_impl takes them.
// Arguments: the groups' stream counts (their sum into n_streams) and the device, which becomes the current one.
static int create_check_args(nnn_batch *h, const int *group_streams, int n_groups, int device, int gmax, int &n_streams)
{
    h->gmax = gmax < 1 ? 1 : (gmax > GROUP ? GROUP : gmax);
    n_streams = 0;
    for (int g = 0; g < n_groups; g++) {
        if (group_streams[g] <= 0) return fail("group %d: stream count must be positive", g);
        if (g + 1 < n_groups && group_streams[g] % TILE) return fail("group %d: every group but the last must be a multiple of %d streams", g, TILE);
        n_streams += group_streams[g];
    }
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail("no HIP device %d (found %d)", device, ndev);
    if (device >= MARK_DEVICES) return fail("device %d: the library keeps per-device call marks for devices 0 .. %d only", device, MARK_DEVICES - 1);
    HIPCHK(hipSetDevice(device));
    h->device = device;
    return 0;
}
static int create_streams_and_events(nnn_batch *h)
{
    HIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&h->ev_in, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&h->ev_last, hipEventDisableTiming));
    // (the internal streams of pipelined calls are created on first use: HIP spreads streams over a few hardware queues in
    // creation order, and a stream that shares its queue with the caller's blocks behind the caller's waits)
    for (int p = 0; p < 2; p++) {
        for (int s = 0; s < ST_COUNT; s++)
            for (int i = 0; i < EVR; i++) HIPCHK(hipEventCreateWithFlags(&h->ev[p][s][i], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&h->ev_done[p], hipEventDisableTiming));
    }
    return 0;
}
// pack every group's model (host side) and take its kernel decisions; the recurrent state is allocated at the widest layer sizes among them
static int create_model_groups(nnn_batch *h, const RNNModel *const *models, const int *group_streams, int n_groups, const Paths &paths,
                               std::vector<std::vector<uint16_t>> &wqs, std::vector<std::vector<float>> &fpars)
{
    wqs.resize(n_groups);
    fpars.resize(n_groups);
    h->groups.resize(n_groups);
    h->group_streams.assign(group_streams, group_streams + n_groups);
    memset(&h->md, 0, sizeof(h->md));
    for (int g = 0, tile0 = 0; g < n_groups; g++) {
        const RNNModel *model = models ? models[g] : nullptr;
        RNNModel *own = nullptr;
        if (!model) {
            size_t len;
            const uint8_t *w = nnn_builtin_weights(&len);
            own = nnn_model_parse(w, len);
            if (!own) return fail("built-in weights failed to parse");
            model = own;
        }
        h->models.push_back(*model);
        RnnPlan plan;
        ModelDims md;
        nnn_model_pack(*model, wqs[g], fpars[g], plan, md);
        delete own;
        nnn_batch::ModelGroup &G = h->groups[g];
        G = plan_model_group(plan, (group_streams[g] + TILE - 1) / TILE, paths);
        if (!G.rows) return fail("model too large for the RNN kernel's LDS operand matrices");
        G.tile0 = tile0;
        tile0 += G.ntiles;
        h->md.nd = md.nd > h->md.nd ? md.nd : h->md.nd;
        h->md.nv = md.nv > h->md.nv ? md.nv : h->md.nv;
        h->md.nn = md.nn > h->md.nn ? md.nn : h->md.nn;
        h->md.ndn = md.ndn > h->md.ndn ? md.ndn : h->md.ndn;
    }
    h->plan.rnn = new uint8_t[n_groups]();
    return 0;
}
// the state arrays (and the few per-call ones beside them), the mapped fault word, the parameter table
static int create_state_arrays(nnn_batch *h)
{
    const size_t Sp = (size_t)h->S_pad;
    const ModelDims &md = h->md;
    Buffers &b = h->b[0];
    memset(&b, 0, sizeof(b));
    b.S = h->S; b.S_pad = h->S_pad; b.NT = h->NT;
    b.nslot = h->nslot;
    b.gru_v_w = md.nv; b.gru_n_w = md.nn; b.gru_dn_w = md.ndn;
    // persistent state
    HIPCHK(dalloc(h, &b.hist, Sp * hist_stride(h->nslot), true));
    HIPCHK(dalloc(h, &b.hp_mem, Sp * 2, true));
    HIPCHK(dalloc(h, &b.hp_last, Sp, true));
    HIPCHK(dalloc(h, &b.dec, Sp * dec_len(h->nslot), true));
    HIPCHK(dalloc(h, &b.xlp0, Sp * h->nslot, true));
    HIPCHK(dalloc(h, &b.lpc_head, (size_t)h->NT * 5 * TILE, false));   // (made and used inside one call)
    HIPCHK(dalloc(h, &b.lpc, Sp * h->nslot * 10, false));   // (remade for every frame before it is read: not part of a snapshot)
    HIPCHK(dalloc(h, &b.ceps_mem, Sp * CEPS_MEM * NB, true));
    HIPCHK(dalloc(h, &b.mem_id, Sp, true));
    HIPCHK(dalloc(h, &b.synth_mem, Sp * FRAME, true));
    HIPCHK(dalloc(h, &b.lastg, Sp * NB, true));
    HIPCHK(dalloc(h, &b.last_period, Sp, true));
    HIPCHK(dalloc(h, &b.last_gain, Sp, true));
    HIPCHK(dalloc(h, &b.gru_v, Sp * md.nv, true));
    HIPCHK(dalloc(h, &b.gru_n, Sp * md.nn, true));
    HIPCHK(dalloc(h, &b.gru_dn, Sp * md.ndn, true));
    HIPCHK(dalloc(h, &b.stamps, 64, false));
    {   // the fault word lives in page-locked host memory the device writes straight into: the host reads it at every call
        void *hp = nullptr, *dp = nullptr;
        HIPCHK(hipHostMalloc(&hp, sizeof(int), hipHostMallocMapped));
        *(volatile int *)hp = 0;
        HIPCHK(hipHostGetDevicePointer(&dp, hp, 0));
        h->fault_host = (volatile int *)hp;
        b.fault = (int *)dp;
    }
    HIPCHK(dalloc(h, &b.ticket, 1, false));
    b.handoff_ticks = HANDOFF_TICKS;
    return grow(h, false, h->sp_tab, 2 * 64 * sizeof(StepParams), 64);
}
// the constant tables, then every group's packed weights
static int create_tables(nnn_batch *h, const std::vector<std::vector<uint16_t>> &wqs, const std::vector<std::vector<float>> &fpars)
{
    Buffers &b = h->b[0];
    std::vector<float> window, dct, tansig, bin_frac;
    std::vector<float2> tw;
    std::vector<int> bin_band;
    make_tables(window, dct, tw, tansig, bin_frac, bin_band, b.wnorm);
    HIPCHK(upload(h, &b.window, window));
    {
        std::vector<float> wa(WINDOW), ws(WINDOW);
        for (int i = 0; i < WINDOW; i++) { wa[i] = window[i] * 0.5f; ws[i] = window[i] * 0.5f; }
        HIPCHK(upload(h, &b.window_a, wa));
        HIPCHK(upload(h, &b.window_s, ws));
    }
    HIPCHK(upload(h, &b.dct, dct));
    HIPCHK(upload(h, &b.tw960, tw));
    HIPCHK(upload(h, &b.tansig, tansig));
    HIPCHK(upload(h, &b.bin_frac, bin_frac));
    HIPCHK(upload(h, &b.bin_band, bin_band));
    {   // band-sum segmentation: every band interval cut into segments of <= 8 bins (54 segments), one lane slot each; the slots of an
        // interval stay inside one row of 16 lanes (slots left idle where the next interval would straddle a row: 59 slots)
        const int *E = kEbandHost;
        std::vector<int> seg(192, 0);
        int ns = 0;
        for (int i = 0; i < NB - 1; i++) {
            int k = E[i] << 2, end = E[i + 1] << 2;
            const int need = (end - k + 7) / 8;
            if (need > 16) return fail("band interval too long for a row of lanes");
            if ((ns & 15) + need > 16) ns = (ns + 15) & ~15;   // (idle slots: count 0)
            seg[128 + i] = ns;
            while (k < end) {
                int c = end - k < 8 ? end - k : 8;
                if (ns >= 64) return fail("band segmentation overflow");
                seg[ns] = k;
                seg[64 + ns] = c;
                ns++;
                k += c;
            }
            seg[160 + i] = ns - seg[128 + i];
        }
        if (ns > 64) return fail("band segmentation overflow");
        HIPCHK(upload(h, &b.seg, seg));
        // the transform kernels' LDS tables, built once in their LDS layout
        std::vector<FftLds> img(1);
        fft_tables_image(img[0], tw.data(), bin_frac.data(), bin_band.data(), seg.data(), dct.data());
        const FftLds *dimg = nullptr;
        HIPCHK(upload(h, &dimg, img));
        b.fft_img = dimg;
    }
    for (size_t g = 0; g < h->groups.size(); g++) {
        const uint16_t *dq = nullptr;
        HIPCHK(upload(h, &dq, wqs[g]));
        h->groups[g].wq = (const uint4 *)dq;
        HIPCHK(upload(h, &h->groups[g].fpar, fpars[g]));
    }
    return 0;
}
// Every array of a scratch field list (NNN_WORK_FIELDS; NNN_TAP_FIELDS at the first nnn_batch_set_taps) for batch `h`: nset sets back to
// back in one allocation per array, then the views of sets 1 .. nset - 1 derived again.  Inside a function that returns the error code.
#define NNN_ALLOC_ONE(name, len) HIPCHK(dalloc(h, &h->b[0].name, (size_t)h->S_pad * (size_t)(len) * h->nset, false));
#define NNN_ALLOC_SETS(FIELDS)                                                              \
    do {                                                                                    \
        FIELDS(NNN_ALLOC_ONE)                                                               \
        for (int set = 1; set < h->nset; set++) h->b[set] = frame_view(h->b[0], set);       \
    } while (0)
// per-frame scratch (doubles as parity taps): every array holds nset sets back to back
static int create_scratch_sets(nnn_batch *h)
{
    // (the arrays only the parity taps fill, 4.1 KB per stream and set, wait for nnn_batch_set_taps(1))
    NNN_ALLOC_SETS(NNN_WORK_FIELDS);
    h->state_bufs.push_back({(void *)h->b[0].pflag, (size_t)h->S_pad * h->nset * sizeof(int)});   // frame numbers restart with reset / load_state
    return 0;
}
// the RNN kernels' dynamic LDS limit is a per-device function attribute: raise it to the hardware's 160 KB once
static int raise_lds_limits()
{
    for (const void *k : big_lds_kernels()) HIPCHK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
    return 0;
}

static int create_impl(nnn_batch *h, const RNNModel *const *models, const int *group_streams, int n_groups, int device, int gmax, const Paths &paths)
{
    int n_streams = 0;
    if (int rc = create_check_args(h, group_streams, n_groups, device, gmax, n_streams)) return rc;
    if (int rc = create_streams_and_events(h)) return rc;
    h->paths = h->created = paths;
    // groups in flight behind the high-pass: what the schedule chosen at creation can use (a schedule set later works on what is there).
    // Nobody choosing, batches above AUTO_BIG streams keep two groups in flight (round 6, see plan_call: their calls overlap kernels).
    h->depth = (paths.n_lanes >= 2 || paths.sched == SCHED_STAGES || (paths.sched_auto && (n_streams + TILE - 1) / TILE * TILE > AUTO_BIG)) ? DEPTH : 1;
    h->nset = h->depth * h->gmax;
    h->nslot = slots_for(h->gmax, h->depth);
    h->S = n_streams;
    h->S_pad = (n_streams + TILE - 1) / TILE * TILE;
    h->NT = h->S_pad / TILE;
    std::vector<std::vector<uint16_t>> wqs;
    std::vector<std::vector<float>> fpars;
    if (int rc = create_model_groups(h, models, group_streams, n_groups, paths, wqs, fpars)) return rc;
    if (int rc = create_state_arrays(h)) return rc;
    if (int rc = create_tables(h, wqs, fpars)) return rc;
    if (int rc = create_scratch_sets(h)) return rc;
    if (int rc = raise_lds_limits()) return rc;
    HIPCHK(hipDeviceSynchronize());
    h->id = g_next_batch_id.fetch_add(1) & 0xFFFFFu;
    if (!h->id) h->id = g_next_batch_id.fetch_add(1) & 0xFFFFFu;
    return 0;
}

static nnn_batch *create_batch(const RNNModel *const *models, const int *group_streams, int n_groups, int device, int gmax, const Paths &paths)
{
    NNN_RT_LOCK;
    nnn_batch *h = new nnn_batch();
    if (create_impl(h, models, group_streams, n_groups, device, gmax, paths) != 0) {
        std::string keep = g_err;
        nnn_batch_destroy(h);
        g_err = keep;
        return nullptr;
    }
    return h;
}

extern "C" nnn_batch *nnn_batch_create_opts(const RNNModel *const *models, const int *group_streams, int n_groups, int device,
                                             const nnn_batch_opts *opts)
{
    if (n_groups <= 0 || !group_streams) {
        fail("need at least one group of streams");
        return nullptr;
    }
    int gmax = GROUP;
    if (opts) {
        for (int r : opts->reserved)
            if (r != 0) {
                fail("nnn_batch_opts.reserved must be zero");
                return nullptr;
            }
        if (opts->max_group_frames < 0) {
            fail("nnn_batch_opts.max_group_frames must not be negative");
            return nullptr;
        }
        if (opts->max_group_frames > GROUP) {
            fail("nnn_batch_opts.max_group_frames must not exceed %d (the kernels' longest frame group)", GROUP);
            return nullptr;
        }
        if (opts->max_group_frames > 0) gmax = opts->max_group_frames;
    }
    return create_batch(models, group_streams, n_groups, device, gmax, read_paths());
}

extern "C" nnn_batch *nnn_batch_create_grouped(const RNNModel *const *models, const int *group_streams, int n_groups, int device)
{
    return nnn_batch_create_opts(models, group_streams, n_groups, device, nullptr);
}

extern "C" int nnn_batch_max_group_frames(const nnn_batch *h) { return h ? h->gmax : 0; }
extern "C" size_t nnn_batch_device_bytes(const nnn_batch *h) { return h ? h->device_bytes : 0; }

extern "C" nnn_batch *nnn_batch_create(const RNNModel *model, int n_streams, int device)
{
    if (n_streams <= 0) {
        fail("n_streams must be positive");
        return nullptr;
    }
    return nnn_batch_create_grouped(&model, &n_streams, 1, device);
}

extern "C" int nnn_batch_num_streams(const nnn_batch *h) { return h ? h->S : 0; }

extern "C" int nnn_batch_synchronize(nnn_batch *h)
{
    if (!h) return fail("null batch");
    HIPCHK(hipSetDevice(h->device));
    if (h->have_last) HIPCHK(hipEventSynchronize(h->ev_last));   // the most recent call, whatever stream it was made on
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->ss_bad_host && *h->ss_bad_host) {   // (reported once)
        *h->ss_bad_host = 0;
        return fail("nnn_batch_import_streams_device: a record did not match its target stream (magic, version, size or GRU sizes); "
                    "that import wrote nothing");
    }
    return report_fault(h);
}

extern "C" int nnn_batch_reset(nnn_batch *h)
{
    NNN_RT_LOCK;
    if (!h) return fail("null batch");
    if (int rc = quiesce(h)) return rc;
    for (auto &sb : h->state_bufs) HIPCHK(hipMemset(sb.first, 0, sb.second));
    if (int rc = hold_release_all(h)) return rc;   // (every hold is released: a fresh batch holds nothing)
    HIPCHK(hipDeviceSynchronize());
    *h->fault_host = 0;
    h->frame_count = 0;
    h->group_count = 0;
    h->last_set = 0;
    h->prev_pipe = false;
    h->pending = 0;   // (frames analysed and never synthesised are dropped with the rest)
    return 0;
}
