// nnn_batch_core.hip -- what every other part of the batch's host side stands on: the error text and the runtime lock, the knob table,
// the plan types, grow-only buffers, struct nnn_batch with report_fault, quiesce and its allocation helpers, and the entry points that need
// no batch.
// Needs only the includes of nnn_batch.hip (the kernels' layout types among them).
#pragma once

static thread_local std::string g_err;
// States are independent and may be driven from different threads.  What must not overlap across
// threads is stream capture on one thread with allocation, freeing or legacy-stream (synchronous memset / memcpy) calls
// on another: the HIP runtime rejects those ("would make the legacy stream depend on a capturing blocking stream").
// Those short sections -- never the per-frame launches -- take this lock.
static std::recursive_mutex g_rt_mu;
// The real-time serving pattern: independent batches ticking one frame per call, each on its own HIP stream.  A batch that sees
// others doing so runs its one-frame groups on k_rnn, which does not hold every compute unit for the pipelined kernel's five
// ticks.  (Also tried for that pattern: running short calls on the batch's own stream so that two batches would not
// depend on the hardware queue their callers' streams share -- 2 x 4096 streams 23.5 -> 19.0 M frames/s, 8 x 4096 43.2 -> 36.4:
// the extra event hops cost more than they free; with GPU_MAX_HW_QUEUES=8 in the environment two batches do overlap, 33.5 M.)
// "Other batches are ticking beside this one": another batch made a call within the last few milliseconds (remembered for 20 ms).
// Alive is not enough -- a host may hold idle batches -- and the answer only picks between two kernels that give the same bits.
// One mark per DEVICE: a batch on another GPU (the node object drives one batch per device, all ticking at once) is not "beside" this one --
// until round 5 the mark was process-wide and every shard of a node saw its neighbours on other GPUs, so the node never took the tick kernels.
constexpr int MARK_DEVICES = 64;
static std::atomic<uint64_t> g_call_mark[MARK_DEVICES];   // [device]: (batch id << 44) | microseconds of the most recent call of any batch on that device
static std::atomic<uint64_t> g_next_batch_id{1};
#define NNN_RT_LOCK std::lock_guard<std::recursive_mutex> rt_lock_(g_rt_mu)
extern "C" const char *nnn_last_error(void) { return g_err.c_str(); }
// The CPUs local to a device's PCI function, in the kernel's cpulist syntax (/sys/bus/pci/devices/<id>/local_cpulist): what the node
// object pins a device's host thread to.  0 and the text in buf, or non-zero when the platform does not say.
extern "C" int nnn_device_local_cpulist(int device, char *buf, size_t cap)
{
    if (!buf || cap < 2) return 1;
    buf[0] = 0;
    char id[64] = {0};
    if (hipDeviceGetPCIBusId(id, (int)sizeof(id), device) != hipSuccess || !id[0]) return 1;
    for (char *p = id; *p; p++)
        if (*p >= 'A' && *p <= 'F') *p = (char)(*p - 'A' + 'a');   // sysfs spells the address in lower case
    char path[160];
    snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/local_cpulist", id);
    FILE *f = fopen(path, "r");
    if (!f) return 1;
    const bool ok = fgets(buf, (int)cap, f) != nullptr;
    fclose(f);
    if (!ok) { buf[0] = 0; return 1; }
    for (char *p = buf; *p; p++)
        if (*p == '\n' || *p == '\r') *p = 0;
    return buf[0] ? 0 : 1;
}
static int fail(const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return 1;
}
int nnn_set_error(const char *msg) { return fail("%s", msg); }   // for the library's other translation units
#define HIPCHK(expr)                                                                       \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) return fail("%s failed: %s", #expr, hipGetErrorString(e_));  \
    } while (0)

// The HIP runtime maps streams onto four hardware queues unless GPU_MAX_HW_QUEUES says otherwise, and two batches whose streams land on one
// queue do not overlap (two 4096-stream batches ticking: 31.3 M frames/s, 43.3 M with eight queues).  The runtime reads the variable when it
// initialises -- at the host's first HIP call -- and it is the HOST's setting: the library does not touch its host's environment (until
// round 4 a constructor exported it; VERDICT r4 #7b).  INTEGRATION.md tells real-time hosts to export GPU_MAX_HW_QUEUES=8 themselves.

// Run-time knobs.  The default build reads exactly the environment variables of the table in include/nnn_batch.h ("Environment"), each at
// batch creation and each exercised by a test.  Four more are developer knobs that let the tests force a path (NNN_HP_TPB, NNN_X_RIDES,
// NNN_LPC_WIDE, NNN_LPC_FC), compiled in only with -DNNN_DEV_KNOBS -- the interpreter build of the tests and scripts/build_variant*.sh
// define it -- and absent from the product.
static const char *knob(const char *name) { return getenv(name); }
#ifdef NNN_DEV_KNOBS
static const char *dev_knob(const char *name) { return getenv(name); }
#else
static const char *dev_knob(const char *) { return nullptr; }
#endif

enum KernelId { K_HP, K_LPC, K_PITCH, K_FFT_XP, K_RNN, K_SYNTH, K_BACK, K_COUNT };
static const char *kKernelNames[K_COUNT] = {"k_hp", "k_lpc", "k_pitch", "k_fft_xp", "k_rnn", "k_synth", "k_back"};

// The five stages of a frame group, one kernel launch each (hp: k_hp + k_lpc; k_rnn: one per resident model).  hp, pitch, rnn and synth carry
// state from frame to frame and loop over the group's frames inside the launch; fft_xp covers all frames of the group
// side by side (block index = frame * blocks_per_frame + block).
enum Stage { ST_HP, ST_PITCH, ST_FFT, ST_RNN, ST_SYN, ST_COUNT };
// The two launches only the split calls make (launch_stage; no events, no schedule nodes: a split call is one group in order on one stream):
// ST_FEAT ends nnn_batch_analyze_* (k_features, then the rows out), ST_GAINS begins nnn_batch_synthesize_* (the caller's gains in).
// The two only the VAD calls make (nnn_batch_vad_*): ST_FFT_FEAT is the transform stage without the spectra's trip
// to memory (k_fft_feat; k_fft_xp while the taps are on), ST_VAD the feature stage and the network up to the VAD output (k_features, k_vad).
enum SplitStage { ST_FEAT = ST_COUNT, ST_GAINS, ST_FFT_FEAT, ST_VAD };
struct SplitIo {                   // the caller's row buffers of a split call (device memory)
    float *features = nullptr;     // [n_frames][n_streams][42]
    int *silence = nullptr;        // [n_frames][n_streams]
    const float *gains = nullptr;  // [n_frames][n_streams][22]
    const float *vad = nullptr;    // [n_frames][n_streams], may be null
};
constexpr int NSTREAMS = 5;    // internal streams of a pipelined call
constexpr int EVR = 16;        // event ring: groups of one call that may still be referred to
enum SchedMode { SCHED_SEQ = 0, SCHED_LANES = 1, SCHED_STAGES = 2 };
constexpr int AUTO_BIG = 16384;   // streams above which the automatic schedule changes (plan_call)
constexpr long long HANDOFF_TICKS = 10000ll * 100000ll;   // Buffers::handoff_ticks outside the test hook: 10 s of the 100 MHz clock

// Every setting that picks a kernel or a schedule.  read_paths fills it from the environment at batch creation; the setters change
// back_mode, use_pipeline, inputs_ready and (nnn_batch_set_schedule) sched, n_lanes and sched_auto later.  Only creation, the two plan
// functions (plan_call, plan_group) and the host-buffer plans (plan_host_call, plan_train_chunk) read it.
struct Paths {
    int sched = SCHED_LANES;       // how a multi-frame call spreads over streams (env NNN_SCHED: seq | lanes | stages)
    bool sched_auto = true;        // nobody chose a schedule (NNN_SCHED / NNN_LANES / nnn_batch_set_schedule): the rule of plan_call
    int n_lanes = 1;               // SCHED_LANES: lanes (the caller's stream + internal ones) besides the high-pass stream; env NNN_LANES, 1..4.
                                   // One since the end of round 3: with the frames of a group side by side in every kernel a second group in flight
                                   // only gets in the first one's way (4096 streams: 55.5 against 54.8 M frames/s, 16 384: 63.8 / 62.3; profiles AN)
                                   // (measured at 4096 streams x 48 frames: 1: 28.5, 2: 37.1, 3: 32.9, 4: 32.2 M frames/s -- the default 4 hardware
                                   // queues are shared with the host's own streams)
    int host_chunk = -1;           // frames per chunk of a host-buffer call (env NNN_HOST_CHUNK): -1 = by call length and size (small
                                   // calls zero-copy), 0 = the whole call in one piece; set, it always takes the staged path
    int wf_min_g = 0;              // groups shorter than this run k_rnn instead of the layer-pipelined kernel (env NNN_RNN_WF_MIN_G; 0 = by batch size)
    int rnn_rows = 0;              // forced rows per RNN block (env NNN_RNN_ROWS), 0 = by model size and batch size
    int hp_split = -1;             // k_hp on two waves per tile (k_hp2): -1 = for launches of up to 256 tiles, 0 / 1 = never / always (env NNN_HP_SPLIT)
    int lpc_head = -1;             // one-frame calls: the LPC sums' first 608 steps in k_hp2's launch (0 = never; env NNN_LPC_HEAD)
    int pitch_chain = 1;           // k_pitch: one workgroup per (frame, quarter tile) instead of a frame loop: 1 = below 16384 streams, 0 = never, 2 = always (env NNN_PITCH_CHAIN)
    int hp_tpb = 0;                // k_hp2's tiles per block: 0 = by launch (2 for groups, 1 for lone frames), 1 / 2 forced (env NNN_HP_TPB)
    int x_rides = -1;              // one-frame calls: the fused back end's X transform in rider blocks of k_pitch's launch (-1 = up to 8192 streams; env NNN_X_RIDES)
    int lpc_wide = -1;             // k_lpc_wide (one lag per wave): -1 = for launches below 512 waves, 0 / 1 = never / always (env NNN_LPC_WIDE)
    int lpc_fc = 0;                // k_lpc: frames per wave, 0 = by launch size (env NNN_LPC_FC)
    int back_mode = -1;            // the fused back end (k_back, nnn_back.hip): 0 = never, 1 = one-frame groups (the real-time tick), 2 = every group;
                                   // 3 / 4 = its RNN stretch alone (k_back<false>) in place of k_rnn / k_rnn_wf for one-frame / all groups;
                                   // -1 = by measurement (plan_group): one-frame groups only, fused up to 8192 streams, the RNN stretch
                                   // alone above that or with other batches ticking beside this one (nnn_batch_set_back_end)
    bool use_pipeline = true;      // nnn_batch_set_pipeline
    bool inputs_ready = false;     // the caller's promise that a call's input is final when the call is made (nnn_batch_set_inputs_ready)
};
static Paths read_paths()
{
    Paths p;
    if (const char *e = knob("NNN_HOST_CHUNK")) p.host_chunk = atoi(e);
    if (const char *e = knob("NNN_RNN_WF_MIN_G")) p.wf_min_g = atoi(e);
    if (const char *e = knob("NNN_HP_SPLIT")) p.hp_split = atoi(e);
    if (const char *e = dev_knob("NNN_HP_TPB")) p.hp_tpb = atoi(e);
    if (const char *e = knob("NNN_LPC_HEAD")) p.lpc_head = atoi(e);
    if (const char *e = dev_knob("NNN_X_RIDES")) p.x_rides = atoi(e);
    if (const char *e = knob("NNN_PITCH_CHAIN")) p.pitch_chain = atoi(e);
    if (const char *e = dev_knob("NNN_LPC_WIDE")) p.lpc_wide = atoi(e);
    if (const char *e = dev_knob("NNN_LPC_FC")) p.lpc_fc = atoi(e);
    if (const char *e = knob("NNN_SCHED")) {
        if (!strcmp(e, "seq")) p.sched = SCHED_SEQ;
        else if (!strcmp(e, "lanes")) p.sched = SCHED_LANES;
        else if (!strcmp(e, "stages")) p.sched = SCHED_STAGES;
        p.sched_auto = false;
    }
    if (const char *e = knob("NNN_LANES")) {
        const int v = atoi(e);
        if (v >= 1 && v <= NSTREAMS - 1) p.n_lanes = v;
        p.sched_auto = false;
    }
    if (const char *e = knob("NNN_RNN_ROWS")) {
        const int v = atoi(e);
        if (v == 16 || v == 32) p.rnn_rows = v;
    }
    return p;
}

// What one group of frames runs (plan_group; launch_stage dispatches on it)
enum BackEnd { BACK_UNFUSED = 0, BACK_RNN_ALONE = 1, BACK_FUSED = 2 };   // k_fft_xp -> RNN -> k_synth, the same with k_back<false> as the RNN, k_back<true>
enum RnnKernel : uint8_t { RK_BACK, RK_WF_BUILTIN, RK_WF_ANY, RK_PLAIN };   // k_back<false>, k_rnn_wf<BkShapeBuiltin>, k_rnn_wf<WfShapeAny>, k_rnn
struct GroupPlan {
    int g = 0;                     // frames
    BackEnd back = BACK_UNFUSED;
    int hp = 0;                    // 0 = k_hp, 1 / 2 = k_hp2<1> / k_hp2<2>
    bool held = false;             // some stream is held (nnn_batch_hold_streams): the high-pass, pitch and back-end kernels in the instantiations that
                                   // look at the live mask (and feed held streams zeros); otherwise the code a batch without a mask runs
    bool floor = false;            // some stream has a gain floor (nnn_batch_set_gain_floor): the back-end kernels in the instantiations that read the floor
                                   // rows; otherwise the code a batch without floors runs
    bool link = false;             // the channels of the batch's stream groups are linked (nnn_batch_set_channel_link): the back-end kernels in the
                                   // instantiations whose gains sink links; otherwise the code a batch without a link runs
    bool head = false;             // k_hp2 also runs the LPC sums' head (and k_pitch<true> takes it)
    bool lpc_in_pitch = false;     // k_pitch<true> does the LPC analysis
    int lpc_fc = 0;                // otherwise: k_lpc with lpc_fc frames per wave behind the high-pass, 0 = k_lpc_wide (lpc_launch)
    bool chain = false;            // k_pitch's frames side by side, chained through flags
    bool riders = false;           // the fused back end's X transform in rider blocks of k_pitch's launch
    uint8_t *rnn = nullptr;        // RnnKernel of each resident model group (made at creation)
};

// A runtime buffer that is kept from call to call (per-call hipMalloc / hipFree cost more than a frame) and replaced by a larger one when
// a call needs more.  `cap` is in the site's own unit (bytes, entries, frames).
enum MemKind : uint8_t { MEM_DEVICE, MEM_PINNED, MEM_MAPPED };   // hipMalloc; page-locked host memory; the same, mapped into the device's address space
template <class T> struct GrowBuf {
    T *p = nullptr;
    size_t cap = 0;
    MemKind kind = MEM_DEVICE;
    int release()
    {
        if (p) HIPCHK(kind == MEM_DEVICE ? hipFree(p) : hipHostFree(p));
        p = nullptr, cap = 0;
        return 0;
    }
    hipError_t alloc(size_t n) { return kind == MEM_DEVICE ? hipMalloc((void **)&p, n) : hipHostMalloc((void **)&p, n, kind == MEM_MAPPED ? hipHostMallocMapped : 0); }
};

struct nnn_batch {
    Buffers b[NSET];               // same state, NSET scratch sets (views into one allocation per scratch array: set s lies
                                   // s * S_pad * LEN after set 0, see frame_view); a group of frames takes consecutive sets
    ModelDims md;                  // state widths: the maxima over the resident models
    struct ModelGroup {            // a run of whole tiles sharing one model
        RnnPlan plan;
        const uint4 *wq = nullptr;     // packed bf16 weights (device)
        const float *fpar = nullptr;   // biases + vad output layer (device)
        size_t rnn_lds = 0;            // dynamic LDS bytes at `rows`
        bool wf = false;               // the layer-pipelined kernel (k_rnn_wf) runs this group
        bool shape_builtin = false;    // ... in its form compiled for the built-in shape class (every plan field a constant)
        WfPlan wp;
        size_t wf_lds = 0;
        int rows = 32;                 // stream rows per RNN block: 32 or 16
        int tile0 = 0, ntiles = 0;
        size_t back_lds = 0, rnn16_lds = 0;   // dynamic LDS of k_back<true> / k_back<false>; 0 = the model is outside the kernel's shape class
        BkActs acts = {};
        int vad_rows = 0, vad_mb = 0;         // k_vad: stream rows per block, stream blocks per GRU wave unit (plan_model_group)
        size_t vad_lds = 0;
        int net_rows = 0;                     // k_net (the network calls): stream rows per block, its dynamic LDS (plan_model_group)
        size_t net_lds = 0;
    };
    Paths paths;                   // as of now
    Paths created;                 // as the batch was created with (clone: depth, rows and kernel forms follow from it)
    GroupPlan plan;                // the group being enqueued
    std::vector<ModelGroup> groups;
    std::vector<RNNModel> models;  // host copies of the resident models (clone)
    std::vector<int> group_streams;
    int device = 0;
    int S = 0, S_pad = 0, NT = 0;
    uint64_t frame_count = 0;
    int depth = 1;                 // scratch-set blocks in rotation = groups in flight behind the high-pass (1 or DEPTH)
    int gmax = GROUP;              // frames per group at most (nnn_batch_opts.max_group_frames): sizes the scratch sets and the history rings
    int nset = GROUP, nslot = slots_for(GROUP, 1);
    size_t device_bytes = 0;       // everything dalloc / upload allocated
    uint64_t group_count = 0;      // groups launched so far: group_count % depth picks the block of gmax scratch sets
    int last_set = 0;              // scratch set of the most recent frame (parity taps)
    std::vector<void *> allocs;     // everything hipMalloc'ed
    std::vector<std::pair<void *, size_t>> state_bufs;  // zeroed by reset, copied by clone / save / load
    GrowBuf<char> stage;            // device staging of the host-buffer entry points (capacities in bytes)
    GrowBuf<float> stage_vad;
    std::vector<char> stage_host;   // host side of the copy back
    // small host-buffer calls (the drop-in single-stream surface: a batch of one, a frame per call) skip both copies: the kernels read the
    // input from, and write the audio and the VAD into, page-locked host memory mapped into the device's address space (round 6)
    GrowBuf<char> zc_host{nullptr, 0, MEM_MAPPED};   // (made on first use, ZC_MAX bytes)
    char *zc_dev = nullptr;
    hipStream_t copy_in = nullptr, copy_out = nullptr;   // host-buffer calls in chunks: uploads, downloads (created on first use)
    std::vector<hipEvent_t> ev_up, ev_run;               // per chunk: uploaded, processed
    GrowBuf<StepParams> sp_tab;     // device, per-frame parameter table of a call: two tables of `cap` frames, consecutive calls alternate
    hipStream_t stream = nullptr;   // default launch stream
    hipStream_t pool[NSTREAMS] = {};   // internal streams of pipelined calls
    hipEvent_t ev[2][ST_COUNT][EVR] = {}; // [call parity]: stage s of group (k mod EVR) of that call done
    hipEvent_t ev_done[2] = {};     // [call parity]: that call complete, on the stream it was made on
    bool have_done[2] = {false, false};
    // the previous call, if it was a pipelined one: the next call's high-pass chain may be started before it has drained
    // (nnn_batch_set_inputs_ready) and needs its synthesis events for the history rings
    bool prev_pipe = false;
    hipStream_t prev_st = nullptr;
    uint64_t prev_frame0 = 0;
    int prev_par = 0;
    std::vector<int> prev_first;
    volatile int *fault_host = nullptr;   // host view of Buffers::fault (page-locked, mapped): a hand-off that never arrived
    unsigned tickets = 0;           // work items handed out so far by chained k_pitch launches (Buffers::ticket never restarts)
    unsigned *frame_log = nullptr;  // nnn_batch_set_frame_log: the next frame's record (device), and the frames that still have room
    size_t frame_log_left = 0;
    uint64_t id = 0, other_seen_us = 0;   // see g_call_mark
    bool beside_others = false;     // as of the current call
    bool host_call = false;         // inside a host-buffer entry point: the input is an upload enqueued by this library, final only in stream order
    hipEvent_t ev_in = nullptr;     // the caller's stream at the start of a pipelined call
    hipEvent_t ev_last = nullptr;   // end of the most recent call, on the stream it was made on
    hipStream_t last_stream = nullptr;
    bool have_last = false;
    uint64_t call_count = 0;
    bool taps_alloc = false;        // the tap-only scratch arrays exist
    bool profiling = false;
    std::vector<hipEvent_t> evp;    // pairs per launch while profiling
    std::vector<int> evp_kernel;
    double k_ms[K_COUNT] = {0};
    int64_t k_launches[K_COUNT] = {0};
    // per-stream state records (nnn_batch_*_streams), made on first use; none of it is counted in device_bytes or copied by snapshots
    int *ss_dims = nullptr;            // device, per tile: the GRU sizes of its model, nv | nn << 8 | ndn << 16
    int *ss_flag = nullptr;            // device: the record check of a device import found a bad record (the import kernel then writes nothing)
    volatile int *ss_bad_host = nullptr;   // host view of the same verdict (page-locked, mapped): reported by nnn_batch_synchronize
    int *ss_bad_dev = nullptr;
    GrowBuf<int> ss_idx;               // device copy of a long scattered index list, and its page-locked source (capacity in entries)
    GrowBuf<int> ss_idx_pin{nullptr, 0, MEM_PINNED};
    hipEvent_t ev_ss_idx = nullptr;    // the last copy out of ss_idx_pin is done
    bool ss_idx_busy = false;
    GrowBuf<char> ss_stage;            // the host variants' records on the device (capacity in bytes)
    // held streams (nnn_batch_hold_streams), made on the first hold and counted in device_bytes
    unsigned *park = nullptr;          // device: the parked record of every stream, [S][NNN_STREAM_STATE_BYTES / 4]; valid while the stream is held
    unsigned long long *live = nullptr;   // device: Buffers::live of every scratch set's argument block
    std::vector<uint8_t> held;         // the host's copy of the mask, for checking arguments and for the host-buffer calls' copies back
    int n_held = 0;
    // gain floors (nnn_batch_set_gain_floor): configuration, not state -- in no record and no snapshot, untouched by
    // reset and load_state.  The rows are made on the first set and counted in device_bytes; the argument blocks point at them only while
    // some floor is above 0 (Buffers::gfloor), so that a batch whose floors are all off runs what a batch without floors runs
    float *gfloor = nullptr;           // device: TI [22] per stream
    std::vector<float> gfloor_host;    // the host's copy, [S][22] (empty until the first set): what get returns and num_floored counts
    int n_floored = 0;                 // streams with any floor > 0
    GrowBuf<char> fl_stage;            // device: a set call's list and values (capacity in entries)
    GrowBuf<char> fl_pin{nullptr, 0, MEM_PINNED};   // ... and their page-locked source
    hipEvent_t ev_fl = nullptr;        // the last copy out of fl_pin is done
    bool fl_busy = false;
    // channel link (nnn_batch_set_channel_link): configuration, not state -- two integers of the host's, carried to
    // the kernels in the argument blocks (Buffers::link), so a set is ordered with the launches by being made between them
    int link_ch = 1, link_mode = 0;    // channels 1 / 2 / 4, NNN_LINK_OFF / MAX / MIN (off is kept as channels 1, mode NNN_LINK_OFF)
    // split calls (nnn_batch_analyze_* / nnn_batch_synthesize_*): frames analysed and not yet synthesised, the
    // scratch sets they lie in and the ring slot of the first one
    int pending = 0, pending_set0 = 0, pending_slot = 0;
    GrowBuf<float> split_stage;        // the host variants' rows on the device: features | silence, or gains | vad (capacity in frames)
};

// While frames are pending every call that reads or moves per-stream state is refused, changing nothing (include/nnn_batch.h).
static int refuse_pending(const nnn_batch *h, const char *what)
{
    if (!h || !h->pending) return 0;
    return fail("%s refused: %d frames are pending (analysed by nnn_batch_analyze_* and not yet synthesised); "
                "nnn_batch_synthesize_* of the same n_frames comes first (nnn_batch_reset drops them)", what, h->pending);
}

// A pitch workgroup that never saw its predecessor's hand-off flag went on with a stale pitch: the streams' state is invalid from
// that frame on.  Sticky: every later call and nnn_batch_synchronize report it until nnn_batch_reset / nnn_batch_load_state.
extern "C" int nnn_batch_fault(const nnn_batch *h) { return h && h->fault_host && *h->fault_host ? 1 : 0; }
static int report_fault(const nnn_batch *h)
{
    if (!nnn_batch_fault(h)) return 0;
    return fail("a pitch workgroup gave up waiting for the previous frame's result (frame hand-off flag never set): the state of the "
                "affected streams is invalid from that frame on; nnn_batch_reset or nnn_batch_load_state clears the condition "
                "(NNN_PITCH_CHAIN=0 runs the frames of a group in a loop instead of side by side)");
}

// everything this batch has enqueued anywhere is complete
static int quiesce(nnn_batch *h)
{
    HIPCHK(hipSetDevice(h->device));
    if (h->have_last) HIPCHK(hipEventSynchronize(h->ev_last));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int i = 0; i < NSTREAMS; i++)
        if (h->pool[i]) HIPCHK(hipStreamSynchronize(h->pool[i]));
    return 0;
}

// `a` (and a companion `b` that grows with it) replaced by buffers of a_bytes (b_bytes), capacity `cap`: under the runtime lock and, where
// `drain` says that enqueued work may still use the old ones, once everything the batch has enqueued is complete.
template <class A, class B = char> static int grow(nnn_batch *h, bool drain, GrowBuf<A> &a, size_t a_bytes, size_t cap, GrowBuf<B> *b = nullptr, size_t b_bytes = 0)
{
    NNN_RT_LOCK;
    if (int rc = drain ? quiesce(h) : 0) return rc;
    if (int rc = a.release()) return rc;
    if (int rc = b ? b->release() : 0) return rc;
    HIPCHK(a.alloc(a_bytes));
    if (b) HIPCHK(b->alloc(b_bytes));
    a.cap = cap;   // (only now that every allocation has succeeded: a failed grow leaves the capacity zero, and the next call tries again)
    if (b) b->cap = cap;
    return 0;
}

template <class T> static hipError_t dalloc(nnn_batch *h, T **p, size_t count, bool is_state)
{
    size_t bytes = count * sizeof(T);
    hipError_t e = hipMalloc((void **)p, bytes ? bytes : 4);
    if (e != hipSuccess) return e;
    h->allocs.push_back(*p);
    h->device_bytes += bytes ? bytes : 4;
    e = hipMemset(*p, 0, bytes);
    if (is_state) h->state_bufs.push_back({(void *)*p, bytes});
    return e;
}
template <class T> static hipError_t upload(nnn_batch *h, const T **p, const std::vector<T> &v)
{
    T *d = nullptr;
    hipError_t e = dalloc(h, &d, v.size(), false);
    if (e != hipSuccess) return e;
    *p = d;
    return hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}

// Page-locked host memory for the host-buffer entry points: transfers from / to it are DMA and overlap with each other and
// with the kernels; any other host pointer works too, through the runtime's own staging.
extern "C" void *nnn_host_alloc(size_t bytes)
{
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) {
        fail("nnn_host_alloc: %zu bytes of page-locked memory not available", bytes);
        return nullptr;
    }
    return p;
}
extern "C" void nnn_host_free(void *p)
{
    if (p) hipHostFree(p);
}
