// nnn_batch.hip -- host side of the batched process_frame backend: the state slab in HBM, the
// frame-group kernel pipeline (five stages, six launches per group, spread over a few HIP streams for long calls), parity taps,
// per-kernel timing.
// C ABI declared in include/nnn_batch.h.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <chrono>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/nnn_batch.h"
#include "../../include/nnn_train.h"
#include "nnn_back.hip"
#include "nnn_model.h"

using namespace nnn;

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
static int quiesce(nnn_batch *h);
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
};

static int hold_prepare(nnn_batch *h);
static int hold_release_all(nnn_batch *h);

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
    static const int E[NB] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24, 28, 34, 40, 48, 60, 78, 100};
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
    h->zc_host.release();
    if (h->ss_dims) hipFree(h->ss_dims);
    if (h->ss_flag) hipFree(h->ss_flag);
    if (h->ss_bad_host) hipHostFree((void *)h->ss_bad_host);
    h->ss_idx.release();
    h->ss_idx_pin.release();
    if (h->ev_ss_idx) hipEventDestroy(h->ev_ss_idx);
    h->ss_stage.release();
    delete[] h->plan.rnn;
    for (int i = 0; i < NSTREAMS; i++)
        if (h->pool[i]) hipStreamDestroy(h->pool[i]);
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
}

// dynamic LDS of k_rnn (mirrors its carve-up): tanh table (256 floats) + live flags (2 x 64 ints), 3 bf16 planes of the
// input matrix, the r * state matrix, the three state matrices and the feature staging for `rows` streams, the cepstral
// ring and its pair distances ((8 x 22 + 28) x `rows` floats)
static size_t rnn_lds_bytes(const RnnPlan &pl, int rows)
{
    auto sw = [](const LayerDesc &L) { return (size_t)(32 * L.rec.ksteps + 8); };
    const size_t cols = (size_t)pl.in_w + pl.rec_w + sw(pl.vad) + sw(pl.noise) + sw(pl.dn) + FS_W;
    return (256 + 128) * 4 + (size_t)3 * rows * cols * 2 + (size_t)(CEPS_MEM * NB + 28) * rows * 4;
}
constexpr size_t kLdsMax = 160 * 1024;
// the layer-pipelined kernel: strides of its per-layer matrices and its dynamic LDS (mirrors k_rnn_wf's carve-up)
static WfPlan rnn_wf_plan(const RnnPlan &pl) { return wf_plan_of(pl); }
static size_t rnn_wf_lds_bytes(const WfPlan &w)
{
    const size_t cols = (size_t)w.w_v + 2 * w.w_n + 3 * w.w_dn + 2 * ((size_t)w.sw_v + w.sw_n + w.sw_dn) + WF_FS_W;
    return (256 + 128) * 4 + (size_t)3 * WF_ROWS * cols * 2 + (size_t)(CEPS_MEM * NB + 28 + 28) * WF_ROWS * 4;
}
// below this many RNN blocks a launch leaves compute units idle and the per-block chain dominates
// (measured at 1024 / 4096 / 16384 streams, profiles/r1_e_rnn_rows.txt)
constexpr int RNN_SMALL_BATCH_BLOCKS = 128;

static int create_impl(nnn_batch *h, const RNNModel *const *models, const int *group_streams, int n_groups, int device, int gmax, const Paths &paths)
{
    h->gmax = gmax < 1 ? 1 : (gmax > GROUP ? GROUP : gmax);
    int n_streams = 0;
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
    h->paths = h->created = paths;
    // groups in flight behind the high-pass: what the schedule chosen at creation can use (a schedule set later works on what is there).
    // Nobody choosing, batches above AUTO_BIG streams keep two groups in flight (round 6, see plan_call: their calls overlap kernels).
    h->depth = (paths.n_lanes >= 2 || paths.sched == SCHED_STAGES || (paths.sched_auto && (n_streams + TILE - 1) / TILE * TILE > AUTO_BIG)) ? DEPTH : 1;
    h->nset = h->depth * h->gmax;
    h->nslot = slots_for(h->gmax, h->depth);
    h->S = n_streams;
    h->S_pad = (n_streams + TILE - 1) / TILE * TILE;
    h->NT = h->S_pad / TILE;
    const size_t Sp = (size_t)h->S_pad;

    // pack every group's model; the recurrent state is allocated at the widest layer sizes among them
    std::vector<std::vector<uint16_t>> wqs(n_groups);
    std::vector<std::vector<float>> fpars(n_groups);
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
        nnn_batch::ModelGroup &G = h->groups[g];
        ModelDims md;
        nnn_model_pack(*model, wqs[g], fpars[g], G.plan, md);
        delete own;
        G.tile0 = tile0;
        G.ntiles = (group_streams[g] + TILE - 1) / TILE;
        // rows per block: the most that fit the LDS; fewer (more, shorter blocks) while the launch cannot fill the GPU
        G.rows = 0;
        for (int rows = 32; rows >= 16 && !G.rows; rows /= 2)   // (64 rows never fit: the states stay in LDS for a whole group)
            if (rnn_lds_bytes(G.plan, rows) <= kLdsMax) G.rows = rows;
        if (!G.rows) return fail("model too large for the RNN kernel's LDS operand matrices");
        while (G.rows > 16 && G.ntiles * (TILE / G.rows) < RNN_SMALL_BATCH_BLOCKS) G.rows /= 2;
        if (paths.rnn_rows && rnn_lds_bytes(G.plan, paths.rnn_rows) <= kLdsMax) G.rows = paths.rnn_rows;
        G.rnn_lds = rnn_lds_bytes(G.plan, G.rows);
        // models of the built-in shape class run the layer-pipelined kernel (its fixed wave roles cover 2 / 2 / 3 / 6 neuron
        // blocks in the input dense / vad / noise / denoise layers)
        G.wp = rnn_wf_plan(G.plan);
        G.wf_lds = rnn_wf_lds_bytes(G.wp);
        // the fused back end / its RNN stretch alone: layers of up to 8 neuron blocks (two units per wave) whose operands fit the LDS
        // (compiled for the built-in model's shape class, nnn_back.hip; any other model takes the unfused kernels)
        {
            const bool shape_ok = bk_same_shape(G.plan, BkShapeBuiltin::plan());
            G.shape_builtin = shape_ok;
            const size_t fb = (size_t)back_lds(G.plan, true).total, rb = (size_t)back_lds(G.plan, false).total;
            G.back_lds = shape_ok && fb <= kLdsMax ? fb : 0;
            G.rnn16_lds = shape_ok && rb <= kLdsMax ? rb : 0;
            G.acts = BkActs{G.plan.dense.act, G.plan.vad.act, G.plan.noise.act, G.plan.dn.act, G.plan.out.act, G.plan.act_vo};
        }
        G.wf = !paths.rnn_rows && G.plan.dense.nb <= 2 && G.plan.vad.nb <= 2 && G.plan.noise.nb <= 3 && G.plan.dn.nb <= 6 && G.plan.vad.rec.ksteps <= WF_KS_REC &&
               G.plan.noise.rec.ksteps <= WF_KS_REC && G.plan.dn.rec.ksteps <= WF_KS_REC && G.wf_lds <= kLdsMax;   // (k_rnn_wf's wave roles)
        tile0 += G.ntiles;
        h->md.nd = md.nd > h->md.nd ? md.nd : h->md.nd;
        h->md.nv = md.nv > h->md.nv ? md.nv : h->md.nv;
        h->md.nn = md.nn > h->md.nn ? md.nn : h->md.nn;
        h->md.ndn = md.ndn > h->md.ndn ? md.ndn : h->md.ndn;
    }
    const ModelDims &md = h->md;
    h->plan.rnn = new uint8_t[n_groups]();

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
    if (int rc = grow(h, false, h->sp_tab, 2 * 64 * sizeof(StepParams), 64)) return rc;
    // tables
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
        static const int E[NB] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24, 28, 34, 40, 48, 60, 78, 100};
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
    for (int g = 0; g < n_groups; g++) {
        const uint16_t *dq = nullptr;
        HIPCHK(upload(h, &dq, wqs[g]));
        h->groups[g].wq = (const uint4 *)dq;
        HIPCHK(upload(h, &h->groups[g].fpar, fpars[g]));
    }
    {   // per-frame scratch (doubles as parity taps): every array holds nset sets back to back
        Buffers &q = h->b[0];
        // (the arrays only the parity taps fill, 4.1 KB per stream and set, wait for nnn_batch_set_taps(1))
#define NNN_F(name, len) HIPCHK(dalloc(h, &q.name, Sp * (size_t)(len) * h->nset, false));
        NNN_WORK_FIELDS(NNN_F)
#undef NNN_F
        for (int set = 1; set < h->nset; set++) h->b[set] = frame_view(h->b[0], set);
        h->state_bufs.push_back({(void *)q.pflag, Sp * h->nset * sizeof(int)});   // frame numbers restart with reset / load_state
    }
    // the RNN kernel's dynamic LDS limit is a per-device function attribute: raise it to the hardware's 160 KB once
    HIPCHK(hipFuncSetAttribute((const void *)k_rnn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
    HIPCHK(hipFuncSetAttribute((const void *)k_rnn_wf<WfShapeAny>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
    HIPCHK(hipFuncSetAttribute((const void *)k_rnn_wf<BkShapeBuiltin>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
    HIPCHK(hipFuncSetAttribute((const void *)k_back<true, BkShapeBuiltin>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
    HIPCHK(hipFuncSetAttribute((const void *)k_back<false, BkShapeBuiltin>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
    HIPCHK(hipFuncSetAttribute((const void *)k_back<true, BkShapeBuiltin, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
    HIPCHK(hipFuncSetAttribute((const void *)k_back<true, BkShapeBuiltin, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
    HIPCHK(hipFuncSetAttribute((const void *)k_back<false, BkShapeBuiltin, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
    HIPCHK(hipFuncSetAttribute((const void *)k_back<true, BkShapeBuiltin, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
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
    return 0;
}

// ---- state snapshots: DenoiseState is Clone in the reference (src/denoise.rs:36) ------------------------------------
struct SnapHeader { uint64_t magic, frame_count, group_count, n_bufs, total, streams; };
constexpr uint64_t kSnapMagic = 0x6e6e6e5f73743032ull;   // "nnn_st02"

extern "C" size_t nnn_batch_state_bytes(const nnn_batch *h)
{
    if (!h) return 0;
    size_t n = sizeof(SnapHeader);
    for (auto &sb : h->state_bufs) n += sb.second;
    return n;
}

extern "C" int nnn_batch_save_state(nnn_batch *h, void *host_dst, size_t dst_bytes)
{
    NNN_RT_LOCK;
    if (!h || !host_dst) return fail("null argument");
    const size_t need = nnn_batch_state_bytes(h);
    if (dst_bytes < need) return fail("state buffer too small: %zu bytes needed", need);
    if (h->n_held) return fail("nnn_batch_save_state refused: %d streams are held (nnn_batch_hold_streams) and the raw state image has no place for their parked records; resume or export them first", h->n_held);
    if (int rc = quiesce(h)) return rc;
    SnapHeader hd{kSnapMagic, h->frame_count, h->group_count, (uint64_t)h->state_bufs.size(), (uint64_t)need, (uint64_t)h->S};
    char *p = (char *)host_dst;
    memcpy(p, &hd, sizeof(hd));
    p += sizeof(hd);
    for (auto &sb : h->state_bufs) {
        HIPCHK(hipMemcpy(p, sb.first, sb.second, hipMemcpyDeviceToHost));
        p += sb.second;
    }
    return 0;
}

extern "C" int nnn_batch_load_state(nnn_batch *h, const void *host_src, size_t src_bytes)
{
    NNN_RT_LOCK;
    if (!h || !host_src) return fail("null argument");
    const size_t need = nnn_batch_state_bytes(h);
    SnapHeader hd;
    if (src_bytes < sizeof(hd)) return fail("not a state snapshot");
    memcpy(&hd, host_src, sizeof(hd));
    if (hd.magic != kSnapMagic || hd.n_bufs != h->state_bufs.size() || hd.total != need || hd.streams != (uint64_t)h->S || src_bytes < need)
        return fail("state snapshot does not match this batch (streams / models / max_group_frames / library build)");
    if (h->n_held) return fail("nnn_batch_load_state refused: %d streams are held (nnn_batch_hold_streams) and the raw state image has no place for their parked records; resume them or nnn_batch_reset first", h->n_held);
    if (int rc = quiesce(h)) return rc;
    const char *p = (const char *)host_src + sizeof(hd);
    for (auto &sb : h->state_bufs) {
        HIPCHK(hipMemcpy(sb.first, p, sb.second, hipMemcpyHostToDevice));
        p += sb.second;
    }
    HIPCHK(hipDeviceSynchronize());
    *h->fault_host = 0;
    h->frame_count = hd.frame_count;
    h->group_count = hd.group_count;
    h->prev_pipe = false;
    return 0;
}

extern "C" nnn_batch *nnn_batch_clone(nnn_batch *h)
{
    NNN_RT_LOCK;
    if (!h) { fail("null batch"); return nullptr; }
    if (quiesce(h)) return nullptr;
    std::vector<const RNNModel *> mp;
    for (const RNNModel &m : h->models) mp.push_back(&m);
    // made as the source was made (not from the environment of now: its depth, ring and kernel forms must match), then set as it is
    nnn_batch *c = create_batch(mp.data(), h->group_streams.data(), (int)h->group_streams.size(), h->device, h->gmax, h->created);
    if (!c) return nullptr;
    bool ok = c->state_bufs.size() == h->state_bufs.size();
    for (size_t i = 0; ok && i < h->state_bufs.size(); i++)
        ok = c->state_bufs[i].second == h->state_bufs[i].second &&
             hipMemcpy(c->state_bufs[i].first, h->state_bufs[i].first, h->state_bufs[i].second, hipMemcpyDeviceToDevice) == hipSuccess;
    if (!ok || hipDeviceSynchronize() != hipSuccess) {
        nnn_batch_destroy(c);
        fail("state copy failed");
        return nullptr;
    }
    if (h->n_held) {   // the same held set and parked records
        ok = hold_prepare(c) == 0 &&
             hipMemcpy(c->park, h->park, (size_t)h->S * NNN_STREAM_STATE_BYTES, hipMemcpyDeviceToDevice) == hipSuccess &&
             hipMemcpy(c->live, h->live, (size_t)h->NT * sizeof(unsigned long long), hipMemcpyDeviceToDevice) == hipSuccess &&
             hipDeviceSynchronize() == hipSuccess;
        if (!ok) {
            nnn_batch_destroy(c);
            fail("copy of the parked records failed");
            return nullptr;
        }
        c->held = h->held;
        c->n_held = h->n_held;
    }
    c->frame_count = h->frame_count;
    c->group_count = h->group_count;
    c->paths = h->paths;
    if (h->b[0].taps && nnn_batch_set_taps(c, h->b[0].taps) != 0) {
        nnn_batch_destroy(c);
        return nullptr;
    }
    return c;
}

// ---- per-stream state records (include/nnn_batch.h, NNN_STREAM_STATE_*) ---------------------------------------------------------
// A record is one stream's DenoiseState in the reference's terms.  Export reads the history ring through the batch's frame count
// (input_mem comes out oldest first).  Import writes input_mem into the ring slots the next frame reads (frame_count - 1 and the
// 1248 samples before it) and re-derives what the batch keeps beside the ring with the high-pass kernels' arithmetic (k_hp / k_hp2):
// the decimated values of the last three frames (and their mirror), x_lp[0] of the next frame's slot and the last filtered sample --
// the bits the batch itself would have made.  Nothing per-frame (lpc, lpc_head, the scratch sets, pflag) is touched: the next frame
// remakes it before reading it, and k_pitch takes the last pitch of a call's first frame from last_period / last_gain, which the record
// holds.  Records are handled as 32-bit words (bit copies; ints and floats alike).
#include "nnn_stream_state.hip"   // the record layout (SS_*), SsArgs and the k_ss_* kernels

static void ss_dims_host(const nnn_batch *h, int s, int d[3])
{
    for (const nnn_batch::ModelGroup &G : h->groups)
        if (s / TILE >= G.tile0 && s / TILE < G.tile0 + G.ntiles) {
            d[0] = G.plan.vad.n;
            d[1] = G.plan.noise.n;
            d[2] = G.plan.dn.n;
            return;
        }
    d[0] = d[1] = d[2] = -1;
}
enum SsOp { SS_RESET = 0, SS_EXPORT = 1, SS_IMPORT = 2, SS_HOLD = 3, SS_RESUME = 4 };
// Everything a call can check on the host, before it writes anything.  host_rec: an import's records in host memory (checked here),
// or nullptr.  Also used by the node (nnn_node.cpp) to check every shard's part of a list before any shard is written.
int nnn_batch_check_streams(const nnn_batch *h, int op, const int *streams, int n, const void *host_rec, size_t bytes, bool need_buf)
{
    if (!h) return fail("null batch");
    if (n < 0) return fail("negative stream count");
    if (n > 0 && !streams) return fail("null stream list");
    if (op == SS_EXPORT && nnn_batch_fault(h)) return fail("export refused: the batch is faulted (nnn_batch_fault); its state is invalid");
    if (op == SS_HOLD && nnn_batch_fault(h)) return fail("hold refused: the batch is faulted (nnn_batch_fault); its state is invalid");
    if (need_buf && n > 0 && !host_rec) return fail("null record buffer");
    if (need_buf && bytes < (size_t)n * NNN_STREAM_STATE_BYTES)
        return fail("record buffer too small: %zu bytes for %d records of %d", bytes, n, NNN_STREAM_STATE_BYTES);
    std::vector<char> seen(op == SS_EXPORT ? 0 : (size_t)h->S, 0);
    for (int i = 0; i < n; i++) {
        const int s = streams[i];
        if (s < 0 || s >= h->S) return fail("stream index %d (entry %d) outside [0, %d)", s, i, h->S);
        if (op != SS_EXPORT) {
            if (seen[(size_t)s]) return fail("stream %d listed twice", s);
            seen[(size_t)s] = 1;
        }
        const bool is_held = h->n_held > 0 && h->held[(size_t)s];
        if (op == SS_HOLD && is_held) return fail("stream %d (entry %d) is already held", s, i);
        if (op == SS_RESUME && !is_held) return fail("stream %d (entry %d) is not held", s, i);
    }
    if (op == SS_IMPORT && host_rec)
        for (int i = 0; i < n; i++) {
            uint32_t w[6];
            memcpy(w, (const char *)host_rec + (size_t)i * NNN_STREAM_STATE_BYTES, sizeof(w));
            if (w[0] != NNN_STREAM_STATE_MAGIC) return fail("record %d: not a stream state record (magic %08x)", i, w[0]);
            if (w[1] != NNN_STREAM_STATE_VERSION) return fail("record %d: version %u, this library reads version %d", i, w[1], NNN_STREAM_STATE_VERSION);
            if (w[2] != NNN_STREAM_STATE_BYTES) return fail("record %d: size %u, expected %d", i, w[2], NNN_STREAM_STATE_BYTES);
            int d[3];
            ss_dims_host(h, streams[i], d);
            if ((int)w[3] != d[0] || (int)w[4] != d[1] || (int)w[5] != d[2])
                return fail("record %d: GRU sizes %d/%d/%d, stream %d's model has %d/%d/%d", i, (int)w[3], (int)w[4], (int)w[5], streams[i], d[0], d[1], d[2]);
        }
    return 0;
}

// first use: the per-tile GRU sizes, the check flag, the mapped report word
static int ss_prepare(nnn_batch *h)
{
    HIPCHK(hipSetDevice(h->device));
    if (h->ss_dims) return 0;
    NNN_RT_LOCK;
    std::vector<int> dims((size_t)h->NT, 0);
    for (const nnn_batch::ModelGroup &G : h->groups)
        for (int t = G.tile0; t < G.tile0 + G.ntiles; t++) dims[(size_t)t] = G.plan.vad.n | G.plan.noise.n << 8 | G.plan.dn.n << 16;
    HIPCHK(hipMalloc((void **)&h->ss_flag, sizeof(int)));
    HIPCHK(hipMemset(h->ss_flag, 0, sizeof(int)));
    {
        void *hp = nullptr, *dp = nullptr;
        HIPCHK(hipHostMalloc(&hp, sizeof(int), hipHostMallocMapped));
        *(volatile int *)hp = 0;
        h->ss_bad_host = (volatile int *)hp;
        HIPCHK(hipHostGetDevicePointer(&dp, hp, 0));
        h->ss_bad_dev = (int *)dp;
    }
    HIPCHK(hipEventCreateWithFlags(&h->ev_ss_idx, hipEventDisableTiming));
    int *d = nullptr;
    HIPCHK(hipMalloc((void **)&d, dims.size() * sizeof(int)));
    HIPCHK(hipMemcpy(d, dims.data(), dims.size() * sizeof(int), hipMemcpyHostToDevice));
    h->ss_dims = d;
    return 0;
}
// Calls of a batch are ordered even when consecutive ones arrive on different streams (processing, state and hold calls alike):
// call_begin picks the call's stream and, if the batch's last call was made on another one, has it wait for that call's end (`e`: how
// that went); call_end makes this call the batch's last one.  A state or hold call also clears prev_pipe, which a pipelined call before
// it leaves set: the next call's high-pass must not start early (nnn_batch_set_inputs_ready) on rings this call writes -- what
// nnn_batch_load_state does.
static hipStream_t call_begin(nnn_batch *h, void *hip_stream, hipError_t &e)
{
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : h->stream;
    e = (h->have_last && h->last_stream != st) ? hipStreamWaitEvent(st, h->ev_last, 0) : hipSuccess;
    return st;
}
static hipError_t call_end(nnn_batch *h, hipStream_t st)
{
    const hipError_t e = hipEventRecord(h->ev_last, st);
    h->last_stream = st;
    h->have_last = true;
    return e;
}
static int ss_args(nnn_batch *h, const int *streams, int n, hipStream_t st, SsArgs &a, bool &tiles)
{
    memset(&a, 0, sizeof(a));
    a.dims = h->ss_dims;
    a.n = n;
    a.first = streams[0];
    bool run = true;
    for (int i = 1; i < n && run; i++) run = streams[i] == streams[0] + i;
    tiles = run && n >= TILE;
    if (run) a.mode = 0;
    else if (n <= SS_SMALL) {
        a.mode = 1;
        for (int i = 0; i < n; i++) a.small[i] = streams[i];
    } else {
        a.mode = 2;
        if ((size_t)n > h->ss_idx.cap) {   // (drained first: the old list may still be read)
            if (int rc = grow(h, true, h->ss_idx, (size_t)n * sizeof(int), (size_t)n, &h->ss_idx_pin, (size_t)n * sizeof(int))) return rc;
            h->ss_idx_busy = false;
        }
        if (h->ss_idx_busy) HIPCHK(hipEventSynchronize(h->ev_ss_idx));   // the page-locked list of the previous call has been copied
        memcpy(h->ss_idx_pin.p, streams, (size_t)n * sizeof(int));
        HIPCHK(hipMemcpyAsync(h->ss_idx.p, h->ss_idx_pin.p, (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
        HIPCHK(hipEventRecord(h->ev_ss_idx, st));
        h->ss_idx_busy = true;
        a.idx = h->ss_idx.p;
    }
    const int nslot = h->nslot, N = (int)(h->frame_count % (uint64_t)nslot);
    a.rb_in = ring_base((N + nslot - 1) % nslot, nslot);
    a.dec_row0 = 240 * ((N + nslot - 3) % nslot);
    a.slot_next = N;
    return 0;
}
static void ss_launch(nnn_batch *h, bool to_records, const SsArgs &a, bool tiles, const void *src, void *dst, hipStream_t st)
{
    const Buffers &b = h->b[0];
    const unsigned grid = tiles ? (unsigned)((a.first + a.n - 1) / TILE - a.first / TILE + 1) : (unsigned)a.n;
    if (to_records) {
        if (tiles) hipLaunchKernelGGL(k_ss_export_tiles, dim3(grid), dim3(256), 0, st, b, a, (unsigned *)dst);
        else hipLaunchKernelGGL(k_ss_export_streams, dim3(grid), dim3(256), 0, st, b, a, (unsigned *)dst);
    } else {
        if (tiles) hipLaunchKernelGGL(k_ss_import_tiles, dim3(grid), dim3(256), 0, st, b, a, (const unsigned *)src);
        else hipLaunchKernelGGL(k_ss_import_streams, dim3(grid), dim3(256), 0, st, b, a, (const unsigned *)src);
    }
}
// one state call: checks, ordering, list, kernels (to_records: export), optional copies of the host variants
static int ss_call(nnn_batch *h, SsOp op, const int *streams, int n, const void *host_src, void *host_dst, const void *d_src, void *d_dst,
                   void *hip_stream, bool device_check)
{
    if (n == 0) return 0;
    if (int rc = ss_prepare(h)) return rc;
    const size_t bytes = (size_t)n * NNN_STREAM_STATE_BYTES;
    if ((host_src || host_dst) && bytes > h->ss_stage.cap && grow(h, false, h->ss_stage, bytes, bytes)) return 1;   // (no drain: host variants wait for their work)
    hipError_t e;
    hipStream_t st = call_begin(h, hip_stream, e);
    if (e != hipSuccess) return fail("could not order the call after the batch's earlier work: %s", hipGetErrorString(hipGetLastError()));
    SsArgs a;
    bool tiles = false;
    if (int rc = ss_args(h, streams, n, st, a, tiles)) return rc;
    if (host_src) {
        HIPCHK(hipMemcpyAsync(h->ss_stage.p, host_src, bytes, hipMemcpyHostToDevice, st));
        d_src = h->ss_stage.p;
    }
    if (device_check) {
        HIPCHK(hipMemsetAsync(h->ss_flag, 0, sizeof(int), st));
        hipLaunchKernelGGL(k_ss_check, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, (const unsigned *)d_src, h->ss_flag, h->ss_bad_dev);
        a.flag = h->ss_flag;
    }
    if (op == SS_EXPORT) ss_launch(h, true, a, tiles, nullptr, host_dst ? (void *)h->ss_stage.p : d_dst, st);
    else ss_launch(h, false, a, tiles, op == SS_RESET ? nullptr : d_src, nullptr, st);
    bool any_held = false;
    for (int i = 0; i < n && h->n_held > 0 && !any_held; i++) any_held = h->held[(size_t)streams[i]] != 0;
    if (any_held)
        hipLaunchKernelGGL(k_ss_parked, dim3((unsigned)n), dim3(256), 0, st, a, (const unsigned long long *)h->live, h->park, op == SS_EXPORT ? 1 : 0,
                           (unsigned *)(host_dst ? (void *)h->ss_stage.p : d_dst), (const unsigned *)(op == SS_IMPORT ? d_src : nullptr));
    if (host_dst) HIPCHK(hipMemcpyAsync(host_dst, h->ss_stage.p, bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipGetLastError());
    HIPCHK(call_end(h, st));
    h->prev_pipe = false;
    if (host_src || host_dst) HIPCHK(hipStreamSynchronize(st));
    return 0;
}

extern "C" int nnn_batch_reset_streams(nnn_batch *h, const int *streams, int n)
{
    if (int rc = nnn_batch_check_streams(h, SS_RESET, streams, n, nullptr, 0, false)) return rc;
    return ss_call(h, SS_RESET, streams, n, nullptr, nullptr, nullptr, nullptr, nullptr, false);
}
extern "C" int nnn_batch_export_streams(nnn_batch *h, const int *streams, int n, void *host_dst, size_t dst_bytes)
{
    if (int rc = nnn_batch_check_streams(h, SS_EXPORT, streams, n, host_dst, dst_bytes, true)) return rc;
    return ss_call(h, SS_EXPORT, streams, n, nullptr, host_dst, nullptr, nullptr, nullptr, false);
}
extern "C" int nnn_batch_import_streams(nnn_batch *h, const int *streams, int n, const void *host_src, size_t src_bytes)
{
    if (int rc = nnn_batch_check_streams(h, SS_IMPORT, streams, n, host_src, src_bytes, true)) return rc;
    return ss_call(h, SS_IMPORT, streams, n, host_src, nullptr, nullptr, nullptr, nullptr, false);
}
extern "C" int nnn_batch_export_streams_device(nnn_batch *h, const int *streams, int n, void *d_dst, void *hip_stream)
{
    if (int rc = nnn_batch_check_streams(h, SS_EXPORT, streams, n, nullptr, 0, false)) return rc;
    if (n > 0 && (!d_dst || ((uintptr_t)d_dst & 3))) return fail("null or unaligned record buffer");
    return ss_call(h, SS_EXPORT, streams, n, nullptr, nullptr, nullptr, d_dst, hip_stream, false);
}
extern "C" int nnn_batch_import_streams_device(nnn_batch *h, const int *streams, int n, const void *d_src, void *hip_stream)
{
    if (int rc = nnn_batch_check_streams(h, SS_IMPORT, streams, n, nullptr, 0, false)) return rc;
    if (n > 0 && (!d_src || ((uintptr_t)d_src & 3))) return fail("null or unaligned record buffer");
    return ss_call(h, SS_IMPORT, streams, n, nullptr, nullptr, d_src, nullptr, hip_stream, true);
}

// ---- hold and resume (include/nnn_batch.h) ---------------------------------------------------------------------
// Hold = the export above into the batch's own parked records, resume = the import from them (which re-phases the history into the ring
// slots the frame counter of NOW reads); the same launch flips the streams' bits of the live mask the processing kernels look at.
static std::vector<unsigned long long> live_all(const nnn_batch *h)
{
    std::vector<unsigned long long> w((size_t)h->NT, ~0ull);
    if (h->S % TILE) w.back() = (1ull << (h->S % TILE)) - 1ull;   // (padding streams are never live)
    return w;
}
static int hold_prepare(nnn_batch *h)
{
    if (h->park) return 0;
    NNN_RT_LOCK;
    if (int rc = quiesce(h)) return rc;
    unsigned *park = nullptr;
    unsigned long long *live = nullptr;
    HIPCHK(dalloc(h, &park, (size_t)h->S * SS_WORDS, false));
    HIPCHK(dalloc(h, &live, (size_t)h->NT, false));
    const std::vector<unsigned long long> w = live_all(h);
    HIPCHK(hipMemcpy(live, w.data(), w.size() * sizeof(w[0]), hipMemcpyHostToDevice));
    HIPCHK(hipDeviceSynchronize());
    h->park = park;
    h->live = live;
    h->held.assign((size_t)h->S, 0);
    h->n_held = 0;
    for (int set = 0; set < NSET; set++) h->b[set].live = live;   // (every argument block, the ones a later nnn_batch_set_taps re-derives included)
    return 0;
}
static int hold_call(nnn_batch *h, bool hold, const int *streams, int n)
{
    if (int rc = nnn_batch_check_streams(h, hold ? SS_HOLD : SS_RESUME, streams, n, nullptr, 0, false)) return rc;
    // (the first hold of a batch allocates the parked records and the mask, which waits for the device: a host that cannot stall at its
    // first mute makes an empty hold -- n = 0 -- when it creates the batch)
    if (n == 0 && !hold) return 0;
    if (int rc = ss_prepare(h)) return rc;
    if (int rc = hold_prepare(h)) return rc;
    if (n == 0) return 0;
    hipError_t e;
    hipStream_t st = call_begin(h, nullptr, e);
    if (e != hipSuccess) return fail("could not order the call after the batch's earlier work: %s", hipGetErrorString(hipGetLastError()));
    SsArgs a;
    bool tiles = false;
    if (int rc = ss_args(h, streams, n, st, a, tiles)) return rc;
    a.by_stream = 1;
    a.live_op = hold ? 1 : 2;
    a.live = h->live;
    unsigned *rec0 = h->park + (tiles ? (size_t)a.first * SS_WORDS : 0);   // (the tile kernels count records from the list's first stream)
    ss_launch(h, hold, a, tiles, rec0, rec0, st);
    // (the launch is enqueued and will flip the device's bits: the host's copy follows it whatever the bookkeeping below reports)
    for (int i = 0; i < n; i++) h->held[(size_t)streams[i]] = hold ? 1 : 0;
    h->n_held += hold ? n : -n;
    HIPCHK(hipGetLastError());
    HIPCHK(call_end(h, st));
    h->prev_pipe = false;
    return 0;
}
extern "C" int nnn_batch_hold_streams(nnn_batch *h, const int *streams, int n) { return hold_call(h, true, streams, n); }
extern "C" int nnn_batch_resume_streams(nnn_batch *h, const int *streams, int n) { return hold_call(h, false, streams, n); }
extern "C" int nnn_batch_num_held(const nnn_batch *h) { return h ? h->n_held : 0; }
extern "C" int nnn_batch_held_mask(const nnn_batch *h, uint8_t *held, size_t n)
{
    if (!h || !held) return fail("null argument");
    if (n < (size_t)h->S) return fail("mask buffer too small: %d entries needed", h->S);
    for (int s = 0; s < h->S; s++) held[s] = h->n_held > 0 ? h->held[(size_t)s] : 0;
    return 0;
}
// nnn_batch_reset: every stream takes part again
static int hold_release_all(nnn_batch *h)
{
    if (!h->live) return 0;
    const std::vector<unsigned long long> w = live_all(h);
    HIPCHK(hipMemcpy(h->live, w.data(), w.size() * sizeof(w[0]), hipMemcpyHostToDevice));
    h->held.assign((size_t)h->S, 0);
    h->n_held = 0;
    return 0;
}

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

// stage `s` of the group planned in p, in scratch sets set0 .. set0 + p.g - 1, parameters at sp0[0..g), on stream `st`.
// plain_out: the parameter table sp0 points into was filled for f32 mono audio (k_synth's plain-format instantiation ignores the table's
// fmt / channels, so the caller states the format of the very call that fills the table, not a field of the batch)
static void launch_stage(nnn_batch *h, int s, int set0, const GroupPlan &p, const StepParams *sp0, hipStream_t st, bool prof, bool plain_out, const StepParams *call = nullptr, int fill = 0)
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
            for (const nnn_batch::ModelGroup &G : h->groups) {
                if (p.riders)   // (its X transform done by k_pitch's rider blocks, see xt_rider)
                    L.go(K_BACK, p.held ? k_back<true, BkShapeBuiltin, true, true> : k_back<true, BkShapeBuiltin, true, false>, dim3((unsigned)(G.ntiles * (TILE / BK_ROWS))), dim3(BK_T), G.back_lds, b, sp0, G.acts, G.wq, G.fpar, G.tile0, g);
                else
                    L.go(K_BACK, p.held ? k_back<true, BkShapeBuiltin, false, true> : k_back<true, BkShapeBuiltin, false, false>, dim3((unsigned)(G.ntiles * (TILE / BK_ROWS))), dim3(BK_T), G.back_lds, b, sp0, G.acts, G.wq, G.fpar, G.tile0, g);
            }
            break;
        }
        L.go(K_FFT_XP, k_fft_xp, dim3(Sp * ug / FFT_SPB), dim3(64 * FFT_SPB), 0, b, sp0, g);
        break;
    case ST_RNN:
        if (p.back == BACK_FUSED) break;
        for (size_t i = 0; i < h->groups.size(); i++) {   // one launch per resident model (a run of whole tiles)
            const nnn_batch::ModelGroup &G = h->groups[i];
            if (p.rnn[i] == RK_BACK)
                L.go(K_RNN, p.held ? k_back<false, BkShapeBuiltin, false, true> : k_back<false, BkShapeBuiltin, false, false>, dim3((unsigned)(G.ntiles * (TILE / BK_ROWS))), dim3(BK_T), G.rnn16_lds, b, sp0, G.acts, G.wq, G.fpar, G.tile0, g);
            else if (p.rnn[i] == RK_WF_BUILTIN)
                L.go(K_RNN, k_rnn_wf<BkShapeBuiltin>, dim3((unsigned)(G.ntiles * (TILE / WF_ROWS))), dim3(64 * WF_WAVES), G.wf_lds, b, G.plan, G.wp,
                     G.wq, G.fpar, G.tile0, g);
            else if (p.rnn[i] == RK_WF_ANY)
                L.go(K_RNN, k_rnn_wf<WfShapeAny>, dim3((unsigned)(G.ntiles * (TILE / WF_ROWS))), dim3(64 * WF_WAVES), G.wf_lds, b, G.plan, G.wp,
                     G.wq, G.fpar, G.tile0, g);
            else
                L.go(K_RNN, k_rnn, dim3((unsigned)(G.ntiles * (TILE / G.rows))), dim3(64 * RNN_WAVES), G.rnn_lds, b, G.plan, G.wq, G.fpar,
                     G.tile0, G.rows, g);
        }
        break;
    case ST_SYN:
        if (p.back == BACK_FUSED) break;
        if (plain_out) L.go(K_SYNTH, k_synth<true>, dim3(Sp / FFT_SPB), dim3(64 * FFT_SPB), 0, b, sp0, g);
        else L.go(K_SYNTH, k_synth<false>, dim3(Sp / FFT_SPB), dim3(64 * FFT_SPB), 0, b, sp0, g);
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

constexpr size_t ZC_MAX = (size_t)1 << 20;                 // host-buffer calls up to this many bytes run on mapped host memory (plan_host_call)
constexpr size_t HOST_CHUNK_MIN_BYTES = (size_t)1 << 20;   // a chunk of a host-buffer call is at least this long
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

// How a host-buffer call crosses the bus (plan_host_call, which reads the batch only; process_host_span runs it,
// nnn_batch_debug_host_plan shows it to the tests)
enum HostRoute { HOST_ZERO_COPY = 0, HOST_ONE_PIECE = 1, HOST_CHUNKED = 2 };
struct HostPlan {
    int route;
    int chunk, n_chunks;   // frames per chunk and chunks (one chunk of n_frames unless HOST_CHUNKED)
    size_t span;           // bytes of the bounding span of the (possibly strided) layout: what is shipped
    size_t vbytes;         // bytes of the VAD rows, 0 = not asked for
    size_t vofs;           // where the VAD rows sit behind the span in a host image of both (zero-copy; one piece with vad_masked)
    int drop;              // 1 = the first frame produces no audio (discard_first on a fresh batch)
    bool vad_masked;       // one piece: the VAD rows come back through the host image too, a held stream's entries are not copied
};
static HostPlan plan_host_call(const nnn_batch *h, int n_frames, const nnn_pcm_layout &L, bool has_vad)
{
    const size_t e = (size_t)pcm_elem_bytes(L.format), groups = (size_t)(h->S / L.channels), fr = (size_t)FRAME * L.channels * e;
    HostPlan p;
    p.route = HOST_ZERO_COPY, p.chunk = n_frames, p.n_chunks = 1;   // (until the rules below say otherwise)
    p.span = (groups - 1) * L.group_stride * e + (size_t)(n_frames - 1) * L.frame_stride * e + fr;
    p.vbytes = has_vad ? (size_t)n_frames * h->S * sizeof(float) : 0;
    p.vofs = (p.span + 15) / 16 * 16;
    p.drop = (L.discard_first && h->frame_count == 0) ? 1 : 0;
    p.vad_masked = has_vad && h->n_held > 0;
    // Small calls -- the RNNoise C ABI's state is a batch of one, a frame per call -- have nothing to overlap and pay for every runtime call they
    // make: two or three staged copies of a few kilobytes cost more than the three kernels between them.  Up to ZC_MAX bytes the kernels work on
    // page-locked host memory directly (the input read over the link by the first kernel, audio and VAD written over it by the last): one
    // memcpy in, one wait, one memcpy out.  Same kernels, same bits.  An explicit NNN_HOST_CHUNK always takes the staged routes.
    if (h->paths.host_chunk < 0 && p.span + p.vbytes + 16 <= ZC_MAX) return p;
    // Chunk length.  The first upload and the last download are not overlapped, so a call wants many chunks (about sixteen); the kernels
    // want groups of a few frames on small batches (a 4096-stream batch runs 4-frame groups at 0.8 of its 24-frame rate, a 65 536-stream
    // batch is within 15 % of its best on one-frame groups -- and still twice as fast as the bus).  Measured with page-locked buffers
    // against the link's own both-ways peak of 97 GB/s (profiles/r5_host_boundary.txt): 4096 streams x 48 frames f32 at 4 / 8 / 16-frame
    // chunks 84 / 79 / 69 GB/s both ways (round 4 used 8), 65 536 x 24 at 1 / 2 / 4 / 8: 90 / 87 / 81 / 71 (int16: 81 / 84 / 77 / 66).
    // Chunks under a megabyte are not worth their launches.
    int chunk = h->paths.host_chunk;
    if (chunk < 0) {
        constexpr int HC = 16;   // longest chunk
        chunk = n_frames / 16;
        if (chunk < 1) chunk = 1;
        if (h->S_pad <= 8192 && chunk < 4) chunk = 4;
        if (chunk > HC) chunk = HC;
        while (chunk < HC && (size_t)chunk * fr * groups < HOST_CHUNK_MIN_BYTES) chunk *= 2;
        if ((size_t)chunk * fr * groups < HOST_CHUNK_MIN_BYTES) chunk = 0;
    }
    // (the chunks' downloads go straight into the caller's buffers, whole rows of every stream: with streams held the call takes the
    // one-piece route, whose copy back leaves out what a held stream owns)
    const bool chunked = chunk > 0 && n_frames > chunk && L.frame_stride == (size_t)FRAME * L.channels && !h->n_held;
    p.route = chunked ? HOST_CHUNKED : HOST_ONE_PIECE;
    if (chunked) p.chunk = chunk, p.n_chunks = (n_frames + chunk - 1) / chunk;
    return p;
}
// The training host call's chunk length (nnn_train_process_host): 16 frames (tuned on the bus, not tied to the kernels' group length) for
// calls of more than two such chunks that are worth their launches, otherwise one piece; NNN_HOST_CHUNK (tests) overrides it.
static int plan_train_chunk(const nnn_batch *h, int n_frames)
{
    constexpr int HC = 16;
    if (const int hc = h->paths.host_chunk; hc >= 0) return hc > 0 && hc < n_frames ? hc : n_frames;
    return n_frames > 2 * HC && (size_t)h->S * HC * FRAME * 4 >= HOST_CHUNK_MIN_BYTES ? HC : n_frames;
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
    if (n_frames <= 0) return 0;
    if (!d_in || !d_out) return fail("null buffer");
    if (int rc = check_layout(h, L)) return rc;
    const long long e = pcm_elem_bytes(L->format);
    const int drop = (L->discard_first && h->frame_count == 0) ? 1 : 0;
    return process_frames(h, d_in, d_out, d_vad, n_frames, L->format, L->channels, (long long)L->group_stride * e,
                          (long long)L->frame_stride * e, drop, hip_stream);
}

// Chunked host calls (the denoiser's and the training rows'): chunk i + 1 crosses the bus on one copy stream while chunk i is processed on
// the batch's stream and chunk i - 1 returns on another (PCIe is full duplex).  upload(t0, n) enqueues n frames from t0 on copy_in,
// run(t0, n) processes them on h->stream, download(t0, n) enqueues what comes back on copy_out.  Nothing more is enqueued after the
// first error; all three streams are drained either way.  The copy streams and an event pair per chunk are made on first use.
template <class Up, class Run, class Down> static int pump_chunks(nnn_batch *h, int n_frames, int C, Up upload, Run run, Down download)
{
    const int nch = (n_frames + C - 1) / C;
    if (!h->copy_in || (int)h->ev_up.size() < nch) {
        NNN_RT_LOCK;
        if (!h->copy_in) {
            HIPCHK(hipStreamCreateWithFlags(&h->copy_in, hipStreamNonBlocking));
            HIPCHK(hipStreamCreateWithFlags(&h->copy_out, hipStreamNonBlocking));
        }
        while ((int)h->ev_up.size() < nch) {
            hipEvent_t a, b;
            HIPCHK(hipEventCreateWithFlags(&a, hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&b, hipEventDisableTiming));
            h->ev_up.push_back(a);
            h->ev_run.push_back(b);
        }
    }
    // (the previous call ended with every stream drained, so the staging is free)
    int rc = 0;
    hipError_t err = hipSuccess;
    for (int i = 0; i < nch && !rc && err == hipSuccess; i++) {
        const int t0 = i * C, n = t0 + C < n_frames ? C : n_frames - t0;
        err = upload(t0, n);
        if (err == hipSuccess) err = hipEventRecord(h->ev_up[i], h->copy_in);
        if (err == hipSuccess) err = hipStreamWaitEvent(h->stream, h->ev_up[i], 0);
        if (err != hipSuccess) break;
        rc = run(t0, n);
        if (rc) break;
        err = hipEventRecord(h->ev_run[i], h->stream);
        if (err == hipSuccess) err = hipStreamWaitEvent(h->copy_out, h->ev_run[i], 0);
        if (err == hipSuccess) err = download(t0, n);
    }
    const hipError_t e1 = hipStreamSynchronize(h->copy_in), e2 = hipStreamSynchronize(h->stream), e3 = hipStreamSynchronize(h->copy_out);
    if (rc) return rc;
    if (err == hipSuccess) err = e1 != hipSuccess ? e1 : (e2 != hipSuccess ? e2 : e3);
    if (err != hipSuccess) return fail("host transfer failed: %s", hipGetErrorString(err));
    return 0;
}

// A long host-buffer call with gap-free frames runs in chunks of p.chunk frames, every transfer a 2-D copy of groups x chunk-bytes
// straight between the caller's buffers and the device staging (DMA when they are page-locked -- nnn_host_alloc -- and staged by the
// runtime when not).  The device staging has the layout of the host buffers.
static int process_host_chunked(nnn_batch *h, const char *in, char *out, float *vad, int n_frames, const nnn_pcm_layout *L, const HostPlan &p)
{
    const size_t e = (size_t)pcm_elem_bytes(L->format), groups = (size_t)(h->S / L->channels), fr = (size_t)FRAME * L->channels * e;
    const size_t pitch = groups > 1 ? L->group_stride * e : (size_t)n_frames * fr, S = (size_t)h->S;
    char *const d = h->stage.p;
    float *const dv = vad ? h->stage_vad.p : nullptr;
    // with a dropped first frame every output sits one frame earlier than its input: a chunk of frames t0 .. t0 + n - 1 then writes frames
    // t0 - 1 .. t0 + n - 2, in place behind inputs that the chunk before has consumed (same stream), and returns those
    auto out0 = [&](int t0) { return (size_t)(t0 ? t0 - p.drop : 0); };
    const int rc = pump_chunks(h, n_frames, p.chunk,
        [&](int t0, int n) { return hipMemcpy2DAsync(d + t0 * fr, pitch, in + t0 * fr, pitch, n * fr, groups, hipMemcpyHostToDevice, h->copy_in); },
        [&](int t0, int n) { return nnn_batch_process_pcm_device(h, d + t0 * fr, d + out0(t0) * fr, dv ? dv + t0 * S : nullptr, n, L, h->stream); },
        [&](int t0, int n) {
            const size_t o0 = out0(t0), o1 = (size_t)(t0 + n - p.drop);
            hipError_t err = hipSuccess;
            if (o1 > o0) err = hipMemcpy2DAsync(out + o0 * fr, pitch, d + o0 * fr, pitch, (o1 - o0) * fr, groups, hipMemcpyDeviceToHost, h->copy_out);
            if (err == hipSuccess && vad) err = hipMemcpyAsync(vad + t0 * S, dv + t0 * S, n * S * sizeof(float), hipMemcpyDeviceToHost, h->copy_out);
            return err;
        });
    return rc ? rc : nnn_batch_synchronize(h);   // (also reports a frame hand-off that never arrived)
}

// The copies back of the host-buffer calls: the frames the call wrote, from a host image `src` of the device buffer into the caller's.
// A held stream's samples and VAD entries are not the call's to write (nnn_batch_hold_streams): the caller's bytes stay as they were,
// per channel where held and live channels share an interleaved group.
static void host_frames_back(const nnn_batch *h, char *out, const char *src, const nnn_pcm_layout *L, int n_out)
{
    const size_t e = (size_t)pcm_elem_bytes(L->format), ch = (size_t)L->channels, groups = (size_t)h->S / ch, fr = (size_t)FRAME * ch * e;
    for (size_t g = 0; g < groups; g++) {
        size_t n_live = ch;
        for (size_t c = 0; c < ch && h->n_held > 0; c++) n_live -= h->held[g * ch + c] ? 1 : 0;
        if (!n_live) continue;
        for (int t = 0; t < n_out; t++) {
            const size_t o = g * L->group_stride * e + (size_t)t * L->frame_stride * e;
            if (n_live == ch) { memcpy(out + o, src + o, fr); continue; }
            for (size_t c = 0; c < ch; c++)
                if (!h->held[g * ch + c])
                    for (size_t i = 0; i < (size_t)FRAME; i++) memcpy(out + o + (i * ch + c) * e, src + o + (i * ch + c) * e, e);
        }
    }
}
static void host_vad_back(const nnn_batch *h, float *vad, const float *src, int n_frames)
{
    if (!h->n_held) { memcpy(vad, src, (size_t)n_frames * h->S * sizeof(float)); return; }
    for (int t = 0; t < n_frames; t++)
        for (int s = 0; s < h->S; s++)
            if (!h->held[(size_t)s]) vad[(size_t)t * h->S + s] = src[(size_t)t * h->S + s];
}

// Host buffers: ship the bounding span of the (possibly strided) layout, run, bring the written frames back, by plan_host_call's route.
static int process_host_span(nnn_batch *h, const void *in, void *out, float *vad, int n_frames, const nnn_pcm_layout *L)
{
    struct InHostCall {   // (nnn_batch::host_call, until the call returns)
        nnn_batch *h;
        ~InHostCall() { h->host_call = false; }
    } in_host_call{h};
    h->host_call = true;
    HIPCHK(hipSetDevice(h->device));
    const HostPlan p = plan_host_call(h, n_frames, *L, vad != nullptr);
    if (p.route == HOST_ZERO_COPY) {
        if (!h->zc_dev) {   // (first use, or an earlier one that failed half-way: zc_dev is set last, and is what says that both exist)
            NNN_RT_LOCK;
            if (int rc = grow(h, true, h->zc_host, ZC_MAX, ZC_MAX)) return rc;
            HIPCHK(hipHostGetDevicePointer((void **)&h->zc_dev, h->zc_host.p, 0));
        }
        memcpy(h->zc_host.p, in, p.span);
        int rc = nnn_batch_process_pcm_device(h, h->zc_dev, h->zc_dev, vad ? (float *)(h->zc_dev + p.vofs) : nullptr, n_frames, L, h->stream);
        if (!rc) rc = nnn_batch_synchronize(h);   // (also reports a frame hand-off that never arrived)
        else hipStreamSynchronize(h->stream);
        if (!rc) {
            host_frames_back(h, (char *)out, h->zc_host.p, L, n_frames - p.drop);
            if (vad) host_vad_back(h, vad, (const float *)(h->zc_host.p + p.vofs), n_frames);
        }
        return rc;
    }
    if (p.span > h->stage.cap || p.vbytes > h->stage_vad.cap) {   // the staging grows by half as much again as is asked for (the VAD rows: twice)
        NNN_RT_LOCK;   // (one lock and one drain for both)
        if (int rc = quiesce(h)) return rc;
        if (p.span > h->stage.cap && grow(h, false, h->stage, p.span + p.span / 2, p.span + p.span / 2)) return 1;
        if (p.vbytes > h->stage_vad.cap && grow(h, false, h->stage_vad, 2 * p.vbytes, 2 * p.vbytes)) return 1;
    }
    if (p.route == HOST_CHUNKED) return process_host_chunked(h, (const char *)in, (char *)out, vad, n_frames, L, p);
    char *d = h->stage.p;
    float *dv = vad ? h->stage_vad.p : nullptr;
    hipError_t err = hipMemcpyAsync(d, in, p.span, hipMemcpyHostToDevice, h->stream);
    int rc = 0;
    if (err != hipSuccess) rc = fail("host staging failed: %s", hipGetErrorString(err));
    if (!rc) rc = nnn_batch_process_pcm_device(h, d, d, dv, n_frames, L, h->stream);
    if (!rc) {
        // `out` may alias `in` and may be strided: bring the span back and copy only real frames
        std::vector<char> &tmp = h->stage_host;
        const size_t image = p.vofs + (p.vad_masked ? p.vbytes : 0);
        if (tmp.size() < image) tmp.resize(image);
        err = hipMemcpyAsync(tmp.data(), d, p.span, hipMemcpyDeviceToHost, h->stream);
        if (err == hipSuccess && vad) err = hipMemcpyAsync(p.vad_masked ? (void *)(tmp.data() + p.vofs) : (void *)vad, dv, p.vbytes, hipMemcpyDeviceToHost, h->stream);
        if (err == hipSuccess) err = hipStreamSynchronize(h->stream);
        if (err == hipSuccess) {
            host_frames_back(h, (char *)out, tmp.data(), L, n_frames - p.drop);
            if (p.vad_masked) host_vad_back(h, vad, (const float *)(tmp.data() + p.vofs), n_frames);
        }
        if (err != hipSuccess) rc = fail("copy back failed: %s", hipGetErrorString(err));
        if (!rc) rc = nnn_batch_synchronize(h);   // (also reports a frame hand-off that never arrived)
    } else {
        hipStreamSynchronize(h->stream);
    }
    return rc;
}

extern "C" int nnn_batch_process_host(nnn_batch *h, const float *in, float *out, float *vad, int n_frames,
                                      size_t stream_stride, size_t frame_stride)
{
    if (!h) return fail("null batch");
    if (n_frames <= 0) return 0;
    if (!in || !out) return fail("null buffer");
    if (n_frames > 1 && frame_stride < (size_t)FRAME) return fail("frame_stride smaller than one frame");
    nnn_pcm_layout L = {NNN_PCM_F32, 1, 0, 0, stream_stride, frame_stride};
    return process_host_span(h, in, out, vad, n_frames, &L);
}

extern "C" int nnn_batch_process_pcm_host(nnn_batch *h, const void *in, void *out, float *vad, int n_frames,
                                          const nnn_pcm_layout *L)
{
    if (!h) return fail("null batch");
    if (n_frames <= 0) return 0;
    if (!in || !out) return fail("null buffer");
    if (int rc = check_layout(h, L)) return rc;
    return process_host_span(h, in, out, vad, n_frames, L);
}

// ---- taps ---------------------------------------------------------------------------------------
struct TapDesc { int len; int is_int; int layout; /* 0 TI, 2 / 4 SM spectrum rows of FSTR (X / P order), 3 hist ring */ int sub_ofs; int sub_len; int needs_taps; };
static int last_slot(const nnn_batch *h) { return h ? (int)((h->frame_count + h->nslot - 1) % h->nslot) : 0; }   // ring slot of the most recent frame
static bool tap_desc(const nnn_batch *h, int tap, TapDesc &d, const void **ptr)
{
    const Buffers *b = h ? &h->b[h->last_set] : nullptr;   // scratch set of the most recent frame
#define TP(field) (b ? (const void *)b->field : nullptr)
    switch (tap) {
    case NNN_TAP_FILTERED: d = {FRAME, 0, 3, 0, FRAME, 0}; *ptr = TP(hist); return true;
    case NNN_TAP_XLP: d = {XLP, 0, 0, 0, XLP, 1}; *ptr = TP(xlp_ti); return true;
    case NNN_TAP_AC: d = {5, 0, 0, last_slot(h) * 10, (h ? h->nslot : 0) * 10, 0}; *ptr = TP(lpc); return true;
    case NNN_TAP_LPC2: d = {5, 0, 0, last_slot(h) * 10 + 5, (h ? h->nslot : 0) * 10, 0}; *ptr = TP(lpc); return true;
    case NNN_TAP_XCORR1: d = {NLAG1, 0, 0, 0, NLAG1, 1}; *ptr = TP(xc1); return true;
    case NNN_TAP_BEST1: d = {2, 1, 0, 0, 2, 1}; *ptr = TP(best1); return true;
    case NNN_TAP_XCORR2C: d = {10, 0, 0, 0, 10, 1}; *ptr = TP(xc2); return true;
    case NNN_TAP_PITCH_SEARCH: d = {1, 1, 0, 0, 1, 1}; *ptr = TP(psearch); return true;
    case NNN_TAP_PITCH: d = {1, 1, 0, 0, 1, 0}; *ptr = TP(pitch); return true;
    case NNN_TAP_PITCH_GAIN: d = {1, 0, 0, 0, 1, 0}; *ptr = TP(pgain); return true;
    case NNN_TAP_X: d = {2 * FREQ, 0, 2, 0, 2 * FREQ, 1}; *ptr = TP(X); return true;   // (the fused back end keeps both spectra in registers)
    case NNN_TAP_P: d = {2 * FREQ, 0, 4, 0, 2 * FREQ, 1}; *ptr = TP(P); return true;   // (layout 4: spectrum_index_p)
    case NNN_TAP_EX: d = {NB, 0, 0, 0, NB, 0}; *ptr = TP(ex); return true;
    case NNN_TAP_EP: d = {NB, 0, 0, 0, NB, 0}; *ptr = TP(ep); return true;
    case NNN_TAP_EXP: d = {NB, 0, 0, 0, NB, 0}; *ptr = TP(exp_); return true;
    case NNN_TAP_FEATURES: d = {NFEAT, 0, 0, 0, NFEAT, 1}; *ptr = TP(feat); return true;
    case NNN_TAP_SILENCE: d = {1, 1, 0, 0, 1, 0}; *ptr = TP(silence); return true;
    case NNN_TAP_G_RAW: d = {NB, 0, 0, 0, NB, 0}; *ptr = TP(g_raw); return true;
    case NNN_TAP_G: d = {NB, 0, 0, 0, NB, 0}; *ptr = TP(g); return true;
    case NNN_TAP_VAD: d = {1, 0, 0, 0, 1, 0}; *ptr = TP(vad); return true;
    case NNN_TAP_BRANCH: d = {1, 1, 0, 0, 1, 0}; *ptr = TP(branch); return true;
    default: return false;
    }
#undef TP
}

extern "C" int nnn_tap_info(int tap, int *len, int *is_int)
{
    TapDesc d;
    const void *p;
    if (!tap_desc(nullptr, tap, d, &p)) return fail("unknown tap %d", tap);
    if (len) *len = d.len;
    if (is_int) *is_int = d.is_int;
    return 0;
}

extern "C" int nnn_batch_set_taps(nnn_batch *h, int on)
{
    if (!h) return fail("null batch");
    if (on && !h->taps_alloc) {   // first use: the tap-only arrays, nset sets like every scratch array
        NNN_RT_LOCK;
        if (int rc = quiesce(h)) return rc;
        const size_t Sp = (size_t)h->S_pad;
        Buffers &q = h->b[0];
#define NNN_F(name, len) HIPCHK(dalloc(h, &q.name, Sp * (size_t)(len) * h->nset, false));
        NNN_TAP_FIELDS(NNN_F)
#undef NNN_F
        for (int set = 1; set < h->nset; set++) h->b[set] = frame_view(h->b[0], set);
        h->taps_alloc = true;
        // (dalloc clears the arrays with hipMemset on the null stream, which the batch's own streams do not wait for: at 65 536 streams the
        // clearing of these gigabytes ran into the first frame's tap stores -- found by round 6's certified-search test)
        HIPCHK(hipDeviceSynchronize());
    }
    // (1: every tap, the coarse pitch search as the full search so that all 147 cross-correlations exist; 2: the same taps from the certified
    // search -- NNN_TAP_XCORR1 then holds NaN at the lags it ruled out)
    for (int set = 0; set < h->nset; set++) h->b[set].taps = on == 2 ? 2 : (on != 0);
    return 0;
}

extern "C" int nnn_batch_read_tap(nnn_batch *h, int tap, void *host_dst, size_t dst_bytes)
{
    NNN_RT_LOCK;
    if (!h) return fail("null batch");
    TapDesc d;
    const void *p;
    if (!tap_desc(h, tap, d, &p)) return fail("unknown tap %d", tap);
    if (d.needs_taps && !h->b[0].taps) return fail("tap %d is only stored after nnn_batch_set_taps(batch, 1)", tap);
    if (dst_bytes < (size_t)h->S * d.len * 4) return fail("tap buffer too small");
    if (int rc = quiesce(h)) return rc;
    HIPCHK(hipDeviceSynchronize());
    uint32_t *dst = (uint32_t *)host_dst;
    const size_t Sp = (size_t)h->S_pad;
    if (d.layout == 0) {
        std::vector<uint32_t> tmp(Sp * d.sub_len);
        HIPCHK(hipMemcpy(tmp.data(), p, tmp.size() * 4, hipMemcpyDeviceToHost));
        for (int s = 0; s < h->S; s++)
            for (int i = 0; i < d.len; i++)
                dst[(size_t)s * d.len + i] = tmp[((size_t)(s / TILE) * d.sub_len + d.sub_ofs + i) * TILE + s % TILE];
    } else if (d.layout == 2 || d.layout == 4) {
        std::vector<uint32_t> tmp(Sp * 2 * FSTR);
        HIPCHK(hipMemcpy(tmp.data(), p, tmp.size() * 4, hipMemcpyDeviceToHost));
        // (a spectrum's row holds (bin k, bin 480 - k) pairs in the transforms' lane order: spectrum_index)
        for (int s = 0; s < h->S; s++)
            for (int k = 0; k < FREQ; k++) {
                const size_t at = (size_t)s * 2 * FSTR + 2 * (size_t)(d.layout == 4 ? spectrum_index_p(k) : spectrum_index(k));
                dst[(size_t)s * d.len + 2 * k] = tmp[at];
                dst[(size_t)s * d.len + 2 * k + 1] = tmp[at + 1];
            }
    } else {  // newest frame in the history ring
        const size_t hstr = (size_t)hist_stride(h->nslot);
        std::vector<uint32_t> tmp(Sp * hstr);
        HIPCHK(hipMemcpy(tmp.data(), p, tmp.size() * 4, hipMemcpyDeviceToHost));
        int slot = last_slot(h);  // slot of the most recent frame
        for (int s = 0; s < h->S; s++) memcpy(dst + (size_t)s * FRAME, tmp.data() + (size_t)s * hstr + slot * FRAME, FRAME * 4);
    }
    return 0;
}

extern "C" int nnn_batch_read_stamps(nnn_batch *h, long long *dst64)
{
    NNN_RT_LOCK;
    if (!h) return fail("null batch");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(dst64, h->b[0].stamps, 64 * sizeof(long long), hipMemcpyDeviceToHost));
    return 0;
}

// The device's activation functions on their own: y[i] = act(x[i]) with act 0 = tansig_approx, 1 = sigmoid_approx,
// 2 = relu (ref: src/util.rs:29-53) -- a direct known-answer check for the parity tests.
extern "C" int nnn_debug_activations(int device, int act, const float *x, float *y, int n)
{
    NNN_RT_LOCK;
    if (!x || !y || n < 0 || act < 0 || act > 2) return fail("bad argument");
    HIPCHK(hipSetDevice(device));
    std::vector<float> window, dct, tansig, bin_frac;
    std::vector<float2> tw;
    std::vector<int> bin_band;
    float wnorm;
    make_tables(window, dct, tw, tansig, bin_frac, bin_band, wnorm);
    float *d = nullptr;
    HIPCHK(hipMalloc((void **)&d, (size_t)(2 * n + 256) * sizeof(float)));
    float *dx = d + 256, *dy = dx + n;
    hipError_t e = hipMemcpy(d, tansig.data(), 201 * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dx, x, (size_t)n * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess && n) {
        hipLaunchKernelGGL(k_activation_kat, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t) nullptr, (const float *)d, (const float *)dx, dy, act, n);
        e = hipDeviceSynchronize();
    }
    if (e == hipSuccess) e = hipMemcpy(y, dy, (size_t)n * sizeof(float), hipMemcpyDeviceToHost);
    hipFree(d);
    if (e != hipSuccess) return fail("activation sweep failed: %s", hipGetErrorString(e));
    return 0;
}

// ---- profiling / scheduling switches -------------------------------------------------------------
extern "C" int nnn_batch_set_profiling(nnn_batch *h, int on)
{
    if (!h) return fail("null batch");
    h->profiling = on != 0;
    return 0;
}
extern "C" int nnn_batch_num_kernels(void) { return K_COUNT; }
extern "C" const char *nnn_batch_kernel_name(int k) { return (k >= 0 && k < K_COUNT) ? kKernelNames[k] : ""; }
extern "C" int nnn_batch_read_kernel_times(nnn_batch *h, double *total_ms, int64_t *launches, int n)
{
    if (!h) return fail("null batch");
    for (int k = 0; k < n && k < K_COUNT; k++) {
        total_ms[k] = h->k_ms[k];
        launches[k] = h->k_launches[k];
        h->k_ms[k] = 0;
        h->k_launches[k] = 0;
    }
    return 0;
}
extern "C" int nnn_batch_set_graph(nnn_batch *h, int on)
{
    (void)on;
    if (!h) return fail("null batch");
    return 0;   // kept for callers of the round-1 ABI: a group is six launches now and they are always eager
}
extern "C" int nnn_batch_set_inputs_ready(nnn_batch *h, int on)
{
    if (!h) return fail("null batch");
    h->paths.inputs_ready = on != 0;
    return 0;
}
// Parity-test record of every frame processed from now on (include/nnn_batch.h): device memory for `frames` frames.
extern "C" int nnn_batch_set_frame_log(nnn_batch *h, void *d_log, size_t frames)
{
    if (!h) return fail("null batch");
    h->frame_log = (unsigned *)d_log;
    h->frame_log_left = d_log ? frames : 0;
    return 0;
}
// Test hook: the hand-off flag of the frame `frames_ahead` frames from now (0 = the next one) is never published, so the workgroups
// waiting for it run into their timeout and raise the fault.  A negative value switches the hook off.
extern "C" int nnn_batch_debug_withhold_flag(nnn_batch *h, int frames_ahead)
{
    if (!h) return fail("null batch");
    const int seq = frames_ahead < 0 ? 0 : (int)((h->frame_count + (uint64_t)frames_ahead) & 0x3fffffffu) + 1;
    for (int set = 0; set < h->nset; set++) {
        h->b[set].dbg_withhold = seq;
        h->b[set].handoff_ticks = seq ? 20000000ll : HANDOFF_TICKS;   // the withheld flag is given up on after 0.2 s
    }
    return 0;
}
// Test hook: the schedule a call of n_frames on the batch's own stream would get now, as integers (include/nnn_batch.h).  Plans only.
extern "C" int nnn_batch_debug_schedule(nnn_batch *h, int n_frames, int32_t *out, size_t cap)
{
    if (!h || !out) return fail("null argument");
    if (n_frames < 1) return fail("n_frames must be at least 1");
    CallPlan cp = plan_call(h, n_frames, h->stream);
    if ((size_t)n_frames > h->sp_tab.cap) cp.early_hp = false;   // (the call would first grow its parameter table, which drains the batch: prev_pipe off)
    const Schedule sc = plan_schedule(h, cp);
    constexpr size_t HEAD = 8, PER_NODE = 8 + 3 * MAX_WAITS;
    if (cap < HEAD + PER_NODE * sc.nodes.size()) return fail("schedule buffer too small: %zu entries needed", HEAD + PER_NODE * sc.nodes.size());
    const int32_t head[HEAD] = {(int32_t)sc.nodes.size(), (int32_t)cp.sizes.size(), cp.pipe, cp.sched, cp.lanes, sc.fill, sc.fill_after_done, sc.last_syn};
    memcpy(out, head, sizeof(head));
    out += HEAD;
    for (const Node &n : sc.nodes) {
        const int32_t v[8] = {n.stage, n.group, n.frames, n.first, n.stream, n.first_use, n.record, n.n_waits};
        memcpy(out, v, sizeof(v));
        for (int w = 0; w < MAX_WAITS; w++) {
            const Wait x = w < n.n_waits ? n.waits[w] : Wait{-1, -1, -1};
            out[8 + 3 * w] = x.origin, out[9 + 3 * w] = x.stage, out[10 + 3 * w] = x.group;
        }
        out += PER_NODE;
    }
    return 0;
}
// Test hook: the route a host-buffer call of n_frames would take now (include/nnn_batch.h).  Plans only.
extern "C" int nnn_batch_debug_host_plan(nnn_batch *h, int n_frames, const nnn_pcm_layout *L, int has_vad, int64_t out[8])
{
    if (!h || !out || n_frames < 1) return fail("null argument or no frames");
    if (int rc = check_layout(h, L)) return rc;
    const HostPlan p = plan_host_call(h, n_frames, *L, has_vad != 0);
    const int64_t v[8] = {p.route, p.chunk, p.n_chunks, (int64_t)p.span, (int64_t)p.vbytes, (int64_t)p.vofs, p.drop, p.vad_masked};
    memcpy(out, v, sizeof(v));
    return 0;
}
extern "C" int nnn_batch_set_back_end(nnn_batch *h, int mode)
{
    if (!h) return fail("null batch");
    if (mode < -1 || mode > 4) return fail("unknown back-end mode %d", mode);
    h->paths.back_mode = mode;
    return 0;
}
extern "C" int nnn_batch_set_pipeline(nnn_batch *h, int on)
{
    if (!h) return fail("null batch");
    h->paths.use_pipeline = on != 0;
    return 0;
}
extern "C" int nnn_batch_set_schedule(nnn_batch *h, int mode, int lanes)
{
    if (!h) return fail("null batch");
    if (mode < SCHED_SEQ || mode > SCHED_STAGES) return fail("unknown schedule %d", mode);
    h->paths.sched = mode;
    if (lanes >= 1 && lanes <= NSTREAMS - 1) h->paths.n_lanes = lanes;
    h->paths.sched_auto = false;
    return 0;
}

// ---- training-feature rows (include/nnn_train.h) ---------------------------------------------------------------------
struct nnn_train {
    nnn_batch *comb = nullptr, *clean = nullptr, *noise = nullptr;   // three sets of DenoiseFeatures state
    GrowBuf<float> stage;            // device staging of the host entry point: [signal | noise | combined | vad | rows], capacity in frames
    GrowBuf<int32_t> stage_cut;
};

extern "C" void nnn_train_destroy(nnn_train *t)
{
    if (!t) return;
    t->stage.release();
    t->stage_cut.release();
    nnn_batch_destroy(t->comb);
    nnn_batch_destroy(t->clean);
    nnn_batch_destroy(t->noise);
    delete t;
}

extern "C" nnn_train *nnn_train_create(int n_streams, int device)
{
    nnn_train *t = new nnn_train();
    t->comb = nnn_batch_create(nullptr, n_streams, device);
    t->clean = t->comb ? nnn_batch_create(nullptr, n_streams, device) : nullptr;
    t->noise = t->clean ? nnn_batch_create(nullptr, n_streams, device) : nullptr;
    if (!t->noise) {
        std::string keep = g_err;
        nnn_train_destroy(t);
        g_err = keep;
        return nullptr;
    }
    return t;
}

extern "C" int nnn_train_reset(nnn_train *t)
{
    if (!t) return fail("null handle");
    if (int rc = nnn_batch_reset(t->comb)) return rc;
    if (int rc = nnn_batch_reset(t->clean)) return rc;
    return nnn_batch_reset(t->noise);
}

// shift_and_filter_input + the part of compute_frame_features the row needs: everything up to the 42 features for the
// mix, only the band energies of X for the clean and noise states (src/training.rs:129-131 computes their full
// features and says itself that only the transform and band energies are needed; nothing else of them is read).
static void enqueue_feature_group(nnn_batch *h, hipStream_t st, const float *in, size_t stream_stride, size_t frame_stride, int g, bool full)
{
    // `g` consecutive frames (<= GROUP) in scratch sets 0 .. g - 1, the same launches as the denoiser's front: the stateful
    // kernels cover the group in one launch, the per-frame feature stage once per frame
    const Buffers &b = h->b[0];
    const unsigned NT = (unsigned)h->NT, Sp = (unsigned)h->S_pad, ug = (unsigned)g;
    StepParams *sp = h->sp_tab.p;
    StepParams v;
    v.in = (const char *)in;
    v.out = nullptr;
    v.vad = nullptr;
    v.group_stride = (long long)stream_stride * 4;
    v.frame_stride = (long long)frame_stride * 4;
    v.fmt = PCM_F32;
    v.channels = 1;
    v.discard = 0;
    v.slot = (int)(h->frame_count % h->nslot);
    v.n_streams = h->S;
    v.log = nullptr;
    v.log_frames = 0;
    hipLaunchKernelGGL(k_fill_params, dim3(1), dim3(64), 0, st, sp, v, g, h->nslot);
    hipLaunchKernelGGL(k_hp<false>, dim3(NT), dim3(64), 0, st, b, (const StepParams *)sp, g, StepParams{}, 0);
    if (full) {
        const int fc = lpc_launch(h, g);
        if (!fc) hipLaunchKernelGGL(k_lpc_wide, dim3(NT * ug), dim3(320), 0, st, b, (const StepParams *)sp, g);
        else hipLaunchKernelGGL(k_lpc, dim3(NT * ((ug + fc - 1) / fc)), dim3(64), 0, st, b, (const StepParams *)sp, g, fc);
        const int chain = pitch_chained(h, g) ? 1 : 0, seq0 = (int)(h->frame_count & 0x3fffffffu) + 1;
        const unsigned grid = Sp / PK_SPB * (chain ? ug : 1u);
        hipLaunchKernelGGL(k_pitch<false>, dim3(grid), dim3(PK_T), 0, st, b, (const StepParams *)sp, g, chain, seq0, h->tickets, 0, 0);
        if (chain) h->tickets += grid;
        hipLaunchKernelGGL(k_fft_xp, dim3(Sp * ug / FFT_SPB), dim3(64 * FFT_SPB), 0, st, b, (const StepParams *)sp, g);
        hipLaunchKernelGGL(k_features, dim3(NT), dim3(64 * FEAT_WAVES), 0, st, b, g);
    } else {
        hipLaunchKernelGGL(k_fft_x, dim3(Sp * ug / FFT_SPB), dim3(64 * FFT_SPB), 0, st, b, (const StepParams *)sp, g);
    }
    h->frame_count += g;
}

extern "C" int nnn_train_process_device(nnn_train *t, const float *d_signal, const float *d_noise, const float *d_combined,
                                        const int32_t *d_cutoff, const float *d_vad, float *d_rows, int n_frames,
                                        size_t stream_stride, size_t frame_stride, void *hip_stream)
{
    if (!t) return fail("null handle");
    if (n_frames <= 0) return 0;
    if (!d_signal || !d_noise || !d_combined || !d_cutoff || !d_vad || !d_rows) return fail("null buffer");
    nnn_batch *h = t->comb;
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : h->stream;
    const size_t S = (size_t)h->S;
    const int gmax = t->comb->gmax;
    for (int f0 = 0; f0 < n_frames; f0 += gmax) {
        const int g = n_frames - f0 < gmax ? n_frames - f0 : gmax;
        const size_t off = (size_t)f0 * frame_stride;
        enqueue_feature_group(t->comb, st, d_combined + off, stream_stride, frame_stride, g, true);
        enqueue_feature_group(t->clean, st, d_signal + off, stream_stride, frame_stride, g, false);
        enqueue_feature_group(t->noise, st, d_noise + off, stream_stride, frame_stride, g, false);
        hipLaunchKernelGGL(k_train_rows, dim3((unsigned)(h->NT * g)), dim3(64), 0, st, t->comb->b[0], t->clean->b[0], t->noise->b[0],
                           (const int *)d_cutoff + (size_t)f0 * S, d_vad + (size_t)f0 * S, d_rows + (size_t)f0 * S * TRAIN_COLS);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int nnn_train_process_host(nnn_train *t, const float *signal, const float *noise, const float *combined,
                                      const int32_t *cutoff, const float *vad, float *rows, int n_frames)
{
    if (!t) return fail("null handle");
    if (n_frames <= 0) return 0;
    if (!signal || !noise || !combined || !cutoff || !vad || !rows) return fail("null buffer");
    nnn_batch *h = t->comb;
    HIPCHK(hipSetDevice(h->device));
    const size_t S = (size_t)h->S, na = S * n_frames * FRAME, nl = S * n_frames;
    if ((size_t)n_frames > t->stage.cap && grow(h, true, t->stage, (3 * na + nl + nl * TRAIN_COLS) * sizeof(float), (size_t)n_frames, &t->stage_cut, nl * sizeof(int32_t))) return 1;
    float *d = t->stage.p, *dv = d + 3 * na, *dr = dv + nl;
    int32_t *dc = t->stage_cut.p;
    // In chunks like the denoiser's host calls.  Audio is [stream][frame][480] (a chunk: 2-D copies, one row per stream), labels and rows
    // are frame-major (a chunk: one run each).
    const size_t pitch = (size_t)n_frames * FRAME * 4;
    const float *src[3] = {signal, noise, combined};
    return pump_chunks(h, n_frames, plan_train_chunk(h, n_frames),
        [&](int t0, int n) {
            const size_t off = (size_t)t0 * FRAME, lo = (size_t)t0 * S;
            hipError_t e = hipSuccess;
            for (int k = 0; k < 3 && e == hipSuccess; k++)
                e = hipMemcpy2DAsync(d + k * na + off, pitch, src[k] + off, pitch, (size_t)n * FRAME * 4, S, hipMemcpyHostToDevice, h->copy_in);
            if (e == hipSuccess) e = hipMemcpyAsync(dv + lo, vad + lo, n * S * 4, hipMemcpyHostToDevice, h->copy_in);
            if (e == hipSuccess) e = hipMemcpyAsync(dc + lo, cutoff + lo, n * S * 4, hipMemcpyHostToDevice, h->copy_in);
            return e;
        },
        [&](int t0, int n) {
            const size_t off = (size_t)t0 * FRAME, lo = (size_t)t0 * S;
            return nnn_train_process_device(t, d + off, d + na + off, d + 2 * na + off, dc + lo, dv + lo, dr + lo * TRAIN_COLS, n,
                                            (size_t)n_frames * FRAME, FRAME, h->stream);
        },
        [&](int t0, int n) {
            return hipMemcpyAsync(rows + t0 * S * TRAIN_COLS, dr + t0 * S * TRAIN_COLS, n * S * TRAIN_COLS * 4, hipMemcpyDeviceToHost, h->copy_out);
        });
}

// ---- model entry points -------------------------------------------------------------------------
extern "C" RNNModel *nnn_model_from_bytes(const uint8_t *bytes, size_t len)
{
    RNNModel *m = nnn_model_parse(bytes, len);
    if (!m) fail("malformed .rnn model");
    return m;
}
extern "C" RNNModel *nnn_model_default(void)
{
    size_t len;
    const uint8_t *w = nnn_builtin_weights(&len);
    return nnn_model_parse(w, len);
}
// RNNoise text model -> .rnn bytes (ref: train/convert_rnnoise.py:18-29).  Python's str.strip / str.split / int():
// ASCII whitespace separators, optional sign, decimal digits (int() also takes '_' separators and non-ASCII digits;
// no model file uses them and they are rejected here).
extern "C" long nnn_convert_rnnoise_text(const char *text, size_t len, uint8_t *out, size_t cap)
{
    static const char kHeader[] = "rnnoise-nu model file version 1";
    auto is_ws = [](char c) { return c == ' ' || (c >= '\t' && c <= '\r'); };
    if (!text) { fail("null text"); return -1; }
    size_t eol = 0;
    while (eol < len && text[eol] != '\n') eol++;
    size_t a = 0, b = eol;
    while (a < b && is_ws(text[a])) a++;
    while (b > a && is_ws(text[b - 1])) b--;
    if (b - a != sizeof(kHeader) - 1 || memcmp(text + a, kHeader, b - a) != 0) { fail("Unexpected input file format"); return -1; }
    long n = 0;
    size_t i = eol < len ? eol + 1 : len;
    while (i < len) {
        while (i < len && is_ws(text[i])) i++;
        if (i >= len) break;
        bool neg = false;
        if (text[i] == '+' || text[i] == '-') neg = text[i++] == '-';
        if (i >= len || text[i] < '0' || text[i] > '9') { fail("token %ld is not an integer", n); return -1; }
        unsigned v = 0;   // only the value modulo 256 matters
        while (i < len && text[i] >= '0' && text[i] <= '9') v = (v * 10u + (unsigned)(text[i++] - '0')) & 0xffffu;
        if (i < len && !is_ws(text[i])) { fail("token %ld is not an integer", n); return -1; }
        const uint8_t byte = (uint8_t)((neg ? 256u - (v & 255u) : v) & 255u);   // Python's non-negative modulo
        if (out) {
            if ((size_t)n >= cap) { fail("output buffer too small"); return -1; }
            out[n] = byte;
        }
        n++;
    }
    return n;
}
extern "C" RNNModel *nnn_model_from_rnnoise_text(const char *text, size_t len)
{
    const long n = nnn_convert_rnnoise_text(text, len, nullptr, 0);
    if (n < 0) return nullptr;
    std::vector<uint8_t> bytes((size_t)n);
    if (nnn_convert_rnnoise_text(text, len, bytes.data(), bytes.size()) != n) return nullptr;
    return nnn_model_from_bytes(bytes.data(), bytes.size());
}
extern "C" void nnn_model_free(RNNModel *m) { delete m; }
// RnnModel is Clone in the reference (#[derive(Clone)], src/rnn.rs:54): an independent copy of the parameters
extern "C" RNNModel *nnn_model_clone(const RNNModel *m)
{
    if (!m) {
        fail("null model");
        return nullptr;
    }
    return new RNNModel(*m);
}
extern "C" void nnn_model_shape(const RNNModel *m, int32_t s[12])
{
    s[0] = m->input_dense.nb_inputs; s[1] = m->input_dense.nb_neurons; s[2] = m->vad_gru.nb_neurons;
    s[3] = m->noise_gru.nb_neurons; s[4] = m->denoise_gru.nb_neurons; s[5] = m->denoise_output.nb_neurons;
    s[6] = m->input_dense.activation; s[7] = m->vad_gru.activation; s[8] = m->noise_gru.activation;
    s[9] = m->denoise_gru.activation; s[10] = m->denoise_output.activation; s[11] = m->vad_output.activation;
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
