// nnn_node.cpp -- all the GPUs of a node behind one object (include/nnn_node.h): contiguous stream shards, one nnn_batch and one host
// thread per device, fan-out and join inside every call.  Host-only code above the batch ABI: everything that touches a device goes
// through nnn_batch_*.  (ref: the reference's hosts walk a vector of independent states, src/nnnoiseless.rs:305-320.)
#include <pthread.h>
#include <sched.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <condition_variable>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/nnn_node.h"

int nnn_set_error(const char *msg);   // nnn_batch_core.hip

// Pins the calling thread to the CPUs local to a device's PCI function ("0-31,128-159" in the kernel's cpulist syntax, from
// nnn_device_local_cpulist): a worker that stages pageable buffers and enqueues for GPU i should run on the socket GPU i hangs off.
// Best effort: an empty or unparsable list leaves the thread where it is.
static bool pin_to_cpulist(const char *list)
{
    cpu_set_t set;
    CPU_ZERO(&set);
    int n = 0;
    for (const char *p = list; *p;) {
        char *e;
        const long a = strtol(p, &e, 10);
        if (e == p) break;
        long b = a;
        p = e;
        if (*p == '-') {
            b = strtol(p + 1, &e, 10);
            if (e == p + 1) break;
            p = e;
        }
        for (long c = a; c <= b && c < CPU_SETSIZE; c++)
            if (c >= 0) { CPU_SET((int)c, &set); n++; }
        if (*p == ',') p++;
        else break;
    }
    return n > 0 && pthread_setaffinity_np(pthread_self(), sizeof(set), &set) == 0;
}

namespace {
// a host thread that runs the jobs its shard is handed, one at a time
struct Worker {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    std::function<int()> job;
    bool has_job = false, done = true, quit = false;
    int rc = 0;
    std::string err;
    void loop()
    {
        for (;;) {
            std::function<int()> j;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return has_job || quit; });
                if (quit) return;
                j = job;
                has_job = false;
            }
            const int r = j();
            std::string e = r ? nnn_last_error() : "";   // (the error text is thread-local: carried back to the caller's thread)
            {
                std::lock_guard<std::mutex> lk(mu);
                rc = r;
                err = e;
                done = true;
            }
            cv.notify_all();
        }
    }
    void post(std::function<int()> j)
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            job = std::move(j);
            has_job = true;
            done = false;
        }
        cv.notify_all();
    }
    int wait()
    {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return done; });
        return rc;
    }
};
}  // namespace

struct nnn_node {
    struct Shard {
        nnn_batch *b = nullptr;
        int device = 0, lo = 0, hi = 0;
        Worker *w = nullptr;
        std::vector<float> vad;   // host calls: this shard's VAD block [n_frames][hi - lo] before it is spread over the node's rows
        std::string cpus;         // the CPUs its worker is pinned to ("" = not pinned)
    };
    std::vector<Shard> shards;
    int n_streams = 0;
    bool failed = false;          // a call failed on some shard: the shards may sit at different frame counts.  Sticky until nnn_node_reset
                                  // (every process call refuses), like a batch's own fault.
    std::string fail_text;
    bool threads = true;          // NNN_NODE_THREADS=0: the shards one after the other on the caller's thread (debugging; the
                                  // test-only interpreter build runs kernels on the calling thread and is not re-entrant)
};

// Every shard runs fn(shard index) -- all of them, also when one fails, on the shards' own threads or (NNN_NODE_THREADS=0, one shard)
// one after the other on the caller's: either way the other shards are joined and have advanced.  Returns the first failure in
// shard order with its text in nnn_last_error().
static int fan_out(nnn_node *n, const std::function<int(int)> &fn)
{
    int rc = 0;
    std::string err;
    if (!n->threads || n->shards.size() == 1) {
        for (size_t i = 0; i < n->shards.size(); i++) {
            const int r = fn((int)i);
            if (r && !rc) {
                rc = r;
                err = nnn_last_error();
            }
        }
    } else {
        for (size_t i = 0; i < n->shards.size(); i++) n->shards[i].w->post([&fn, i] { return fn((int)i); });
        for (size_t i = 0; i < n->shards.size(); i++) {
            const int r = n->shards[i].w->wait();
            if (r && !rc) {
                rc = r;
                err = n->shards[i].w->err;
            }
        }
    }
    if (rc) nnn_set_error(err.c_str());
    return rc;
}
// a processing call: refused while the node is failed; a failure makes it so
static int process_call(nnn_node *n, const std::function<int(int)> &fn)
{
    if (n->failed) {
        std::string t = "node failed earlier (reset it): " + n->fail_text;
        return nnn_set_error(t.c_str());
    }
    const int rc = fan_out(n, fn);
    if (rc) {
        n->failed = true;
        n->fail_text = nnn_last_error();
        nnn_set_error(n->fail_text.c_str());
    }
    return rc;
}

extern "C" void nnn_node_destroy(nnn_node *n)
{
    if (!n) return;
    for (auto &s : n->shards) {
        if (s.w) {
            {
                std::lock_guard<std::mutex> lk(s.w->mu);
                s.w->quit = true;
            }
            s.w->cv.notify_all();
            if (s.w->th.joinable()) s.w->th.join();
            delete s.w;
        }
        if (s.b) nnn_batch_destroy(s.b);
    }
    delete n;
}

extern "C" nnn_node *nnn_node_create(const RNNModel *model, int n_streams, const int *devices, int n_devices, const nnn_batch_opts *opts)
{
    if (!devices || n_devices <= 0) {
        nnn_set_error("need at least one device");
        return nullptr;
    }
    if (n_streams < n_devices) {
        nnn_set_error("fewer streams than devices");
        return nullptr;
    }
    nnn_node *n = new nnn_node();
    n->n_streams = n_streams;
    if (const char *e = getenv("NNN_NODE_THREADS")) n->threads = atoi(e) != 0;
    n->shards.resize((size_t)n_devices);
    const int base = n_streams / n_devices, rem = n_streams % n_devices;
    for (int i = 0; i < n_devices; i++) {   // contiguous, balanced: nnnoiseless_amd/shard.py's shard_range
        nnn_node::Shard &s = n->shards[(size_t)i];
        s.device = devices[i];
        s.lo = i * base + (i < rem ? i : rem);
        s.hi = s.lo + base + (i < rem ? 1 : 0);
    }
    // One worker per shard, pinned to the CPUs local to its device's PCI function (the socket its GPU hangs off: a worker stages pageable
    // buffers and enqueues for that GPU), then every worker makes its own batch: the thread is pinned BEFORE it allocates and uploads, so the page-locked
    // staging buffers and the tables' host copies come from its GPU's socket.  The creations themselves still run one after another:
    // nnn_batch_create_opts holds the library's runtime lock for its whole length (allocation and legacy-stream copies must not overlap
    // another thread's stream capture, g_rt_mu in nnn_batch_core.hip), so eight devices take eight creations' time.
    if (n->threads && n_devices > 1)
        for (auto &s : n->shards) {
            s.w = new Worker();
            s.w->th = std::thread([w = s.w] { w->loop(); });
        }
    const int rc = fan_out(n, [&](int i) {
        nnn_node::Shard &s = n->shards[(size_t)i];
        char cpus[512];
        if (s.w && nnn_device_local_cpulist(s.device, cpus, sizeof(cpus)) == 0 && pin_to_cpulist(cpus)) s.cpus = cpus;
        const int cnt = s.hi - s.lo;
        s.b = nnn_batch_create_opts(model ? &model : nullptr, &cnt, 1, s.device, opts);
        return s.b ? 0 : 1;
    });
    if (rc) {
        std::string keep = nnn_last_error();
        nnn_node_destroy(n);
        nnn_set_error(keep.c_str());
        return nullptr;
    }
    return n;
}

extern "C" int nnn_node_num_streams(const nnn_node *n) { return n ? n->n_streams : 0; }
extern "C" int nnn_node_num_shards(const nnn_node *n) { return n ? (int)n->shards.size() : 0; }
extern "C" int nnn_node_shard(const nnn_node *n, int i, int *device, int *lo, int *hi)
{
    if (!n || i < 0 || i >= (int)n->shards.size()) return nnn_set_error("no such shard");
    if (device) *device = n->shards[(size_t)i].device;
    if (lo) *lo = n->shards[(size_t)i].lo;
    if (hi) *hi = n->shards[(size_t)i].hi;
    return 0;
}
extern "C" const char *nnn_node_shard_cpus(const nnn_node *n, int i)
{
    return (n && i >= 0 && i < (int)n->shards.size()) ? n->shards[(size_t)i].cpus.c_str() : "";
}
extern "C" nnn_batch *nnn_node_batch(nnn_node *n, int i) { return (n && i >= 0 && i < (int)n->shards.size()) ? n->shards[(size_t)i].b : nullptr; }

extern "C" int nnn_node_reset(nnn_node *n)
{
    if (!n) return nnn_set_error("null node");
    const int rc = fan_out(n, [n](int i) { return nnn_batch_reset(n->shards[(size_t)i].b); });
    if (!rc) {
        n->failed = false;
        n->fail_text.clear();
    }
    return rc;
}

// the shards' VAD blocks ([t][shard stream]) into the node's rows ([t][all streams])
static void spread_vad(nnn_node *n, float *vad, int n_frames)
{
    if (!vad) return;
    for (auto &s : n->shards) {
        const size_t cnt = (size_t)(s.hi - s.lo);
        if (nnn_batch_num_held(s.b) == 0) {
            for (int t = 0; t < n_frames; t++) memcpy(vad + (size_t)t * n->n_streams + s.lo, s.vad.data() + (size_t)t * cnt, cnt * sizeof(float));
            continue;
        }
        // (a held stream's entries are not the call's to write, nnn_batch_hold_streams: the caller's values stay)
        std::vector<uint8_t> held(cnt);
        nnn_batch_held_mask(s.b, held.data(), cnt);
        for (int t = 0; t < n_frames; t++)
            for (size_t i = 0; i < cnt; i++)
                if (!held[i]) vad[(size_t)t * n->n_streams + s.lo + i] = s.vad[(size_t)t * cnt + i];
    }
}

extern "C" int nnn_node_process_host(nnn_node *n, const float *in, float *out, float *vad, int n_frames, size_t stream_stride, size_t frame_stride)
{
    if (!n) return nnn_set_error("null node");
    if (n_frames <= 0) return 0;
    if (!in || !out) return nnn_set_error("null buffer");
    const int rc = process_call(n, [&](int i) {
        nnn_node::Shard &s = n->shards[(size_t)i];
        if (vad) s.vad.resize((size_t)n_frames * (size_t)(s.hi - s.lo));
        return nnn_batch_process_host(s.b, in + (size_t)s.lo * stream_stride, out + (size_t)s.lo * stream_stride, vad ? s.vad.data() : nullptr,
                                      n_frames, stream_stride, frame_stride);
    });
    if (!rc) spread_vad(n, vad, n_frames);
    return rc;
}

extern "C" int nnn_node_process_pcm_host(nnn_node *n, const void *in, void *out, float *vad, int n_frames, const nnn_pcm_layout *L)
{
    if (!n) return nnn_set_error("null node");
    if (n_frames <= 0) return 0;
    if (!in || !out || !L) return nnn_set_error("null argument");
    if (L->channels < 1) return nnn_set_error("channels must be positive");
    for (auto &s : n->shards)
        if (s.lo % L->channels || s.hi % L->channels) return nnn_set_error("the stream split cuts a channel group: n_streams / channels must divide evenly over the shards");
    const size_t e = L->format == NNN_PCM_I16 ? 2 : 4;
    const int rc = process_call(n, [&](int i) {
        nnn_node::Shard &s = n->shards[(size_t)i];
        if (vad) s.vad.resize((size_t)n_frames * (size_t)(s.hi - s.lo));
        const size_t off = (size_t)(s.lo / L->channels) * L->group_stride * e;   // the shard's first group
        return nnn_batch_process_pcm_host(s.b, (const char *)in + off, (char *)out + off, vad ? s.vad.data() : nullptr, n_frames, L);
    });
    if (!rc) spread_vad(n, vad, n_frames);
    return rc;
}

extern "C" int nnn_node_process_device_streams(nnn_node *n, const float *const *d_in, float *const *d_out, float *const *d_vad,
                                               void *const *hip_streams, int n_tables, int n_frames, size_t stream_stride, size_t frame_stride)
{
    if (!n) return nnn_set_error("null node");
    if (n_tables != (int)n->shards.size()) return nnn_set_error("the pointer tables must have one entry per shard");
    if (n_frames <= 0) return 0;
    if (!d_in || !d_out) return nnn_set_error("null buffer table");
    return process_call(n, [&](int i) {
        return nnn_batch_process_device(n->shards[(size_t)i].b, d_in[i], d_out[i], d_vad ? d_vad[i] : nullptr, n_frames, stream_stride, frame_stride,
                                        hip_streams ? hip_streams[i] : nullptr);
    });
}
extern "C" int nnn_node_process_device(nnn_node *n, const float *const *d_in, float *const *d_out, float *const *d_vad, int n_frames,
                                       size_t stream_stride, size_t frame_stride)
{
    return nnn_node_process_device_streams(n, d_in, d_out, d_vad, nullptr, n ? (int)n->shards.size() : 0, n_frames, stream_stride, frame_stride);
}

extern "C" int nnn_node_synchronize(nnn_node *n)
{
    if (!n) return nnn_set_error("null node");
    return fan_out(n, [n](int i) { return nnn_batch_synchronize(n->shards[(size_t)i].b); });
}

extern "C" int nnn_node_fault(const nnn_node *n)
{
    if (!n) return 0;
    for (auto &s : n->shards)
        if (nnn_batch_fault(s.b)) return 1;
    return 0;
}

// ---- per-stream state records by node-global index --------------------------------------------------------------------------------
// The list is split by shard (part k: the shard-local indices, and where each entry sits in the caller's list); every part is checked on
// its shard before any shard is written.
int nnn_batch_check_streams(const nnn_batch *h, int op, const int *streams, int n, const void *host_rec, size_t bytes, bool need_buf);   // nnn_batch_streams.hip
enum { NODE_SS_RESET = 0, NODE_SS_EXPORT = 1, NODE_SS_IMPORT = 2, NODE_SS_HOLD = 3, NODE_SS_RESUME = 4 };   // (nnn_batch_streams.hip's SsOp)
static int node_split(const nnn_node *n, const int *streams, int n_list, std::vector<std::vector<int>> &local, std::vector<std::vector<int>> &at)
{
    if (!n) return nnn_set_error("null node");
    if (n_list < 0) return nnn_set_error("negative stream count");
    if (n_list > 0 && !streams) return nnn_set_error("null stream list");
    local.assign(n->shards.size(), {});
    at.assign(n->shards.size(), {});
    for (int i = 0; i < n_list; i++) {
        const int s = streams[i];
        if (s < 0 || s >= n->n_streams) {
            char t[96];
            snprintf(t, sizeof(t), "stream index %d (entry %d) outside [0, %d)", s, i, n->n_streams);
            return nnn_set_error(t);
        }
        size_t k = 0;
        while (s >= n->shards[k].hi) k++;   // (shards are contiguous and in order)
        local[k].push_back(s - n->shards[k].lo);
        at[k].push_back(i);
    }
    return 0;
}

extern "C" int nnn_node_reset_streams(nnn_node *n, const int *streams, int n_list)
{
    std::vector<std::vector<int>> local, at;
    if (int rc = node_split(n, streams, n_list, local, at)) return rc;
    for (size_t k = 0; k < local.size(); k++)
        if (int rc = nnn_batch_check_streams(n->shards[k].b, NODE_SS_RESET, local[k].data(), (int)local[k].size(), nullptr, 0, false)) return rc;
    for (size_t k = 0; k < local.size(); k++)
        if (!local[k].empty())
            if (int rc = nnn_batch_reset_streams(n->shards[k].b, local[k].data(), (int)local[k].size())) return rc;
    return 0;
}

extern "C" int nnn_node_export_streams(nnn_node *n, const int *streams, int n_list, void *host_dst, size_t dst_bytes)
{
    std::vector<std::vector<int>> local, at;
    if (int rc = node_split(n, streams, n_list, local, at)) return rc;
    if (n_list > 0 && !host_dst) return nnn_set_error("null record buffer");
    if (dst_bytes < (size_t)n_list * NNN_STREAM_STATE_BYTES) return nnn_set_error("record buffer too small");
    for (size_t k = 0; k < local.size(); k++)
        if (int rc = nnn_batch_check_streams(n->shards[k].b, NODE_SS_EXPORT, local[k].data(), (int)local[k].size(), nullptr, 0, false)) return rc;
    std::vector<unsigned char> part;
    for (size_t k = 0; k < local.size(); k++) {
        if (local[k].empty()) continue;
        part.resize(local[k].size() * NNN_STREAM_STATE_BYTES);
        if (int rc = nnn_batch_export_streams(n->shards[k].b, local[k].data(), (int)local[k].size(), part.data(), part.size())) return rc;
        for (size_t j = 0; j < at[k].size(); j++)
            memcpy((char *)host_dst + (size_t)at[k][j] * NNN_STREAM_STATE_BYTES, part.data() + j * NNN_STREAM_STATE_BYTES, NNN_STREAM_STATE_BYTES);
    }
    return 0;
}

extern "C" int nnn_node_import_streams(nnn_node *n, const int *streams, int n_list, const void *host_src, size_t src_bytes)
{
    std::vector<std::vector<int>> local, at;
    if (int rc = node_split(n, streams, n_list, local, at)) return rc;
    if (n_list > 0 && !host_src) return nnn_set_error("null record buffer");
    if (src_bytes < (size_t)n_list * NNN_STREAM_STATE_BYTES) return nnn_set_error("record buffer too small");
    std::vector<std::vector<unsigned char>> parts(local.size());
    for (size_t k = 0; k < local.size(); k++) {
        parts[k].resize(local[k].size() * NNN_STREAM_STATE_BYTES);
        for (size_t j = 0; j < at[k].size(); j++)
            memcpy(parts[k].data() + j * NNN_STREAM_STATE_BYTES, (const char *)host_src + (size_t)at[k][j] * NNN_STREAM_STATE_BYTES, NNN_STREAM_STATE_BYTES);
        if (int rc = nnn_batch_check_streams(n->shards[k].b, NODE_SS_IMPORT, local[k].data(), (int)local[k].size(), parts[k].data(), parts[k].size(), true))
            return rc;
    }
    for (size_t k = 0; k < local.size(); k++)
        if (!local[k].empty())
            if (int rc = nnn_batch_import_streams(n->shards[k].b, local[k].data(), (int)local[k].size(), parts[k].data(), parts[k].size())) return rc;
    return 0;
}

// hold / resume by node-global index (nnn_batch_hold_streams): every shard's part is checked before any shard is changed
static int node_hold(nnn_node *n, bool hold, const int *streams, int n_list)
{
    std::vector<std::vector<int>> local, at;
    if (int rc = node_split(n, streams, n_list, local, at)) return rc;
    for (size_t k = 0; k < local.size(); k++)
        if (int rc = nnn_batch_check_streams(n->shards[k].b, hold ? NODE_SS_HOLD : NODE_SS_RESUME, local[k].data(), (int)local[k].size(), nullptr, 0, false)) return rc;
    for (size_t k = 0; k < local.size(); k++)
        if (!local[k].empty())
            if (int rc = hold ? nnn_batch_hold_streams(n->shards[k].b, local[k].data(), (int)local[k].size())
                              : nnn_batch_resume_streams(n->shards[k].b, local[k].data(), (int)local[k].size())) return rc;
    return 0;
}
extern "C" int nnn_node_hold_streams(nnn_node *n, const int *streams, int n_list) { return node_hold(n, true, streams, n_list); }
extern "C" int nnn_node_resume_streams(nnn_node *n, const int *streams, int n_list) { return node_hold(n, false, streams, n_list); }
extern "C" int nnn_node_num_held(const nnn_node *n)
{
    int total = 0;
    if (n)
        for (const auto &s : n->shards) total += nnn_batch_num_held(s.b);
    return total;
}

// gain floors by node-global index (nnn_batch_set_gain_floor): every shard's part is checked before any shard is changed
int nnn_batch_check_gain_floor(const nnn_batch *h, const int *streams, int n, const float *floors, int bands, bool set);   // nnn_batch_floor.hip
extern "C" int nnn_node_set_gain_floor(nnn_node *n, const int *streams, int n_list, const float *floors, int bands)
{
    std::vector<std::vector<int>> local, at;
    if (int rc = node_split(n, streams, n_list, local, at)) return rc;
    if (n_list > 0 && !floors) return nnn_set_error("null floor values");
    if (bands != 1 && bands != 22) return nnn_set_error("bands must be 1 or 22");
    std::vector<std::vector<float>> parts(local.size());
    for (size_t k = 0; k < local.size(); k++) {
        for (size_t j = 0; j < at[k].size(); j++)
            parts[k].insert(parts[k].end(), floors + (size_t)at[k][j] * bands, floors + (size_t)(at[k][j] + 1) * bands);
        if (int rc = nnn_batch_check_gain_floor(n->shards[k].b, local[k].data(), (int)local[k].size(), parts[k].data(), bands, true)) return rc;
    }
    for (size_t k = 0; k < local.size(); k++)
        if (!local[k].empty())
            if (int rc = nnn_batch_set_gain_floor(n->shards[k].b, local[k].data(), (int)local[k].size(), parts[k].data(), bands)) return rc;
    return 0;
}
extern "C" int nnn_node_get_gain_floor(nnn_node *n, const int *streams, int n_list, float *floors)
{
    std::vector<std::vector<int>> local, at;
    if (int rc = node_split(n, streams, n_list, local, at)) return rc;
    if (n_list > 0 && !floors) return nnn_set_error("null floor buffer");
    std::vector<float> part;
    for (size_t k = 0; k < local.size(); k++) {
        if (local[k].empty()) continue;
        part.resize(local[k].size() * 22);
        if (int rc = nnn_batch_get_gain_floor(n->shards[k].b, local[k].data(), (int)local[k].size(), part.data())) return rc;
        for (size_t j = 0; j < at[k].size(); j++) memcpy(floors + (size_t)at[k][j] * 22, part.data() + j * 22, 22 * sizeof(float));
    }
    return 0;
}
extern "C" int nnn_node_num_floored(const nnn_node *n)
{
    int total = 0;
    if (n)
        for (const auto &s : n->shards) total += nnn_batch_num_floored(s.b);
    return total;
}

// channel link of every shard (nnn_batch_set_channel_link): every shard is checked -- its own refusals, and a first stream that would split a
// link group over two shards -- before any shard is changed
int nnn_batch_check_channel_link(const nnn_batch *h, int channels, int mode, int first);   // nnn_batch_link.hip
extern "C" int nnn_node_set_channel_link(nnn_node *n, int channels, int mode)
{
    if (!n) return nnn_set_error("null node");
    for (const auto &s : n->shards)
        if (int rc = nnn_batch_check_channel_link(s.b, channels, mode, s.lo)) return rc;
    for (const auto &s : n->shards)
        if (int rc = nnn_batch_set_channel_link(s.b, channels, mode)) return rc;
    return 0;
}
extern "C" int nnn_node_get_channel_link(const nnn_node *n, int *channels, int *mode)
{
    if (!n || n->shards.empty()) return nnn_set_error("null node");
    return nnn_batch_get_channel_link(n->shards[0].b, channels, mode);
}
