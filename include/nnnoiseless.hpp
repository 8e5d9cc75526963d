// SPDX-License-Identifier: BSD-3-Clause
// nnnoiseless.hpp -- C++ host-side mirror of the reference's public interface for the process_frame path
// (Rust is not available in the build image, so the host side above the C ABI is C++; the Rust façade a
// maintainer would compile is in bindings/rust/).  Same names, argument meaning and error behaviour:
//
//   reference (Rust)                                         here (C++)
//   RnnModel::from_bytes(&[u8]) -> Option<RnnModel>          RnnModel::from_bytes(ptr, len) -> std::optional<RnnModel>   src/rnn.rs:75-77
//   RnnModel::default()                                      RnnModel::default_model()                                  src/rnn.rs:235-240
//   DenoiseState::FRAME_SIZE                                 DenoiseState::FRAME_SIZE                                   src/denoise.rs:46
//   DenoiseState::new() / from_model / with_model            DenoiseState::create() / from_model / with_model           src/denoise.rs:53-74
//   process_frame(&mut self, &mut [f32], &[f32]) -> f32      process_frame(float* out, const float* in) -> float        src/denoise.rs:95-116
//   #[derive(Clone)] DenoiseState                            DenoiseState::clone() / BatchDenoiser::clone()             src/denoise.rs:36
//   for ch { states[ch].process_frame(..) }                  BatchDenoiser::process(...)                                src/signal.rs:102-104
//
// Everything runs in the HIP kernels behind include/nnn_batch.h; failures throw std::runtime_error.
#pragma once
#include <array>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "nnn_batch.h"
#include "nnn_fit.h"
#include "nnn_gate.h"
#include "nnn_mix.h"
#include "nnn_pick.h"
#include "nnn_node.h"
#include "nnn_pack.h"
#include "nnn_rate.h"
#include "nnn_resample.h"
#include "nnn_score.h"
#include "nnn_sim.h"
#include "nnn_train.h"

namespace nnnoiseless {

class RnnModel {
  public:
    static std::optional<RnnModel> from_bytes(const uint8_t *bytes, size_t len)
    {
        RNNModel *m = nnn_model_from_bytes(bytes, len);
        if (!m) return std::nullopt;
        return RnnModel(m);
    }
    // an RNNoise / rnnoise-nu text model (train/convert_rnnoise.py + from_bytes in one step)
    static std::optional<RnnModel> from_rnnoise_text(const std::string &text)
    {
        RNNModel *m = nnn_model_from_rnnoise_text(text.data(), text.size());
        if (!m) return std::nullopt;
        return RnnModel(m);
    }
    static RnnModel default_model() { return RnnModel(nnn_model_default()); }
    const RNNModel *raw() const { return m_.get(); }
    // a copy with its own storage (nnn_model_clone); plain copies of this class share one immutable model
    RnnModel deep_clone() const
    {
        RNNModel *m = nnn_model_clone(m_.get());
        if (!m) throw std::runtime_error(std::string("nnnoiseless: ") + nnn_last_error());
        return RnnModel(m);
    }

  private:
    explicit RnnModel(RNNModel *m) : m_(m, nnn_model_free) {}
    std::shared_ptr<RNNModel> m_;  // Clone in the reference; sharing is equivalent for an immutable model
};

// n independent DenoiseStates advanced in lock-step on one GPU
// Page-locked host memory for the host-buffer calls (nnn_host_alloc): n elements of T.
template <class T> class PinnedBuffer {
  public:
    explicit PinnedBuffer(size_t n) : p_((T *)nnn_host_alloc(n * sizeof(T))), n_(n)
    {
        if (!p_) throw std::runtime_error(std::string("nnnoiseless: ") + nnn_last_error());
    }
    ~PinnedBuffer() { nnn_host_free(p_); }
    PinnedBuffer(const PinnedBuffer &) = delete;
    PinnedBuffer &operator=(const PinnedBuffer &) = delete;
    T *data() { return p_; }
    const T *data() const { return p_; }
    size_t size() const { return n_; }
    T &operator[](size_t i) { return p_[i]; }

  private:
    T *p_;
    size_t n_;
};

class BatchDenoiser {
  public:
    BatchDenoiser(int n_streams, const RnnModel *model = nullptr, int device = 0)
        : b_(nnn_batch_create(model ? model->raw() : nullptr, n_streams, device), nnn_batch_destroy)
    {
        if (!b_) throw std::runtime_error(std::string("nnnoiseless: ") + nnn_last_error());
    }
    // several models resident at once: streams [0, n0) run models[0], the next n1 models[1], ... (nullptr = built-in)
    BatchDenoiser(const std::vector<std::pair<const RnnModel *, int>> &groups, int device = 0)
    {
        std::vector<const RNNModel *> ms;
        std::vector<int> ns;
        for (const auto &g : groups) {
            ms.push_back(g.first ? g.first->raw() : nullptr);
            ns.push_back(g.second);
        }
        b_.reset(nnn_batch_create_grouped(ms.data(), ns.data(), (int)ns.size(), device), nnn_batch_destroy);
        if (!b_) throw std::runtime_error(std::string("nnnoiseless: ") + nnn_last_error());
    }
    // a batch sized for calls of at most `max_group_frames` frames (1 = a real-time host ticking one frame per call: 33 KB per
    // stream instead of 360; longer calls still work, cut into groups of that many frames)
    static BatchDenoiser sized(int n_streams, int max_group_frames, const RnnModel *model = nullptr, int device = 0)
    {
        const RNNModel *m = model ? model->raw() : nullptr;
        nnn_batch_opts o = {};
        o.max_group_frames = max_group_frames;
        BatchDenoiser d(nnn_batch_create_opts(&m, &n_streams, 1, device, &o));
        if (!d.b_) throw std::runtime_error(std::string("nnnoiseless: ") + nnn_last_error());
        return d;
    }
    int num_streams() const { return nnn_batch_num_streams(b_.get()); }
    size_t device_bytes() const { return nnn_batch_device_bytes(b_.get()); }
    int max_group_frames() const { return nnn_batch_max_group_frames(b_.get()); }
    // packed PCM in the reference callers' formats (int16 / unit floats, interleaved channels, first frame dropped)
    void process_pcm(const void *in, void *out, float *vad, int n_frames, const nnn_pcm_layout &layout)
    {
        check(nnn_batch_process_pcm_host(b_.get(), in, out, vad, n_frames, &layout));
    }
    void process_pcm_device(const void *d_in, void *d_out, float *d_vad, int n_frames, const nnn_pcm_layout &layout,
                            void *hip_stream = nullptr)
    {
        check(nnn_batch_process_pcm_device(b_.get(), d_in, d_out, d_vad, n_frames, &layout, hip_stream));
    }
    // host buffers: sample i of frame t of stream s at [s * stream_stride + t * frame_stride + i]; vad[t * n_streams + s]
    // (long calls cross the bus in chunks beside the kernels; PinnedBuffer memory goes by DMA, both directions at once)
    void process(const float *in, float *out, float *vad, int n_frames, size_t stream_stride, size_t frame_stride)
    {
        check(nnn_batch_process_host(b_.get(), in, out, vad, n_frames, stream_stride, frame_stride));
    }
    // promise that every process_device call's input is final when the call is made: consecutive calls may then overlap at
    // their boundary (include/nnn_batch.h); outputs stay ordered on the call's stream
    void set_inputs_ready(bool on) { check(nnn_batch_set_inputs_ready(b_.get(), on ? 1 : 0)); }
    // device buffers, asynchronous on `hip_stream` (nullptr = the batch's own stream)
    void process_device(const float *d_in, float *d_out, float *d_vad, int n_frames, size_t stream_stride, size_t frame_stride,
                        void *hip_stream = nullptr)
    {
        check(nnn_batch_process_device(b_.get(), d_in, d_out, d_vad, n_frames, stream_stride, frame_stride, hip_stream));
    }
    // split calls (nnn_batch.h "Split calls"): the first half of process_frame for up to max_group_frames frames -- features
    // [n_frames][n_streams][42] and silence flags [n_frames][n_streams] out -- and the second half with the caller's band gains
    // [n_frames][n_streams][22] in place of the network's (vad [n_frames][n_streams] optional).  `layout` describes the audio buffer of
    // each half.  Device buffers, asynchronous; an analyze is followed by the synthesize of the same n_frames before any other call.
    void analyze_device(const void *d_in, float *d_features, int32_t *d_silence, int n_frames, const nnn_pcm_layout &layout, void *hip_stream = nullptr)
    {
        check(nnn_batch_analyze_device(b_.get(), d_in, d_features, d_silence, n_frames, &layout, hip_stream));
    }
    void synthesize_device(const float *d_gains, const float *d_vad, void *d_out, int n_frames, const nnn_pcm_layout &layout, void *hip_stream = nullptr)
    {
        check(nnn_batch_synthesize_device(b_.get(), d_gains, d_vad, d_out, n_frames, &layout, hip_stream));
    }
    // the same with host buffers (staged in one piece, synchronous)
    void analyze(const void *in, float *features, int32_t *silence, int n_frames, const nnn_pcm_layout &layout)
    {
        check(nnn_batch_analyze_host(b_.get(), in, features, silence, n_frames, &layout));
    }
    void synthesize(const float *gains, const float *vad, void *out, int n_frames, const nnn_pcm_layout &layout)
    {
        check(nnn_batch_synthesize_host(b_.get(), gains, vad, out, n_frames, &layout));
    }
    int pending_frames() const { return nnn_batch_pending_frames(b_.get()); }
    // VAD only (nnn_batch.h "VAD-only calls"): vad [n_frames][n_streams], the values process returns, for up to max_group_frames frames and
    // without the denoiser -- no audio out; synthesis_mem, lastg and the noise / denoise GRU states keep their bytes.  `layout` describes the
    // input (discard_first 0).  Device buffers, asynchronous; host buffers, staged in one piece and synchronous.
    void vad_device(const void *d_in, float *d_vad, int n_frames, const nnn_pcm_layout &layout, void *hip_stream = nullptr)
    {
        check(nnn_batch_vad_device(b_.get(), d_in, d_vad, n_frames, &layout, hip_stream));
    }
    void vad_host(const void *in, float *vad, int n_frames, const nnn_pcm_layout &layout)
    {
        check(nnn_batch_vad_host(b_.get(), in, vad, n_frames, &layout));
    }
    // Network only (nnn_batch.h "Network-only calls"): features [n_frames][n_streams][42] (silence [n_frames][n_streams], may be null) ->
    // raw gains [n_frames][n_streams][22] and vad [n_frames][n_streams] (may be null) from every stream's resident model; moves the three
    // GRU states and nothing else; any n_frames >= 1; allowed between analyze and synthesize.  Device buffers, asynchronous; host buffers,
    // staged in one piece and synchronous.
    void network_device(const float *d_features, const int32_t *d_silence, float *d_gains, float *d_vad, int n_frames, void *hip_stream = nullptr)
    {
        check(nnn_batch_network_device(b_.get(), d_features, d_silence, d_gains, d_vad, n_frames, hip_stream));
    }
    void network_host(const float *features, const int32_t *silence, float *gains, float *vad, int n_frames)
    {
        check(nnn_batch_network_host(b_.get(), features, silence, gains, vad, n_frames));
    }
    void synchronize() { check(nnn_batch_synchronize(b_.get())); }
    // true once a frame hand-off inside the pitch stage has failed (nnn_batch_fault): sticky until reset() / load_state(); for hosts
    // that synchronise their own HIP stream instead of calling synchronize()
    bool fault() const { return nnn_batch_fault(b_.get()) != 0; }
    void reset() { check(nnn_batch_reset(b_.get())); }
    // a second batch with the same models and a copy of every stream's state (DenoiseState: Clone)
    BatchDenoiser clone() const
    {
        nnn_batch *c = nnn_batch_clone(b_.get());
        if (!c) throw std::runtime_error(std::string("nnnoiseless: ") + nnn_last_error());
        return BatchDenoiser(c);
    }
    // the streams' state as bytes (a raw image: loads into a batch of the same shape made by the same build)
    std::vector<uint8_t> save_state() const
    {
        std::vector<uint8_t> buf(nnn_batch_state_bytes(b_.get()));
        check(nnn_batch_save_state(b_.get(), buf.data(), buf.size()));
        return buf;
    }
    void load_state(const std::vector<uint8_t> &buf) { check(nnn_batch_load_state(b_.get(), buf.data(), buf.size())); }
    // per-stream state records (NNN_STREAM_STATE_BYTES each, record i for streams[i]): portable between slots, batches and DenoiseStates
    void reset_streams(const std::vector<int> &streams) { check(nnn_batch_reset_streams(b_.get(), streams.data(), (int)streams.size())); }
    std::vector<uint8_t> export_streams(const std::vector<int> &streams) const
    {
        std::vector<uint8_t> buf(streams.size() * NNN_STREAM_STATE_BYTES);
        check(nnn_batch_export_streams(b_.get(), streams.data(), (int)streams.size(), buf.data(), buf.size()));
        return buf;
    }
    void import_streams(const std::vector<int> &streams, const std::vector<uint8_t> &records)
    {
        check(nnn_batch_import_streams(b_.get(), streams.data(), (int)streams.size(), records.data(), records.size()));
    }
    // hold and resume (nnn_batch_hold_streams): held streams sit out the processing calls -- state parked, input not read, output and VAD
    // rows left as they were, no work done for blocks of streams that are all held -- and continue bit for bit when resumed
    void hold_streams(const std::vector<int> &streams) { check(nnn_batch_hold_streams(b_.get(), streams.data(), (int)streams.size())); }
    void resume_streams(const std::vector<int> &streams) { check(nnn_batch_resume_streams(b_.get(), streams.data(), (int)streams.size())); }
    int num_held() const { return nnn_batch_num_held(b_.get()); }
    std::vector<uint8_t> held() const   // [num_streams()]: 1 = held
    {
        std::vector<uint8_t> m((size_t)num_streams());
        check(nnn_batch_held_mask(b_.get(), m.data(), m.size()));
        return m;
    }
    // gain floors (nnn_batch_set_gain_floor): in every processing call a non-silent frame's raw network gain becomes max(gain, floor) before
    // the pitch filter and the smoothing see it.  floors: one value per listed stream (all its 22 bands) or 22 per stream; 0 = off.
    // Configuration, not state: resets, imports, hold / resume and load_state leave the floors alone, clone() copies them.
    static float attenuation_limit_db(float db) { return std::pow(10.0f, -db / 20.0f); }   // "never more than db dB down" as a floor
    void set_gain_floor(const std::vector<int> &streams, const std::vector<float> &floors)
    {
        const int bands = floors.size() == streams.size() * 22 && !streams.empty() ? 22 : 1;
        if (floors.size() != streams.size() * (size_t)bands) throw std::invalid_argument("set_gain_floor: 1 or 22 floors per listed stream");
        check(nnn_batch_set_gain_floor(b_.get(), streams.data(), (int)streams.size(), floors.data(), bands));
    }
    std::vector<float> gain_floor(const std::vector<int> &streams) const   // [streams.size() * 22]
    {
        std::vector<float> f(streams.size() * 22);
        check(nnn_batch_get_gain_floor(b_.get(), streams.data(), (int)streams.size(), f.data()));
        return f;
    }
    int num_floored() const { return nnn_batch_num_floored(b_.get()); }
    // channel link (nnn_batch_set_channel_link): the streams of group s / channels -- the channels of one stereo or four-channel group at the
    // PCM boundary -- get one common gain per band, the largest (NNN_LINK_MAX) or smallest (NNN_LINK_MIN) of their network outputs, before
    // the floor, the pitch filter and the smoothing see it; silent frames and held streams neither give nor take.  channels 2 or 4;
    // channels 1 or NNN_LINK_OFF: off.  Configuration, not state: resets, imports, hold / resume and load_state leave it alone, clone()
    // copies it.
    void set_channel_link(int channels, nnn_link_mode mode = NNN_LINK_MAX) { check(nnn_batch_set_channel_link(b_.get(), channels, (int)mode)); }
    std::pair<int, nnn_link_mode> channel_link() const   // (1, NNN_LINK_OFF) while off
    {
        int channels = 1, mode = NNN_LINK_OFF;
        check(nnn_batch_get_channel_link(b_.get(), &channels, &mode));
        return {channels, (nnn_link_mode)mode};
    }
    // records in device memory, asynchronous on hip_stream (nullptr: the batch's own stream)
    void export_streams_device(const std::vector<int> &streams, void *d_dst, void *hip_stream = nullptr)
    {
        check(nnn_batch_export_streams_device(b_.get(), streams.data(), (int)streams.size(), d_dst, hip_stream));
    }
    void import_streams_device(const std::vector<int> &streams, const void *d_src, void *hip_stream = nullptr)
    {
        check(nnn_batch_import_streams_device(b_.get(), streams.data(), (int)streams.size(), d_src, hip_stream));
    }
    nnn_batch *raw() { return b_.get(); }

  private:
    explicit BatchDenoiser(nnn_batch *owned) : b_(owned, nnn_batch_destroy) {}
    static void check(int rc)
    {
        if (rc) throw std::runtime_error(std::string("nnnoiseless: ") + nnn_last_error());
    }
    std::shared_ptr<nnn_batch> b_;
};

// the per-frame body of the reference's training-data generator (src/training.rs:113-160) for n_streams triples
class TrainingFeatures {
  public:
    static constexpr int ROW_WIDTH = NNN_TRAIN_COLS;
    explicit TrainingFeatures(int n_streams, int device = 0) : t_(nnn_train_create(n_streams, device), nnn_train_destroy), n_streams_(n_streams)
    {
        if (!t_) throw std::runtime_error(std::string("nnnoiseless: ") + nnn_last_error());
    }
    // host buffers: signal / noise / combined [n_streams][n_frames][480]; cutoff, vad [n_frames][n_streams]; rows [..][87]
    void process(const float *signal, const float *noise, const float *combined, const int32_t *cutoff, const float *vad,
                 float *rows, int n_frames)
    {
        if (nnn_train_process_host(t_.get(), signal, noise, combined, cutoff, vad, rows, n_frames))
            throw std::runtime_error(std::string("nnnoiseless: ") + nnn_last_error());
    }
    void reset() { nnn_train_reset(t_.get()); }
    int num_streams() const { return n_streams_; }
    nnn_train *raw() { return t_.get(); }

  private:
    friend class NoiseSimulator;
    std::shared_ptr<nnn_train> t_;
    int n_streams_ = 0;
};

// the generator's NoiseSimulator (src/training.rs:263-422) for every triple of a TrainingFeatures, on the device (nnn_sim.h): two int16
// arenas of clips, per-frame offsets [n_frames][n_streams] in, training rows (or the three signals and the two labels) out
class NoiseSimulator {
  public:
    using Params = nnn_sim_params;
    static Params default_params() { return Params{1.0f, 1.0f, {0, 0}, {0, 0}, {0, 0}, {0, 0}, 21}; }   // NoiseSimulator::new
    explicit NoiseSimulator(TrainingFeatures &features) : t_(features.t_), s_(nnn_sim_create(features.t_.get()), nnn_sim_destroy)
    {
        if (!s_) throw std::runtime_error(std::string("nnnoiseless: ") + nnn_last_error());
    }
    void load_signal(const int16_t *pcm, uint64_t elems) { check(nnn_sim_load(s_.get(), NNN_SIM_ARENA_SIGNAL, pcm, elems)); }
    void load_noise(const int16_t *pcm, uint64_t elems) { check(nnn_sim_load(s_.get(), NNN_SIM_ARENA_NOISE, pcm, elems)); }
    void adopt_device(int which, const int16_t *d_pcm, uint64_t elems) { check(nnn_sim_adopt_device(s_.get(), which, d_pcm, elems)); }
    void set_params(const std::vector<int> &streams, const std::vector<Params> &recs)
    {
        if (streams.size() != recs.size()) throw std::invalid_argument("nnnoiseless: one record per listed stream");
        check(nnn_sim_set_params(s_.get(), streams.data(), (int)streams.size(), recs.data()));
    }
    std::vector<Params> params(const std::vector<int> &streams)
    {
        std::vector<Params> recs(streams.size());
        check(nnn_sim_get_params(s_.get(), streams.data(), (int)streams.size(), recs.data()));
        return recs;
    }
    // host buffers: rows [n_frames][n_streams][87]; an offset that leaves its arena refuses the call
    void process(const uint64_t *sig_off, const uint64_t *noise_off, float *rows, int n_frames)
    {
        check(nnn_sim_process_host(s_.get(), sig_off, noise_off, rows, n_frames));
    }
    // host buffers: signal / noise / combined [n_streams][n_frames][480]; cutoff, vad [n_frames][n_streams]
    void signals(const uint64_t *sig_off, const uint64_t *noise_off, float *signal, float *noise, float *combined, int32_t *cutoff, float *vad,
                 int n_frames)
    {
        check(nnn_sim_signals_host(s_.get(), sig_off, noise_off, signal, noise, combined, cutoff, vad, n_frames));
    }
    // raw device pointers, asynchronous on hip_stream (nullptr = the training object's own stream)
    void process_device(const uint64_t *d_sig_off, const uint64_t *d_noise_off, float *d_rows, int n_frames, void *hip_stream = nullptr)
    {
        check(nnn_sim_process_device(s_.get(), d_sig_off, d_noise_off, d_rows, n_frames, hip_stream));
    }
    void signals_device(const uint64_t *d_sig_off, const uint64_t *d_noise_off, float *d_signal, float *d_noise, float *d_combined,
                        int32_t *d_cutoff, float *d_vad, int n_frames, size_t stream_stride, size_t frame_stride, void *hip_stream = nullptr)
    {
        check(nnn_sim_signals_device(s_.get(), d_sig_off, d_noise_off, d_signal, d_noise, d_combined, d_cutoff, d_vad, n_frames, stream_stride,
                                     frame_stride, hip_stream));
    }
    void reset() { check(nnn_sim_reset(s_.get())); }   // pair with TrainingFeatures::reset
    bool fault() { return nnn_sim_fault(s_.get()) > 0; }
    nnn_sim *raw() { return s_.get(); }

  private:
    static void check(int rc)
    {
        if (rc) throw std::runtime_error(std::string("nnnoiseless: ") + nnn_last_error());
    }
    std::shared_ptr<nnn_train> t_;   // (the simulator borrows the training object: kept alive here, destroyed after s_)
    std::shared_ptr<nnn_sim> s_;
};

// the reference's train/rnn_train.py and dump_rnn.py on the device (nnn_fit.h): forward pass, loss, BPTT and Adam for the 3-GRU network
// over windows of consecutive training rows; host buffers are dense [window][n_seq][...]
class Trainer {
  public:
    using Settings = nnn_fit_settings;
    using Rows = nnn_fit_rows;
    struct Losses { float total, gain, vad, reg, msse; };
    // template_rnn empty: the reference's training set-up with zero parameters, to be overwritten by set_params
    explicit Trainer(const std::vector<uint8_t> &template_rnn = {}, int max_seq = 32, int max_window = 2000, int device = 0)
        : f_(nnn_fit_create(template_rnn.empty() ? nullptr : template_rnn.data(), template_rnn.size(), max_seq, max_window, device), nnn_fit_destroy)
    {
        if (!f_) throw std::runtime_error(std::string("nnnoiseless: ") + nnn_last_error());
    }
    std::vector<float> get(int which = NNN_FIT_SEL_PARAMS)
    {
        std::vector<float> v(NNN_FIT_PARAMS);
        check(nnn_fit_get(f_.get(), which, v.data()));
        return v;
    }
    void set(const std::vector<float> &v, int which = NNN_FIT_SEL_PARAMS)
    {
        if (v.size() != (size_t)NNN_FIT_PARAMS) throw std::invalid_argument("nnnoiseless: a parameter vector holds NNN_FIT_PARAMS values");
        check(nnn_fit_set(f_.get(), which, v.data()));
    }
    int64_t step_count()
    {
        int64_t n = 0;
        check(nnn_fit_get_step(f_.get(), &n));
        return n;
    }
    void set_step_count(int64_t n) { check(nnn_fit_set_step(f_.get(), n)); }
    Settings settings()
    {
        Settings s;
        check(nnn_fit_get_settings(f_.get(), &s));
        return s;
    }
    void set_settings(const Settings &s) { check(nnn_fit_set_settings(f_.get(), &s)); }
    std::vector<uint8_t> export_rnn()
    {
        std::vector<uint8_t> out(NNN_FIT_RNN_BYTES);
        check(nnn_fit_export_rnn(f_.get(), out.data(), out.size()));
        return out;
    }
    void forward(const float *rows, int n_seq, int window, float *gains, float *vad) { check(nnn_fit_forward_host(f_.get(), rows, n_seq, window, gains, vad)); }
    Losses loss(const float *rows, const float *w, int n_seq, int window)
    {
        check(nnn_fit_loss_host(f_.get(), rows, w, n_seq, window));
        return losses();
    }
    Losses grad(const float *rows, const float *w, int n_seq, int window)
    {
        check(nnn_fit_grad_host(f_.get(), rows, w, n_seq, window));
        return losses();
    }
    // raw device pointers, asynchronous on hip_stream (nullptr = the trainer's own stream)
    void forward_device(const Rows &r, float *d_gains, float *d_vad, void *hip_stream = nullptr) { check(nnn_fit_forward_device(f_.get(), &r, d_gains, d_vad, hip_stream)); }
    void loss_device(const Rows &r, void *hip_stream = nullptr) { check(nnn_fit_loss_device(f_.get(), &r, hip_stream)); }
    void grad_device(const Rows &r, void *hip_stream = nullptr) { check(nnn_fit_grad_device(f_.get(), &r, hip_stream)); }
    void step(void *hip_stream = nullptr) { check(nnn_fit_step(f_.get(), hip_stream)); }
    Losses losses()
    {
        float v[5];
        check(nnn_fit_losses(f_.get(), v));
        return Losses{v[0], v[1], v[2], v[3], v[4]};
    }
    nnn_fit *raw() { return f_.get(); }

  private:
    static void check(int rc)
    {
        if (rc) throw std::runtime_error(std::string("nnnoiseless: ") + nnn_last_error());
    }
    std::shared_ptr<nnn_fit> f_;
};

// per-stream sums between a reference and a test signal, carried across calls on the device (nnn_score.h): A = sum r^2, B = sum y^2,
// C = sum r y, E = sum (r - y)^2 in f64, in one fixed order; SNR and SI-SDR are host arithmetic on them
class Scorer {
  public:
    struct Totals {
        std::vector<double> sums;        // [n_streams][4]: A, B, C, E
        std::vector<uint64_t> frames;    // [n_streams]
    };
    explicit Scorer(int n_streams, int max_delay = NNN_SCORE_MAX_DELAY, int device = 0)
        : n_(n_streams), h_(nnn_score_create(n_streams, max_delay, device), nnn_score_destroy)
    {
        if (!h_) throw std::runtime_error(std::string("nnnoiseless: ") + nnn_last_error());
    }
    int num_streams() const { return n_; }
    // delays of the listed streams (idx empty: one per stream); also zeroes their history, totals and count
    void set_delay(const std::vector<int> &idx, const std::vector<int32_t> &delays)
    {
        if (delays.size() != (idx.empty() ? (size_t)n_ : idx.size())) throw std::invalid_argument("nnnoiseless: one delay per listed stream");
        check(nnn_score_set_delay(h_.get(), idx.empty() ? nullptr : idx.data(), (int)delays.size(), delays.data()));
    }
    std::vector<int32_t> delay()
    {
        std::vector<int32_t> d((size_t)n_);
        check(nnn_score_get_delay(h_.get(), nullptr, n_, d.data()));
        return d;
    }
    // idx empty: every stream
    void reset(const std::vector<int> &idx = {}) { check(nnn_score_reset(h_.get(), idx.empty() ? nullptr : idx.data(), (int)idx.size())); }
    // host memory, dense [n_streams][n_frames][480]; valid nullptr or [n_frames][n_streams]; frame_sums nullptr or [n_frames][n_streams][4]
    void accumulate(const float *ref, const float *test, int n_frames, const uint8_t *valid = nullptr, double *frame_sums = nullptr)
    {
        check(nnn_score_accumulate_host(h_.get(), ref, test, valid, frame_sums, n_frames));
    }
    // raw device pointers, asynchronous on hip_stream (nullptr = the scorer's own stream); strides in floats
    void accumulate_device(const float *d_ref, const float *d_test, int n_frames, size_t stream_stride, size_t frame_stride,
                           const uint8_t *d_valid = nullptr, double *d_frame_sums = nullptr, void *hip_stream = nullptr)
    {
        check(nnn_score_accumulate_device(h_.get(), d_ref, d_test, d_valid, d_frame_sums, n_frames, stream_stride, frame_stride, hip_stream));
    }
    Totals totals()
    {
        Totals t{std::vector<double>((size_t)n_ * NNN_SCORE_SUMS), std::vector<uint64_t>((size_t)n_)};
        check(nnn_score_totals(h_.get(), t.sums.data(), t.frames.data()));
        return t;
    }
    void totals_device(double *d_out, uint64_t *d_counts, void *hip_stream = nullptr) { check(nnn_score_totals_device(h_.get(), d_out, d_counts, hip_stream)); }
    // the figures, as nnnoiseless_amd/score.py has them: inf or nan for zero denominators, as IEEE division and log10 give
    static double snr_db(double A, double E) { return 10.0 * std::log10(A / E); }
    static double si_sdr_db(double A, double B, double C) { return 10.0 * std::log10(C * C / (A * B - C * C)); }
    nnn_score *raw() { return h_.get(); }

  private:
    static void check(int rc)
    {
        if (rc) throw std::runtime_error(std::string("nnnoiseless: ") + nnn_last_error());
    }
    int n_;
    std::shared_ptr<nnn_score> h_;
};

// the VAD gate behind the denoiser (nnn_gate.h): per stream a threshold on the speech probability, a grace period, a look-back that delays
// the audio a few frames so the onset is not cut, and a gain for the closed gate (0 = mute); the rule is exact and stated in the header
class VadGate {
  public:
    explicit VadGate(int n_streams, int max_lookback = 0, int device = 0)
        : n_(n_streams), h_(nnn_gate_create(n_streams, max_lookback, device), nnn_gate_destroy)
    {
        if (!h_) throw std::runtime_error(std::string("nnnoiseless: ") + nnn_last_error());
    }
    int num_streams() const { return n_; }
    // parameters of the listed streams (idx empty: one per stream); also resets those streams
    void set_params(const std::vector<nnn_gate_params> &params, const std::vector<int> &idx = {})
    {
        if (params.size() != (idx.empty() ? (size_t)n_ : idx.size())) throw std::invalid_argument("nnnoiseless: one parameter record per listed stream");
        check(nnn_gate_set_params(h_.get(), idx.empty() ? nullptr : idx.data(), (int)params.size(), params.data()));
    }
    // the same parameters for every stream
    void set_params(float threshold, int grace, int lookback, float level)
    {
        set_params(std::vector<nnn_gate_params>((size_t)n_, nnn_gate_params{threshold, grace, lookback, level}));
    }
    std::vector<nnn_gate_params> params()
    {
        std::vector<nnn_gate_params> p((size_t)n_);
        check(nnn_gate_get_params(h_.get(), nullptr, n_, p.data()));
        return p;
    }
    // idx empty: every stream
    void reset(const std::vector<int> &idx = {}) { check(nnn_gate_reset(h_.get(), idx.empty() ? nullptr : idx.data(), (int)idx.size())); }
    // host memory, dense [n_streams][n_frames][480] (out may be in); vad [n_frames][n_streams]; live nullptr or [n_streams]; open nullptr or
    // [n_frames][n_streams]
    void apply(const float *in, float *out, const float *vad, int n_frames, const uint8_t *live = nullptr, uint8_t *open = nullptr)
    {
        check(nnn_gate_apply_host(h_.get(), in, out, vad, live, open, n_frames));
    }
    // raw device pointers, asynchronous on hip_stream (nullptr = the gate's own stream); strides in floats; d_out == d_in is in place
    void apply_device(const float *d_in, float *d_out, const float *d_vad, int n_frames, size_t stream_stride, size_t frame_stride,
                      const uint8_t *d_live = nullptr, uint8_t *d_open = nullptr, void *hip_stream = nullptr)
    {
        check(nnn_gate_apply_device(h_.get(), d_in, d_out, d_vad, d_live, d_open, n_frames, stream_stride, frame_stride, hip_stream));
    }
    // the packed boundary of BatchDenoiser::process_pcm_device
    void apply_pcm_device(const void *d_in, void *d_out, const float *d_vad, int n_frames, const nnn_pcm_layout &layout, const uint8_t *d_live = nullptr,
                          uint8_t *d_open = nullptr, void *hip_stream = nullptr)
    {
        check(nnn_gate_apply_pcm_device(h_.get(), d_in, d_out, d_vad, d_live, d_open, n_frames, &layout, hip_stream));
    }
    // records of NNN_GATE_STATE_BYTES bytes each: a stream moved to another gate continues bit for bit
    std::vector<uint8_t> export_streams(const std::vector<int> &idx)
    {
        std::vector<uint8_t> rec(idx.size() * (size_t)NNN_GATE_STATE_BYTES);
        check(nnn_gate_export_streams(h_.get(), idx.data(), (int)idx.size(), rec.data(), rec.size()));
        return rec;
    }
    void import_streams(const std::vector<int> &idx, const std::vector<uint8_t> &records)
    {
        check(nnn_gate_import_streams(h_.get(), idx.data(), (int)idx.size(), records.data(), records.size()));
    }
    nnn_gate *raw() { return h_.get(); }

  private:
    static void check(int rc)
    {
        if (rc) throw std::runtime_error(std::string("nnnoiseless: ") + nnn_last_error());
    }
    int n_;
    std::shared_ptr<nnn_gate> h_;
};

// the conference mixer behind the gate (nnn_mix.h): per stream a room and a gain; every live member of a room receives the sum of the room's
// other talkers (mix-minus); the rule is exact and stated in the header
class Mixer {
  public:
    explicit Mixer(int n_streams, int device = 0) : n_(n_streams), h_(nnn_mix_create(n_streams, device), nnn_mix_destroy)
    {
        if (!h_) throw std::runtime_error(std::string("nnnoiseless: ") + nnn_last_error());
    }
    int num_streams() const { return n_; }
    // rooms (-1 = alone) and gains (0 .. NNN_MIX_MAX_GAIN) of the listed streams (idx empty: one per stream), in force from the next call;
    // set_rooms leaves the ramp state alone: mute a stream before moving it
    void set_rooms(const std::vector<int32_t> &room, const std::vector<int> &idx = {})
    {
        if (room.size() != (idx.empty() ? (size_t)n_ : idx.size())) throw std::invalid_argument("nnnoiseless: one room per listed stream");
        check(nnn_mix_set_rooms(h_.get(), idx.empty() ? nullptr : idx.data(), (int)room.size(), room.data()));
    }
    void set_gains(const std::vector<float> &gain, const std::vector<int> &idx = {})
    {
        if (gain.size() != (idx.empty() ? (size_t)n_ : idx.size())) throw std::invalid_argument("nnnoiseless: one gain per listed stream");
        check(nnn_mix_set_gains(h_.get(), idx.empty() ? nullptr : idx.data(), (int)gain.size(), gain.data()));
    }
    std::vector<int32_t> rooms()
    {
        std::vector<int32_t> r((size_t)n_);
        check(nnn_mix_get_rooms(h_.get(), nullptr, n_, r.data()));
        return r;
    }
    std::vector<float> gains()
    {
        std::vector<float> g((size_t)n_);
        check(nnn_mix_get_gains(h_.get(), nullptr, n_, g.data()));
        return g;
    }
    // idx empty: every stream
    void reset(const std::vector<int> &idx = {}) { check(nnn_mix_reset(h_.get(), idx.empty() ? nullptr : idx.data(), (int)idx.size())); }
    // host memory, dense [n_streams][n_frames][480] (out must not be in); talk nullptr or [n_frames][n_streams] (the gate's open flags); live
    // nullptr or [n_streams]; heard nullptr or [n_frames][n_streams]
    void apply(const float *in, float *out, int n_frames, const uint8_t *talk = nullptr, const uint8_t *live = nullptr, int32_t *heard = nullptr)
    {
        check(nnn_mix_apply_host(h_.get(), in, out, talk, live, heard, n_frames));
    }
    // raw device pointers, asynchronous on hip_stream (nullptr = the mixer's own stream); strides in floats, a pair per side; never in place
    void apply_device(const float *d_in, float *d_out, int n_frames, size_t in_stream_stride, size_t in_frame_stride, size_t out_stream_stride,
                      size_t out_frame_stride, const uint8_t *d_talk = nullptr, const uint8_t *d_live = nullptr, int32_t *d_heard = nullptr,
                      void *hip_stream = nullptr)
    {
        check(nnn_mix_apply_device(h_.get(), d_in, d_out, d_talk, d_live, d_heard, n_frames, in_stream_stride, in_frame_stride, out_stream_stride,
                                   out_frame_stride, hip_stream));
    }
    // the packed boundary of BatchDenoiser::process_pcm_device, a layout (and format) per side
    void apply_pcm_device(const void *d_in, void *d_out, int n_frames, const nnn_pcm_layout &in_layout, const nnn_pcm_layout &out_layout,
                          const uint8_t *d_talk = nullptr, const uint8_t *d_live = nullptr, int32_t *d_heard = nullptr, void *hip_stream = nullptr)
    {
        check(nnn_mix_apply_pcm_device(h_.get(), d_in, d_out, d_talk, d_live, d_heard, n_frames, &in_layout, &out_layout, hip_stream));
    }
    nnn_mix *raw() { return h_.get(); }

  private:
    static void check(int rc)
    {
        if (rc) throw std::runtime_error(std::string("nnnoiseless: ") + nnn_last_error());
    }
    int n_;
    std::shared_ptr<nnn_mix> h_;
};

// the talker picker between the gate and the mixer (nnn_pick.h): per stream a room and a pin, per object k, decay and stick; of every
// room's open gates the k loudest talk, an incumbent keeps its place until a challenger is stick times louder; the rule is exact and
// stated in the header
class Picker {
  public:
    explicit Picker(int n_streams, int device = 0) : n_(n_streams), h_(nnn_pick_create(n_streams, device), nnn_pick_destroy)
    {
        if (!h_) throw std::runtime_error(std::string("nnnoiseless: ") + nnn_last_error());
    }
    int num_streams() const { return n_; }
    // rooms (-1 = alone; the mixer's labels) and pins (0 or 1) of the listed streams (idx empty: one per stream), in force from the next call
    void set_rooms(const std::vector<int32_t> &room, const std::vector<int> &idx = {})
    {
        if (room.size() != (idx.empty() ? (size_t)n_ : idx.size())) throw std::invalid_argument("nnnoiseless: one room per listed stream");
        check(nnn_pick_set_rooms(h_.get(), idx.empty() ? nullptr : idx.data(), (int)room.size(), room.data()));
    }
    void set_pinned(const std::vector<uint8_t> &pinned, const std::vector<int> &idx = {})
    {
        if (pinned.size() != (idx.empty() ? (size_t)n_ : idx.size())) throw std::invalid_argument("nnnoiseless: one pin per listed stream");
        check(nnn_pick_set_pinned(h_.get(), idx.empty() ? nullptr : idx.data(), (int)pinned.size(), pinned.data()));
    }
    // k in 1 .. NNN_PICK_MAX_K, decay in [0, 1], stick in [1, NNN_PICK_MAX_STICK]
    void set_policy(int k, float decay, float stick) { check(nnn_pick_set_policy(h_.get(), k, decay, stick)); }
    std::vector<int32_t> rooms()
    {
        std::vector<int32_t> r((size_t)n_);
        check(nnn_pick_get_rooms(h_.get(), nullptr, n_, r.data()));
        return r;
    }
    std::vector<uint8_t> pinned()
    {
        std::vector<uint8_t> p((size_t)n_);
        check(nnn_pick_get_pinned(h_.get(), nullptr, n_, p.data()));
        return p;
    }
    void policy(int &k, float &decay, float &stick) { check(nnn_pick_get_policy(h_.get(), &k, &decay, &stick)); }
    // idx empty: every stream
    void reset(const std::vector<int> &idx = {}) { check(nnn_pick_reset(h_.get(), idx.empty() ? nullptr : idx.data(), (int)idx.size())); }
    // host memory: in dense [n_streams][n_frames][480]; talk [n_frames][n_streams] (what Mixer::apply takes as talk); open nullptr or
    // [n_frames][n_streams] (the gate's open flags); live nullptr or [n_streams]; dominant and level nullptr or [n_frames][n_streams]
    void select(const float *in, uint8_t *talk, int n_frames, const uint8_t *open = nullptr, const uint8_t *live = nullptr, int32_t *dominant = nullptr,
                double *level = nullptr)
    {
        check(nnn_pick_select_host(h_.get(), in, open, live, talk, dominant, level, n_frames));
    }
    // raw device pointers, asynchronous on hip_stream (nullptr = the picker's own stream); strides in floats; d_talk may be d_open itself
    void select_device(const float *d_in, uint8_t *d_talk, int n_frames, size_t stream_stride, size_t frame_stride, const uint8_t *d_open = nullptr,
                       const uint8_t *d_live = nullptr, int32_t *d_dominant = nullptr, double *d_level = nullptr, void *hip_stream = nullptr)
    {
        check(nnn_pick_select_device(h_.get(), d_in, d_open, d_live, d_talk, d_dominant, d_level, n_frames, stream_stride, frame_stride, hip_stream));
    }
    // the packed boundary of BatchDenoiser::process_pcm_device
    void select_pcm_device(const void *d_in, uint8_t *d_talk, int n_frames, const nnn_pcm_layout &layout, const uint8_t *d_open = nullptr,
                           const uint8_t *d_live = nullptr, int32_t *d_dominant = nullptr, double *d_level = nullptr, void *hip_stream = nullptr)
    {
        check(nnn_pick_select_pcm_device(h_.get(), d_in, d_open, d_live, d_talk, d_dominant, d_level, n_frames, &layout, hip_stream));
    }
    nnn_pick *raw() { return h_.get(); }

  private:
    static void check(int rc)
    {
        if (rc) throw std::runtime_error(std::string("nnnoiseless: ") + nnn_last_error());
    }
    int n_;
    std::shared_ptr<nnn_pick> h_;
};

class DenoiseState {
  public:
    static constexpr size_t FRAME_SIZE = NNN_FRAME_SIZE;
    static DenoiseState create(int device = 0) { return DenoiseState(nullptr, device); }                    // DenoiseState::new()
    static DenoiseState from_model(const RnnModel &m, int device = 0) { return DenoiseState(&m, device); }
    static DenoiseState with_model(const RnnModel &m, int device = 0) { return DenoiseState(&m, device); }
    // `out` may alias `in`; returns the VAD probability
    float process_frame(float *out, const float *in)
    {
        float vad = 0.f;
        b_.process(in, out, &vad, 1, FRAME_SIZE, FRAME_SIZE);
        return vad;
    }
    DenoiseState clone() const { return DenoiseState(b_.clone()); }   // #[derive(Clone)], src/denoise.rs:36
    // this state as a portable record (NNN_STREAM_STATE_BYTES), and a state that continues from one (a batch slot's export_streams)
    std::vector<uint8_t> export_state() const { return b_.export_streams({0}); }
    static DenoiseState from_state(const std::vector<uint8_t> &record, const RnnModel *m = nullptr, int device = 0)
    {
        DenoiseState s(m, device);
        s.b_.import_streams({0}, record);
        return s;
    }

  private:
    DenoiseState(const RnnModel *m, int device) : b_(BatchDenoiser::sized(1, 1, m, device)) {}   // one frame per call: sized for it
    explicit DenoiseState(BatchDenoiser b) : b_(std::move(b)) {}
    BatchDenoiser b_;
};

// n mono streams of one common sample rate -> 48 kHz with the CLI's 16-tap windowed sinc (src/nnnoiseless.rs:19-32, 106-131)
class Resampler {
  public:
    Resampler(int n_streams, double source_rate, int device = 0)
        : r_(nnn_resampler_create(n_streams, source_rate / 48000.0, device), nnn_resampler_destroy)
    {
        if (!r_) throw std::runtime_error(std::string("nnnoiseless: ") + nnn_last_error());
    }
    long max_output(long n_in) const { return nnn_resampler_max_output(r_.get(), n_in); }
    // host buffers, dense [n_streams][n_in] -> [n_streams][cap_out]; returns the samples produced per stream
    long process(const float *in, long n_in, float *out, long cap_out)
    {
        long n = 0;
        if (nnn_resampler_process_host(r_.get(), in, n_in, out, cap_out, &n)) throw std::runtime_error(std::string("nnnoiseless: ") + nnn_last_error());
        return n;
    }
    void reset() { nnn_resampler_reset(r_.get()); }

  private:
    std::shared_ptr<nnn_resampler> r_;
};

// Streams at another sample rate in and out of a 48 kHz batch (include/nnn_rate.h): the CLI's resampler in front of the batch's ordinary
// call and the same interpolator at the inverse ratio behind it, one asynchronous call; the adapter carries the partial frame and
// both legs' histories.  It borrows the batch, which must outlive it.
class RateAdapter {
  public:
    RateAdapter(BatchDenoiser &batch, double source_rate, long max_in) : a_(nnn_rate_create(batch.raw(), source_rate, max_in), nnn_rate_destroy)
    {
        if (!a_) throw std::runtime_error(std::string("nnnoiseless: ") + nnn_last_error());
    }
    long max_output(long n_in) const { return nnn_rate_max_output(a_.get(), n_in); }
    int max_frames(long n_in) const { return nnn_rate_max_frames(a_.get(), n_in); }
    long carried() const { return nnn_rate_carried(a_.get()); }
    struct Counts {
        long n_out;     // source-rate samples per stream the call returned
        int n_frames;   // frames (VAD rows) it completed
    };
    // host buffers, dense [n_streams][n_in] -> [n_streams][cap_out], vad [cap_frames][n_streams] (may be null); format NNN_PCM_F32 or NNN_PCM_I16
    Counts process(const void *in, long n_in, void *out, long cap_out, float *vad, int cap_frames, int format = NNN_PCM_F32)
    {
        Counts c = {0, 0};
        check(nnn_rate_process_host(a_.get(), in, n_in, out, cap_out, &c.n_out, vad, cap_frames, &c.n_frames, format));
        return c;
    }
    // device buffers, strides in elements of the format; asynchronous on hip_stream (nullptr = the batch's own stream)
    Counts process_device(const void *d_in, long n_in, size_t in_stride, void *d_out, long cap_out, size_t out_stride, float *d_vad, int cap_frames,
                          int format = NNN_PCM_F32, void *hip_stream = nullptr)
    {
        Counts c = {0, 0};
        check(nnn_rate_process_device(a_.get(), d_in, n_in, in_stride, d_out, cap_out, out_stride, &c.n_out, d_vad, cap_frames, &c.n_frames, format, hip_stream));
        return c;
    }
    void reset() { check(nnn_rate_reset(a_.get())); }
    // beside BatchDenoiser::reset_streams: the listed streams' histories and carried samples cleared from the next call on
    void reset_streams(const std::vector<int> &streams) { check(nnn_rate_reset_streams(a_.get(), streams.data(), (int)streams.size())); }

  private:
    static void check(int rc)
    {
        if (rc) throw std::runtime_error(std::string("nnnoiseless: ") + nnn_last_error());
    }
    std::shared_ptr<nnn_rate> a_;
};

// Files of unequal length through one batch, slots refilled (include/nnn_pack.h): every file gets, bit for bit, what the reference CLI's loop
// gives it alone -- whole frames only, the first one processed and not written -- while the batch runs full.  It borrows the batch, which
// must outlive it, have one model and nothing held; a run leaves it with every stream it used reset and nothing held.
class FilePacker {
  public:
    using Summary = std::array<int64_t, 8>;   // steps, useful, padded, held steps, launched, held frames, files placed, largest padding of a file
    FilePacker(BatchDenoiser &batch, int channels = 1, int step_frames = 0) : p_(nnn_pack_create(batch.raw(), channels, step_frames), nnn_pack_destroy)
    {
        if (!p_) throw std::runtime_error(std::string("nnnoiseless: ") + nnn_last_error());
    }
    // the plan of a run over files of `frames` WHOLE frames, in slot units: pure host arithmetic, no batch, no device
    static Summary plan(int n_slots, int step_frames, const std::vector<uint64_t> &frames, std::vector<int32_t> *slot_of_file = nullptr,
                        std::vector<int32_t> *first_step_of_file = nullptr)
    {
        Summary s = {};
        if (slot_of_file) slot_of_file->assign(frames.size(), -1);
        if (first_step_of_file) first_step_of_file->assign(frames.size(), -1);
        check(nnn_pack_plan(n_slots, step_frames, frames.data(), (int)frames.size(), slot_of_file ? slot_of_file->data() : nullptr,
                            first_step_of_file ? first_step_of_file->data() : nullptr, s.data()));
        return s;
    }
    // host arenas (synchronous); offsets of `files` in elements of the arena's format; in_format NNN_PCM_F32 / NNN_PCM_I16 / NNN_PACK_*,
    // out_format NNN_PCM_F32 / NNN_PCM_I16; vad may be null.  Returns the run's summary in stream units.
    Summary run(const void *in, uint64_t in_elems, int in_format, void *out, uint64_t out_elems, int out_format, float *vad, uint64_t vad_elems,
                const std::vector<nnn_pack_file> &files)
    {
        check(nnn_pack_run_host(p_.get(), in, in_elems, in_format, out, out_elems, out_format, vad, vad_elems, files.data(), (int)files.size()));
        return last_summary();
    }
    // device arenas; asynchronous on hip_stream (nullptr = the batch's own stream)
    Summary run_device(const void *d_in, uint64_t in_elems, int in_format, void *d_out, uint64_t out_elems, int out_format, float *d_vad,
                       uint64_t vad_elems, const std::vector<nnn_pack_file> &files, void *hip_stream = nullptr)
    {
        check(nnn_pack_run_device(p_.get(), d_in, in_elems, in_format, d_out, out_elems, out_format, d_vad, vad_elems, files.data(), (int)files.size(),
                                  hip_stream));
        return last_summary();
    }
    Summary last_summary() const
    {
        Summary s = {};
        check(nnn_pack_last_summary(p_.get(), s.data()));
        return s;
    }

  private:
    static void check(int rc)
    {
        if (rc) throw std::runtime_error(std::string("nnnoiseless: ") + nnn_last_error());
    }
    std::shared_ptr<nnn_pack> p_;
};


// All the GPUs of a node behind one object (include/nnn_node.h): contiguous stream shards, one batch and one host thread per device.
class NodeDenoiser {
  public:
    NodeDenoiser(int n_streams, const std::vector<int> &devices, const RnnModel *model = nullptr, int max_group_frames = 0)
    {
        nnn_batch_opts o = {};
        o.max_group_frames = max_group_frames;
        n_ = nnn_node_create(model ? model->raw() : nullptr, n_streams, devices.data(), (int)devices.size(), max_group_frames ? &o : nullptr);
        if (!n_) throw std::runtime_error(std::string("nnnoiseless: ") + nnn_last_error());
    }
    ~NodeDenoiser() { nnn_node_destroy(n_); }
    NodeDenoiser(const NodeDenoiser &) = delete;
    NodeDenoiser &operator=(const NodeDenoiser &) = delete;
    int num_streams() const { return nnn_node_num_streams(n_); }
    int num_shards() const { return nnn_node_num_shards(n_); }
    // in / out: [n_streams][n_frames][480], vad: [n_frames][n_streams] (may be null); every device works on its share at once
    void process(const float *in, float *out, float *vad, int n_frames)
    {
        if (nnn_node_process_host(n_, in, out, vad, n_frames, (size_t)n_frames * NNN_FRAME_SIZE, NNN_FRAME_SIZE))
            throw std::runtime_error(std::string("nnnoiseless: ") + nnn_last_error());
    }
    // buffers resident on the shards' own devices, one pointer (and optionally one hipStream_t) per shard; asynchronous: synchronize()
    void process_device(const std::vector<const float *> &d_in, const std::vector<float *> &d_out, const std::vector<float *> &d_vad, int n_frames,
                        size_t stream_stride, size_t frame_stride, const std::vector<void *> &hip_streams = {})
    {
        const int n = num_shards();
        if ((int)d_in.size() != n || (int)d_out.size() != n || (!d_vad.empty() && (int)d_vad.size() != n) || (!hip_streams.empty() && (int)hip_streams.size() != n))
            throw std::invalid_argument("nnnoiseless: one table entry per shard");
        if (nnn_node_process_device_streams(n_, d_in.data(), d_out.data(), d_vad.empty() ? nullptr : d_vad.data(),
                                            hip_streams.empty() ? nullptr : hip_streams.data(), n, n_frames, stream_stride, frame_stride))
            throw std::runtime_error(std::string("nnnoiseless: ") + nnn_last_error());
    }
    void synchronize()
    {
        if (nnn_node_synchronize(n_)) throw std::runtime_error(std::string("nnnoiseless: ") + nnn_last_error());
    }
    // the CPUs shard i's host thread is pinned to (its device's local CPUs), "" when not pinned
    std::string shard_cpus(int i) const { return nnn_node_shard_cpus(n_, i); }
    // after a call that failed on some shard the node refuses further calls until reset() (the shards sit at different frame counts)
    void reset()
    {
        if (nnn_node_reset(n_)) throw std::runtime_error(std::string("nnnoiseless: ") + nnn_last_error());
    }
    bool fault() const { return nnn_node_fault(n_) != 0; }
    nnn_node *raw() { return n_; }

  private:
    nnn_node *n_ = nullptr;
};

}  // namespace nnnoiseless
